"""Patch-wise query strategies of the scored path (reference: PW_NNAL.py): the branches of CNN_query / query_multimg,
the uncertainty filters and gen_A_matrices, with the reference's signatures.  `sess` is a device.DeviceSession, `model` a device.DeviceModel."""
from collections import OrderedDict

import numpy as np

from . import NNAL_tools, PW_NN, patch_utils


def binary_uncertainty_filter(posts, B):
    """PW_NNAL.py:671-681: the B posteriors closest to 0.5 (ties: lower index first)."""
    return np.argsort(np.abs(np.array(posts) - 0.5), kind='stable')[:B]


def device_uncertainty_filter(sess, posts, B, with_keys=False):
    """Same selection on the device (alq_score_entropy + alq_topk_uncertain) for posteriors that
    are already resident: `posts` float32 device tensor [n] -> int64 device tensor [B]
    (with_keys: also their keys |p - .5| as a float64 device tensor [B], ascending)."""
    from ._lib import check, ptr
    torch = sess.torch
    sess.bind_stream()
    n = int(posts.numel())
    B = min(int(B), n)
    keys = sess.empty((n,), torch.float64)
    check(sess.lib.alq_score_entropy(sess.ctx, ptr(posts), n, ptr(keys), None))
    out = sess.topk_smallest(keys, B)
    if with_keys:
        return out, keys.index_select(0, out)
    return out


def pool_posteriors_device(expr, model, sess, all_padded_imgs, pool_inds, x_feed_dict={}, _vols=None):
    """The device sweep of bin_uncertainty_filter_multimg: the class-1 posteriors of THIS rank's block [a, b) of the
    concatenated pool (pool_shard.work_block; everything in one process) as a float32 device tensor, in concatenated
    subject order, per-subject stats from expr.train_stats, batch_eval's gather and passes.  Returns (a, b, p1).
    `_vols`: a dict subject -> patch_utils.DeviceVolumes the caller keeps across calls (filled on first use)."""
    from . import pool_shard
    sizes = [len(p) for p in pool_inds]
    m = len(all_padded_imgs[0]) - 1
    n = int(np.sum(sizes))
    a, b = pool_shard.work_block(n)
    p1 = sess.empty((b - a,), sess.torch.float32)
    off = 0
    for i in range(len(pool_inds)):
        lo, hi = max(a, off) - off, min(b, off + sizes[i]) - off      # this rank's part of subject i, local positions
        if hi > lo:
            stats = [[expr.train_stats[i, 2 * j], expr.train_stats[i, 2 * j + 1]] for j in range(m)]
            v = None
            if _vols is not None:          # (not a reference argument) per-subject volumes the caller keeps on the device
                if i not in _vols:
                    _vols[i] = patch_utils.DeviceVolumes(sess, all_padded_imgs[i][:-1])
                v = _vols[i]
            PW_NN.posteriors_device(model, sess, all_padded_imgs[i][:-1], np.asarray(pool_inds[i])[lo:hi], expr.pars['patch_shape'],
                                    expr.pars['ntb'], stats, x_feed_dict, _vols=v, _first_sample=off + lo,
                                    out=p1[off + lo - a:off + hi - a])
        elif sizes[i] > 0:
            PW_NN.mc_dropout_args(model, x_feed_dict)       # another rank's subject: keep the RNG streams in step
        off += sizes[i]
    return a, b, p1


def bin_uncertainty_filter_multimg(expr, model, sess, all_padded_imgs, pool_inds, B, x_feed_dict={}, _vols=None):
    """PW_NNAL.py:684-736: posteriors of every subject's pool voxels (per-subject stats from
    expr.train_stats), then the B most uncertain over the concatenation, split back per subject.

    Under torch.distributed (one process per GPU, volumes replicated) every rank evaluates one contiguous block of the
    concatenated pool (pool_shard.work_block, pool_posteriors_device) and the posterior vector is assembled on every rank by
    one all-reduce of owner-filled entries (pool_shard.allgather_rows: x + 0.0 is exact), after which this function
    continues exactly as in one process - per-patch results do not depend on how the pool is cut into device passes."""
    from . import pool_shard
    s = len(pool_inds)
    sizes = [len(p) for p in pool_inds]
    n = int(np.sum(sizes))
    a, b, p1 = pool_posteriors_device(expr, model, sess, all_padded_imgs, pool_inds, x_feed_dict, _vols)
    allp = np.zeros(n)
    allp[a:b] = p1.cpu().numpy()
    if (a, b) != (0, n):
        allp = pool_shard.allgather_rows(n, np.arange(a, b), allp[a:b], sess)
    if len(x_feed_dict) > 0:
        return allp
    order = binary_uncertainty_filter(allp, B)
    sel_inds = patch_utils.global2local_inds(order, sizes)
    ends = np.cumsum(sizes)
    sel_posts = [allp[ends[i] - sizes[i]:ends[i]][sel_inds[i]] for i in range(s)]
    return sel_inds, sel_posts


def gen_A_matrices(expr, model, sess, sel_patches, sel_posts, diag_load=1e-5):
    """PW_NNAL.py:738-816: conditional Fisher matrices A_i = (1-p) g0 g0^T + p g1 g1^T + diag_load I
    of the (already normalised) patches, with the reference's saturation branches on `sel_posts`.
    Returns a list of float64 [L, L] arrays.  One batched device pass replaces the per-sample
    `sess.run(model.grad_posts[j])` + `shrink_gradient` loop."""
    sel_posts = np.asarray(sel_posts, dtype=np.float64)
    n = len(sel_posts)
    if n == 0:
        return []
    x = np.asarray(sel_patches)
    res = model.fisher(x.reshape((n,) + model.in_shape), p1=sel_posts, diag_load=diag_load)
    idx = list(getattr(model, 'grad_layer_idx', range(model.L)))
    if idx == list(range(model.L)):
        return [res['A'][i] for i in range(n)]
    # `grad_layers` subset (NN.py:627-633): A_size = len(grad_posts['1'])/2 (:751), the shrunk gradients of those layers
    # only; the same host formula as the reference (:810-814) on the device's g0, g1
    p = np.where(sel_posts < 1e-6, 0., np.where(sel_posts > 1 - 1e-6, 1., sel_posts))
    g0, g1 = res['g0'][:, idx], res['g1'][:, idx]
    eye = np.eye(len(idx)) * diag_load
    return [(1. - p[i]) * np.outer(g0[i], g0[i]) + p[i] * np.outer(g1[i], g1[i]) + eye for i in range(n)]


def _refine_features(F, B):
    """-> (refined matrix, True when the conditioning loop trimmed it down to ONE feature: the image-level query then drops
    the feature term, NNAL.py:443-445)."""
    nnz_feats = np.sum(F > 0, axis=1)
    feat_inds = np.argsort(-nnz_feats)[:int(B / 2)]
    ref_F = F[feat_inds, :]
    while np.linalg.matrix_rank(ref_F) < len(feat_inds):
        feat_inds = feat_inds[:-1]
        ref_F = F[feat_inds, :]
    single = False
    while np.linalg.cond(ref_F) > 1e6:
        feat_inds = feat_inds[:-1]
        ref_F = F[feat_inds, :]
        if len(feat_inds) == 1:
            print('Only one feature is selected.')
            single = True
            break
    return ref_F, single


def refine_feature_matrix(F, B):
    """PW_NNAL.refine_feature_matrix (PW_NNAL.py:819-849): the (at most B/2) features with the most positive entries,
    trimmed from the back until the matrix has full row rank and a condition number <= 1e6."""
    return _refine_features(F, B)[0]


def _entropy_query_single(expr, model, sess, padded_imgs, pool_inds):
    posts = PW_NN.batch_eval(model, sess, padded_imgs, pool_inds, expr.pars['patch_shape'],
                             expr.pars['ntb'], expr.pars['stats'], 'posteriors')[0]
    return binary_uncertainty_filter(posts, expr.pars['k'])


def fisher_candidates(expr, model, sess, padded_imgs, pool_inds, vols=None, on_device=False):
    """The device part of CNN_query(...,'fi') (PW_NNAL.py:89-136): posteriors, uncertainty filter
    to B candidates, their patches (channel-index normalisation of :125-129) and A-matrices.
    Returns (sel_inds, sel_posts, A list).  `vols`: the padded volumes already on the device (uploaded once per query).
    on_device: A stays the fp64 device tensor [B, L, L] the Fisher pass wrote (the device SDP solver takes it as it is)."""
    B = expr.pars['B']
    if vols is None:
        vols = patch_utils.DeviceVolumes(sess, padded_imgs)
    posts = PW_NN.batch_eval(model, sess, padded_imgs, pool_inds, expr.pars['patch_shape'],
                             expr.pars['ntb'], expr.pars['stats'], 'posteriors', _vols=vols)[0]
    if B < len(pool_inds):
        sel_inds = binary_uncertainty_filter(posts, B)
    else:
        # the reference's `posts.shape[1]` raises here; the evident intent is "all"
        sel_inds = np.arange(len(pool_inds))
    sel_posts = posts[sel_inds]
    m = len(padded_imgs)
    t = vols.gather(np.asarray(pool_inds)[sel_inds], expr.pars['patch_shape'],
                    np.asarray(expr.pars['stats'], dtype=np.float64)[:m], quirk=1)
    p1_in = sess.to_device(sel_posts.astype(np.float32), sess.torch.float32)
    out = model.fisher_device(t, len(sel_inds), p1_in, 1e-5, want=('A',))
    if on_device:
        return sel_inds, sel_posts, out['A']
    A = out['A'].cpu().numpy()
    return sel_inds, sel_posts, [A[i] for i in range(len(sel_inds))]


def egl_scores_device(model, t, n, p1):
    """EGL scores of n binary candidates (device patches t, posteriors of class 1 p1): ONE alq_grad_sqnorms pass with the
    unit cotangent gives ||u_t||^2, u = d(z0 - z1) / d theta, for both classes (NNAL_tools.egl_binary_scores).  The
    columns follow `grad_layers`, like the reference's T = len(grad_log_posts['0'])."""
    sq = model.grad_sqnorms_device(t, n, cls=-1).cpu().numpy()
    return NNAL_tools.egl_binary_scores(sq, p1)


def get_HV_inds(padded_img, patch_shape, thr, pool_inds, _vols=None):
    """PW_NNAL.get_HV_inds (PW_NNAL.py:632-669): the positions in `pool_inds` (ascending) of the pool voxels whose local
    variance is above `thr` - the 2-D variance map of every slice of the un-padded image with the patch RADIUS
    int((patch_shape[0] - 1) / 2) as the window size (:654-655), evaluated on the device at the pool voxels only
    (alq_local_var2d, indexed form) where the reference builds the whole map with one scipy convolution pair per slice.
    `_vols` (not a reference argument): a patch_utils.DeviceVolumes whose first modality is `padded_img`, already resident."""
    sess = _vols.sess if _vols is not None else None
    pool_inds = np.asarray(pool_inds, dtype=np.int64)
    if len(pool_inds) == 0:
        return np.zeros(0, dtype=np.int64)
    rads = patch_utils.patch_radii(patch_shape)
    if _vols is None:
        from . import device
        sess = device.default_session()
        _vols = patch_utils.DeviceVolumes(sess, [padded_img])
    scores = _vols.local_var(rads[0], 0, pool_inds, rads)
    return (scores > thr).nonzero().reshape(-1).cpu().numpy()


def CNN_query(expr, model, sess, padded_imgs, pool_inds, tr_inds, method_name):
    """PW_NNAL.CNN_query (PW_NNAL.py:18-166), branches `ps-random`, `entropy` and `fi`, plus `egl`, which the reference has only at
    image level (NNAL.py:234-285): uncertainty filter to B like `fi`, score, the k largest (stable: ties -> lower
    candidate first).  Returns positions into `pool_inds` (the caller maps them, PW_AL.py:405-408)."""
    pool_inds = np.asarray(pool_inds)
    if method_name == 'random':
        return np.random.permutation(len(pool_inds))[:expr.pars['k']]
    if method_name == 'ps-random':
        # PW_NNAL.py:38-49: random draws among the pool voxels of high local variance (of the first modality).  The reference
        # reads `exp.pars` there (a NameError); `expr.pars` is meant
        valid_pool_inds = get_HV_inds(padded_imgs[0], expr.pars['patch_shape'], 2., pool_inds,
                                      _vols=patch_utils.DeviceVolumes(sess, padded_imgs[:1]))
        rand_inds = np.random.permutation(len(valid_pool_inds))[:expr.pars['k']]
        return valid_pool_inds[rand_inds]
    if method_name == 'entropy':
        return _entropy_query_single(expr, model, sess, padded_imgs, pool_inds)
    if method_name == 'MC-entropy':
        # PW_NNAL.py:66-87.  The reference passes x_feed_dict as batch_eval's NINTH positional argument, which is
        # `mask` (PW_NN.py:365-366): the keep probability never reaches the feed and every iteration evaluates the
        # same deterministic posteriors.  Mirrored: MC_iters evaluations at keep_prob = 1, running average.
        x_feed_dict = {model.keep_prob: model.dropout_rate}
        total_posts = 0
        for i in range(expr.pars['MC_iters']):
            posts = PW_NN.batch_eval(model, sess, padded_imgs, pool_inds, expr.pars['patch_shape'], expr.pars['ntb'],
                                     expr.pars['stats'], 'posteriors', x_feed_dict)[0]
            total_posts = (posts + i * total_posts) / (i + 1)
        return np.argsort(np.abs(total_posts - .5), kind='stable')[:expr.pars['k']]
    if method_name == 'egl':
        B = expr.pars['B']
        vols = patch_utils.DeviceVolumes(sess, padded_imgs)
        posts = PW_NN.batch_eval(model, sess, padded_imgs, pool_inds, expr.pars['patch_shape'],
                                 expr.pars['ntb'], expr.pars['stats'], 'posteriors', _vols=vols)[0]
        sel_inds = binary_uncertainty_filter(posts, B) if B < len(pool_inds) else np.arange(len(pool_inds))
        t = vols.gather(pool_inds[sel_inds], expr.pars['patch_shape'],
                        np.asarray(expr.pars['stats'], dtype=np.float64)[:len(padded_imgs)], quirk=1)
        scores = egl_scores_device(model, t, len(sel_inds), posts[sel_inds])
        return sel_inds[np.argsort(-scores, kind='stable')[:expr.pars['k']]]
    if method_name == 'fi':
        lambda_ = expr.pars['lambda_']
        vols = patch_utils.DeviceVolumes(sess, padded_imgs)            # one upload for the whole query
        # expr.pars['SDP_solver'] = 'DEVICE' (not a value of the reference, whose 'CVXOPT' / 'MOSEK' both mean the host routine
        # here): the solve runs where the A-matrices are
        on_device = expr.pars.get('SDP_solver') == 'DEVICE'
        if on_device and lambda_ > 0:
            raise NotImplementedError("SDP_solver 'DEVICE' has the lambda_ = 0 form only (lambda_ = %r)" % (lambda_,))
        sel_inds, sel_posts, A = fisher_candidates(expr, model, sess, padded_imgs, pool_inds, vols, on_device=on_device)
        ref_F = None
        if lambda_ > 0:
            # PW_NNAL.py:138-150: features of the candidates, refined to a well-conditioned full-row-rank subset and
            # centred (the SDP's equality block needs X q = 0 to hold for the uniform q).  The reference evaluates them
            # for lambda_ = 0 too and never uses them there (NNAL_tools.py:626,646); skipped.
            F = PW_NN.batch_eval(model, sess, padded_imgs, pool_inds[sel_inds], expr.pars['patch_shape'],
                                 expr.pars['ntb'], expr.pars['stats'], 'feature_layer', _vols=vols)[0]
            ref_F = refine_feature_matrix(F, expr.pars['B'])
            ref_F = ref_F - np.mean(ref_F, axis=1, keepdims=True)
        if on_device:
            soln = NNAL_tools.SDP_query_distribution_device(sess, A, lambda_, ref_F, expr.pars['k'])
        else:
            soln = NNAL_tools.SDP_query_distribution(A, lambda_, ref_F, expr.pars['k'])
        q_opt = np.array(soln['x'][:len(sel_inds)]).ravel()
        Q_inds = NNAL_tools.sample_query_dstr(q_opt, expr.pars['k'], replacement=True)
        return sel_inds[Q_inds]
    raise NotImplementedError("query method %r is outside the scored path (random, ps-random, entropy, MC-entropy, egl, fi)" % (method_name,))


def _features_device(expr, model, sess, padded_mods, inds, stats):
    """feature_layer of the voxels `inds` of one subject as a device tensor [n, fdim] fp32 (memory order of the layer:
    a fixed permutation of the reference's flatten order, irrelevant to dot products and norms)."""
    torch = sess.torch
    vols = patch_utils.DeviceVolumes(sess, padded_mods)
    inds = np.asarray(inds)
    out = sess.empty((len(inds), model.feature_dim), torch.float32)
    for a in range(0, len(inds), PW_NN._CHUNK):
        b = min(len(inds), a + PW_NN._CHUNK)
        t = vols.gather(inds[a:b], expr.pars['patch_shape'], np.asarray(stats, dtype=np.float64)[:len(padded_mods)], quirk=1)
        _, _, feat = model.forward_device(t, b - a, False, True)
        out[a:b] = feat
    return out


def _row_norms(sess, F):
    from ._lib import check, ptr
    nrm = sess.empty((int(F.shape[0]),), sess.torch.float64)
    check(sess.lib.alq_row_norms(sess.ctx, ptr(F), int(F.shape[0]), int(F.shape[1]), ptr(nrm)))
    return nrm


def _cosine_sims(sess, A, na, Bm, nb):
    """[len(A), len(Bm)] float64 device tensor of cosine similarities (alq_cosine_sims)."""
    from ._lib import check, ptr
    S = sess.empty((int(A.shape[0]), int(Bm.shape[0])), sess.torch.float64)
    check(sess.lib.alq_cosine_sims(sess.ctx, ptr(A), int(A.shape[0]), ptr(Bm), int(Bm.shape[0]), int(A.shape[1]), ptr(na), ptr(nb), ptr(S)))
    return S


def _subject_stats(expr, i, m, attr='train_stats'):
    st = getattr(expr, attr)
    return [[st[i, 2 * j], st[i, 2 * j + 1]] for j in range(m)]


def rep_entropy_query(expr, model, sess, all_padded_imgs, pool_inds):
    """query_multimg 'rep-entropy' (PW_NNAL.py:284-351): among the B most uncertain voxels, greedily pick the k whose
    feature vectors best "represent" the rest of the pool - each step adds the candidate maximising
    sum_r max_{c in Q + candidate} cos(f_r, f_c) over the remaining pool voxels r.  The similarity block is one device
    GEMM (alq_cosine_sims, fp64 accumulation like the reference's float64 NumPy), a greedy step one streaming pass that
    scores ALL candidates at once (alq_colsum_max) where the reference scores one candidate per Python iteration."""
    from ._lib import check, ptr
    torch = sess.torch
    sess.bind_stream()
    k, B = expr.pars['k'], expr.pars['B']
    m = len(all_padded_imgs[0]) - 1
    s = len(pool_inds)
    F = [_features_device(expr, model, sess, all_padded_imgs[i][:-1], pool_inds[i], _subject_stats(expr, i, m)) if len(pool_inds[i])
         else sess.empty((0, model.feature_dim), torch.float32) for i in range(s)]
    sel_inds, sel_posts = bin_uncertainty_filter_multimg(expr, model, sess, all_padded_imgs, pool_inds, B)
    F_unc = torch.cat([F[i].index_select(0, sess.to_device(np.asarray(sel_inds[i]), torch.int64)) for i in range(s) if len(sel_inds[i]) > 0])
    rem = []
    for i in range(s):
        keep = np.setdiff1d(np.arange(len(pool_inds[i])), np.asarray(sel_inds[i], dtype=np.int64))
        rem.append(F[i].index_select(0, sess.to_device(keep, torch.int64)))
    F_rem = torch.cat(rem)
    nB, nR = int(F_unc.shape[0]), int(F_rem.shape[0])
    S = _cosine_sims(sess, F_rem, _row_norms(sess, F_rem), F_unc, _row_norms(sess, F_unc))        # [remaining, uncertain]
    work = sess.empty((sess.lib.alq_colsum_work_bytes(nR, nB),), torch.uint8)
    scores = sess.empty((nB,), torch.float64)
    cmax = sess.empty((nR,), torch.float64)
    Q, taken = [], np.zeros(nB, bool)
    for it in range(min(k, nB)):
        check(sess.lib.alq_colsum_max(sess.ctx, ptr(S), nR, nB, ptr(cmax) if it else None, None, ptr(scores), ptr(work)))
        sc = scores.cpu().numpy()
        sc[taken] = -np.inf
        j = int(np.argmax(sc))                      # first maximum among the candidates left, in their original order (:339-343)
        Q.append(j)
        taken[j] = True
        check(sess.lib.alq_take_colmax(sess.ctx, ptr(S), nR, nB, j, 0 if it else 1, ptr(cmax)))
    local = patch_utils.global2local_inds(Q, [len(sel_inds[i]) for i in range(s)])
    return [np.array(sel_inds[i])[local[i]] for i in range(s)]


def core_set_query(expr, model, sess, all_padded_imgs, pool_inds, labeled_inds):
    """query_multimg 'core-set' (PW_NNAL.py:353-451): k-centre greedy on cosine similarity - start from every pool voxel's
    largest similarity to the labelled set, then k times take the voxel LEAST similar to anything chosen or labelled.
    As in the reference the labelled side is the LAST subject of `labeled_inds` only (its loop variable `i` is read
    after the loop, :399-404), evaluated in batches of 1000 (NN.gen_batch_inds) with `expr.labeled_stats`."""
    from . import NN
    from ._lib import check, ptr
    torch = sess.torch
    sess.bind_stream()
    k = expr.pars['k']
    m = len(all_padded_imgs[0]) - 1
    s = len(pool_inds)
    sizes = [len(p) for p in pool_inds]
    F_u = torch.cat([_features_device(expr, model, sess, all_padded_imgs[i][:-1], pool_inds[i], _subject_stats(expr, i, m))
                     if sizes[i] else sess.empty((0, model.feature_dim), torch.float32) for i in range(s)])
    n = int(F_u.shape[0])
    norms_u = _row_norms(sess, F_u)
    sims = torch.full((n,), -np.inf, dtype=torch.float64, device=sess.device)
    i = len(labeled_inds) - 1
    nT = len(labeled_inds[i])
    if expr.labeled_paths == expr.train_paths:
        lab_mods = all_padded_imgs[i][:-1]
    else:
        from . import PW_AL
        lab_mods = PW_AL.load_and_pad(list(expr.labeled_paths[i][:-1]) + [expr.labeled_paths[i][-1]], expr.pars['patch_shape'])[:-1]
    for batch in NN.gen_batch_inds(nT, 1000):
        F_T = _features_device(expr, model, sess, lab_mods, np.array(labeled_inds[i])[batch], _subject_stats(expr, i, m, 'labeled_stats'))
        St = _cosine_sims(sess, F_T, _row_norms(sess, F_T), F_u, norms_u)                           # [labelled batch, pool]
        check(sess.lib.alq_fold_rowmax(sess.ctx, ptr(St), int(F_T.shape[0]), n, ptr(sims)))
    Q = []
    for _ in range(min(k, n)):
        q_ind = int(np.argmin(sims.cpu().numpy()))
        Q.append(q_ind)
        Sq = _cosine_sims(sess, F_u[q_ind:q_ind + 1], norms_u[q_ind:q_ind + 1], F_u, norms_u)      # [1, pool]
        check(sess.lib.alq_fold_rowmax(sess.ctx, ptr(Sq), 1, n, ptr(sims)))
        sims[q_ind] = np.inf
    return patch_utils.global2local_inds(Q, sizes)


def committee_holder(expr, model, sess):
    """`expr.model_holder` (PW_AL.py:780-790), or - for a caller that has none - a net built once like `model` (layer dict,
    input shape, skips, dropout, max_batch, optimiser, grad_layers) on the same session and cached on `expr`."""
    if getattr(model, 'dense', False):
        raise NotImplementedError('committee_holder: not defined for a fully-convolutional model (1x1 conv head)')
    holder = getattr(expr, 'model_holder', None)
    if holder is None:
        from .device import DeviceModel
        drop = [list(model.dropout_layers), model.dropout_rate] if len(model.dropout_layers) else None
        holder = DeviceModel(sess, model.layer_dict, model.in_shape, model.skips, model.feature_idx, drop, model.max_batch,
                             name=model.name + '_holder')
        if model._opt is not None:
            holder.get_optimizer(model._opt['lr'], model.train_layers, model._opt['name'])
        if len(model.grad_layers):
            holder.get_gradients(model.grad_layers)
        expr.model_holder = holder
    return holder


def committee_query(expr, model, sess, all_padded_imgs, pool_inds, labeled_inds, method_name):
    """query_multimg 'ensemble' and 'QBC-JS' (PW_NNAL.py:453-545).  M = len(expr.pretrained_paths) members, evaluated in
    order i = 0 .. M-1 on `expr.model_holder` (the main `model` is not touched): with no labels yet, member i is the weights
    file pretrained_paths[i]; otherwise every member starts from expr.prev_weights_path and is fine-tuned once by
    finetune_multimg (members differ through the NumPy stream only).  Each member's class-1 posteriors of the pool
    (bin_uncertainty_filter_multimg's device sweep at keep_prob 1, no host copy) update the float64 running means on the
    device (alq_committee_update, one launch per member); the keys of the last member go to the device top-k:
    ensemble argsort(|av - .5|), QBC-JS argsort(-(ent(av) - avH)), ties -> lower pool position.

    The reference is broken in three places; resolved by its evident intent:
      1. expr.prev_weights_path is never set: it is the current model (PW_AL.py:834-843), `curr_weights_<iters>` in
         PW_AL.Experiment_MultiImg.run_method; a caller without one gets `model`'s current weights.
      2. run_method creates model_holder / pretrained_paths for 'ensemble' only: here both methods have them.
      3. pretrained_paths is a hard-coded file-server list: it comes from pars['pretrained_paths'] (ValueError without it).
    Under torch.distributed each rank sweeps its pool_shard.work_block; the keys are assembled exactly
    (pool_shard.allgather_rows) and every rank runs the same top-k.  Fine-tuning is replicated on every rank."""
    from . import PW_AL, pool_shard
    torch = sess.torch
    if model.nclass != 2:
        raise ValueError("query method %r: the committee formulas are binary (PW_NNAL.py:453-545), the net has %d classes"
                         % (method_name, model.nclass))
    paths = getattr(expr, 'pretrained_paths', None)
    if paths is None:
        paths = expr.pars.get('pretrained_paths')
    if not paths:
        raise ValueError("query method %r needs the committee's weight files in pars['pretrained_paths'] (their number is "
                         "the committee size)" % (method_name,))
    k = expr.pars['k']
    sizes = [len(p) for p in pool_inds]
    n = int(np.sum(sizes))
    n_labels = int(np.sum([len(labeled_inds[i]) for i in range(len(labeled_inds))])) if labeled_inds is not None else 0
    holder = committee_holder(expr, model, sess)
    mode = 0 if method_name == 'ensemble' else 1
    start = None
    if n_labels > 0 and getattr(expr, 'prev_weights_path', None) is None:
        start = OrderedDict((nme, [np.array(W), np.array(b)]) for nme, (W, b) in model.var_dict.items())
    dvols = {}                                                  # one upload per subject for all members
    a, b = pool_shard.work_block(n)
    mean_p = sess.empty((b - a,), torch.float64)
    mean_h = sess.empty((b - a,), torch.float64) if mode == 1 else None
    keys = sess.empty((b - a,), torch.float64)
    M = len(paths)
    for i in range(M):
        if n_labels == 0:
            holder.perform_assign_ops(paths[i], sess)
        else:
            if start is None:
                holder.perform_assign_ops(expr.prev_weights_path, sess)
            else:
                holder.set_weights(start)
            PW_AL.finetune_multimg(expr, holder, sess, all_padded_imgs, labeled_inds)
        _, _, p1 = pool_posteriors_device(expr, holder, sess, all_padded_imgs, pool_inds, {holder.keep_prob: 1.}, dvols)
        sess.committee_update(p1, i, mode, mean_p, mean_h, keys if i == M - 1 else None)
    if (a, b) != (0, n):
        K = pool_shard.allgather_rows(n, np.arange(a, b), keys.cpu().numpy(), sess)
        keys = sess.to_device(K, torch.float64)
    order = sess.topk_smallest(keys, min(k, n)).cpu().numpy()
    return patch_utils.global2local_inds(order, sizes)


def query_multimg(expr, model, sess, all_padded_imgs, pool_inds, labeled_inds, method_name):
    """PW_NNAL.query_multimg (PW_NNAL.py:169-629), branches `ps-random` (:205-224), `entropy` (:226-230), `ensemble` / `QBC-JS` (:453-545,
    committee_query) and `fi` (:547-627), plus `egl` (image level only in the reference, NNAL.py:234-285; candidates gathered and sharded like
    `fi`, the k largest scores over all subjects, ties -> lower candidate first).  Returns, per subject, positions into
    that subject's pool_inds."""
    k = expr.pars['k']
    B = expr.pars['B']
    sizes = [len(p) for p in pool_inds]
    if method_name == 'random':
        inds = np.random.permutation(int(np.sum(sizes)))[:k]
        return patch_utils.global2local_inds(inds, sizes)
    if method_name == 'ps-random':
        # PW_NNAL.py:205-224: per subject the pool voxels of high local variance (first modality, threshold 2), then k random
        # draws over their concatenation; fewer than k qualifying voxels: all of them
        dvols = {}
        valid_pool_inds = []
        for i in range(len(all_padded_imgs)):
            if len(pool_inds[i]) and i not in dvols:
                dvols[i] = patch_utils.DeviceVolumes(sess, all_padded_imgs[i][:-1])
            valid_pool_inds.append(get_HV_inds(all_padded_imgs[i][0], expr.pars['patch_shape'], 2., pool_inds[i], _vols=dvols.get(i)))
        valid_inds_sizes = [len(v) for v in valid_pool_inds]
        rand_inds = np.random.permutation(int(np.sum(valid_inds_sizes)))[:k]
        local_inds = patch_utils.global2local_inds(rand_inds, valid_inds_sizes)
        return [valid_pool_inds[i][local_inds[i]] for i in range(len(valid_pool_inds))]
    if method_name == 'entropy':
        return bin_uncertainty_filter_multimg(expr, model, sess, all_padded_imgs, pool_inds, k)[0]
    if method_name in ('MC-entropy', 'BALD'):
        # PW_NNAL.py:232-282: MC_iters dropout passes over the whole pool (keep_prob = model.dropout_rate through
        # batch_eval's x_feed_dict), running means with the reference's update (new + i * mean) / (i + 1).
        # MC-entropy ranks by |mean posterior - .5|; BALD by H(mean posterior) - mean H(posterior), zeros lifted by 1e-6.
        def bin_entropy(p):
            a, b = p.copy(), 1 - p
            a[a == 0] += 1e-6
            b[b == 0] += 1e-6
            return -a * np.log(a) - b * np.log(b)
        feed = {model.keep_prob: model.dropout_rate}
        mean_p, mean_h = 0, 0
        for it in range(expr.pars['MC_iters']):
            p = bin_uncertainty_filter_multimg(expr, model, sess, all_padded_imgs, pool_inds, k, feed)
            mean_p = (p + it * mean_p) / (it + 1)
            if method_name == 'BALD':
                mean_h = (bin_entropy(p) + it * mean_h) / (it + 1)
        if method_name == 'MC-entropy':
            order = np.argsort(np.abs(mean_p - .5), kind='stable')
        else:
            order = np.argsort(-(bin_entropy(mean_p) - mean_h), kind='stable')
        return patch_utils.global2local_inds(order[:k], sizes)
    if method_name in ('ensemble', 'QBC-JS'):
        return committee_query(expr, model, sess, all_padded_imgs, pool_inds, labeled_inds, method_name)
    if method_name == 'rep-entropy':
        return rep_entropy_query(expr, model, sess, all_padded_imgs, pool_inds)
    if method_name == 'core-set':
        return core_set_query(expr, model, sess, all_padded_imgs, pool_inds, labeled_inds)
    if method_name == 'egl':
        from . import pool_shard
        dvols = {}
        sel_inds, sel_posts = bin_uncertainty_filter_multimg(expr, model, sess, all_padded_imgs, pool_inds, B, _vols=dvols)
        m = len(all_padded_imgs[0]) - 1
        stats = np.asarray(expr.train_stats, dtype=np.float64)
        nsel = [len(s_) for s_ in sel_inds]
        ncand = int(np.sum(nsel))
        a, b = pool_shard.work_block(ncand)            # this rank's block of the candidate list (volumes are replicated)
        rows = []
        off = 0
        for i in range(len(pool_inds)):
            lo, hi = max(a, off) - off, min(b, off + nsel[i]) - off
            if hi > lo:
                vols = dvols.get(i) or patch_utils.DeviceVolumes(sess, all_padded_imgs[i][:m])
                t = vols.gather(np.asarray(pool_inds[i])[np.asarray(sel_inds[i])[lo:hi]], expr.pars['patch_shape'],
                                stats[i, :2 * m], quirk=0)                 # slab rule, patch_utils.py:1203-1207
                rows.append(egl_scores_device(model, t, hi - lo, np.asarray(sel_posts[i][lo:hi], dtype=np.float64))[:, None])
            off += nsel[i]
        S = np.concatenate(rows) if rows else np.zeros((0, 1))
        if (a, b) != (0, ncand):
            S = pool_shard.allgather_rows(ncand, np.arange(a, b), S, sess)
        order = np.argsort(-S[:, 0], kind='stable')[:k]
        local = patch_utils.global2local_inds(order, nsel)
        return [np.array(sel_inds[i])[local[i]] for i in range(len(sel_inds))]
    if method_name == 'fi':
        from . import pool_shard
        dvols = {}                                                       # one upload per subject for the whole query
        sel_inds, sel_posts = bin_uncertainty_filter_multimg(expr, model, sess, all_padded_imgs, pool_inds, B, _vols=dvols)
        m = len(all_padded_imgs[0]) - 1
        stats = np.asarray(expr.train_stats, dtype=np.float64)
        nsel = [len(s_) for s_ in sel_inds]
        ncand = int(np.sum(nsel))
        a, b = pool_shard.work_block(ncand)            # this rank's block of the candidate list (volumes are replicated)
        # expr.pars['SDP_solver'] = 'DEVICE' (this build's value): the A-matrices stay where the Fisher pass wrote them and the
        # solve runs there (lambda_ = 0 only); one process: no host copy at all, several ranks: the gathered rows go up once
        on_device = expr.pars.get('SDP_solver') == 'DEVICE'
        if on_device and expr.pars['lambda_'] > 0:
            raise NotImplementedError("SDP_solver 'DEVICE' has the lambda_ = 0 form only (lambda_ = %r)" % (expr.pars['lambda_'],))
        rows = []
        off = 0
        for i in range(len(pool_inds)):
            lo, hi = max(a, off) - off, min(b, off + nsel[i]) - off
            if hi > lo:
                vols = dvols.get(i) or patch_utils.DeviceVolumes(sess, all_padded_imgs[i][:m])
                t = vols.gather(np.asarray(pool_inds[i])[np.asarray(sel_inds[i])[lo:hi]], expr.pars['patch_shape'],
                                stats[i, :2 * m], quirk=0)                 # slab rule, patch_utils.py:1203-1207
                p1_in = sess.to_device(np.asarray(sel_posts[i][lo:hi], dtype=np.float32), sess.torch.float32)
                out = model.fisher_device(t, hi - lo, p1_in, 1e-3, want=('A',))   # diag_load 1e-3, :578
                rows.append(out['A'] if on_device and (a, b) == (0, ncand) else out['A'].cpu().numpy())
            off += nsel[i]
        # PW_NNAL.py:600-614: 'CVXOPT' -> SDP_query_distribution, 'MOSEK' -> solve_FIAL_SDP; both end in
        # the same A-optimal-design problem, solved here by NNAL_tools' own routine (parity unpinned)
        if on_device:
            if (a, b) == (0, ncand):
                A_dev = sess.torch.cat(rows) if rows else sess.empty((0, model.L, model.L), sess.torch.float64)
            else:
                A_rows = np.concatenate(rows) if rows else np.zeros((0, model.L, model.L))
                A_dev = sess.to_device(pool_shard.allgather_rows(ncand, np.arange(a, b), A_rows, sess), sess.torch.float64)
            soln = NNAL_tools.SDP_query_distribution_device(sess, A_dev, expr.pars['lambda_'], [], k)
            q_opt = np.array(soln['x'][:ncand]).ravel()
        else:
            A_rows = np.concatenate(rows) if rows else np.zeros((0, model.L, model.L))
            if (a, b) != (0, ncand):
                A_rows = pool_shard.allgather_rows(ncand, np.arange(a, b), A_rows, sess)
            A = [A_rows[j] for j in range(ncand)]
            if expr.pars.get('SDP_solver', 'CVXOPT') == 'MOSEK':
                q_opt = np.asarray(NNAL_tools.solve_FIAL_SDP(A)[0]).ravel()
            else:
                soln = NNAL_tools.SDP_query_distribution(A, expr.pars['lambda_'], [], k)
                q_opt = np.array(soln['x'][:len(A)]).ravel()
        draws = NNAL_tools.sample_query_dstr(q_opt, k, replacement=True)
        local = patch_utils.global2local_inds(draws, [len(s) for s in sel_inds])
        return [np.array(sel_inds[i])[local[i]] for i in range(len(sel_inds))]
    raise NotImplementedError("query method %r is outside the scored path (random, ps-random, entropy, MC-entropy, BALD, ensemble, QBC-JS, "
                              "rep-entropy, core-set, egl, fi)" % (method_name,))


def stoch_approx_IF(model, sess, tr_patches, pool_patches, max_iter, scale=50):
    """PW_NNAL.stoch_approx_IF (PW_NNAL.py:851-881): V_0 = the last-layer gradients of the pool patches at their predicted
    ("weak") labels, then max_iter times V <- G + V + H_r V / scale with H_r the last-layer Hessian of a uniformly drawn training
    patch.  Returns (V [(d+1)c, n_pool] float64, weak_labels).  The draws are the reference's, max_iter calls of
    np.random.randint(ntr) on the global stream, taken up front; the reference forms every H_r with np.kron and multiplies it into V,
    here each column takes c dot products and a rank-c update on the device (alq_llfc_stoch_if) and only the distinct drawn
    patches are forwarded."""
    tr_patches = np.asarray(tr_patches)
    ntr = tr_patches.shape[0]
    draws = np.array([np.random.randint(ntr) for _ in range(int(max_iter))], dtype=np.int64)
    uniq, inv = np.unique(draws, return_inverse=True)
    pool_t, n_pool = model._as_device_batch(pool_patches)
    tr_t = model._as_device_batch(tr_patches[uniq])[0] if len(uniq) else None
    V, weak = model.llfc_stoch_if_device(pool_t, n_pool, tr_t, inv.reshape(-1), scale)
    idx = sess.to_device(model.llfc_reference_order(), sess.torch.int64)
    V_t = V.index_select(1, idx).to(sess.torch.float64).t().contiguous()      # the feature permutation, once, on the way out
    return V_t.cpu().numpy(), weak.cpu().numpy()


def _is_device_tensor(x):
    return hasattr(x, 'data_ptr') and hasattr(x, 'device')


def _segment_min_device(sess, overseg_img, inds, scores, n_labels):
    """alq_segment_min: float64 device table [S, n_labels] of an over-segmentation [H, W, S] (a host array, uploaded here, or an
    int32 device tensor as regions.oversegment(..., keep_on_device=True) leaves it, read where it lies), the scored voxels
    `inds` (host) and their `scores` (float64 device tensor)."""
    import ctypes as C
    from ._lib import check, ptr
    torch = sess.torch
    sess.bind_stream()
    on_device = _is_device_tensor(overseg_img)
    seg = overseg_img if on_device else np.asarray(overseg_img)
    if seg.ndim != 3:
        raise ValueError('the over-segmentation must be a 3-D volume')
    shape = tuple(int(v) for v in seg.shape)
    nvox = shape[0] * shape[1] * shape[2]
    inds = np.ascontiguousarray(np.asarray(inds, dtype=np.int64)).reshape(-1)
    n = int(inds.shape[0])
    if int(scores.numel()) != n:
        raise ValueError('%d scores for %d voxels' % (int(scores.numel()), n))
    if n and (inds.min() < 0 or inds.max() >= nvox):
        raise IndexError('voxel index outside the over-segmentation %r' % (shape,))
    if len(np.unique(inds)) != n:
        raise ValueError('superpix_scoring: duplicate voxel indices (the reference keeps an arbitrary one of their scores)')
    table = sess.empty((shape[2], int(n_labels)), torch.float64)
    if on_device:
        d_lab = seg if seg.dtype == torch.int32 and seg.is_contiguous() else seg.to(torch.int32).contiguous()
    else:
        d_lab = sess.to_device(seg.astype(np.int32), torch.int32)
    d_inds = sess.to_device(inds, torch.int64)
    dims = (C.c_int64 * 3)(*shape)
    check(sess.lib.alq_segment_min(sess.ctx, ptr(d_lab), dims, int(n_labels), ptr(d_inds) if n else None,
                                   ptr(scores) if n else None, n, ptr(table)))
    return table


def superpix_scoring(overseg_img, inds, scores):
    """PW_NNAL.superpix_scoring (PW_NNAL.py:944-1021): the scores of a set of voxels (raveled indices `inds` into the 3-D
    over-segmentation, unique) extended to super-pixels: float64 [S, overseg_img.max() + 1], entry (z, l) = the smallest score
    among the scored voxels of super-pixel l in slice z (regionprops' min_intensity of a score image that is inf elsewhere).
    inf where a (slice, label) got no scored voxel AND where the label is absent from the slice - the reference's code gives
    inf in both cases, whatever its docstring says; column 0 (background) stays inf.  Device: alq_segment_min.  overseg_img may
    be an int32 device tensor (regions.oversegment(..., keep_on_device=True)): it is read where it lies."""
    from . import device
    sess = device.default_session()
    if _is_device_tensor(overseg_img):
        seg, n_labels = overseg_img, int(overseg_img.max().item()) + 1
    else:
        seg = np.asarray(overseg_img)
        n_labels = int(seg.max()) + 1
    sc = sess.to_device(np.asarray(scores, dtype=np.float64).reshape(-1), sess.torch.float64)
    return _segment_min_device(sess, seg, inds, sc, n_labels).cpu().numpy()


def SuPix_query(expr, model, sess, padded_imgs, pool_inds, overseg_img, method_name, n_segments=100, compactness=0.1, T=10, min_size=0,
                mask=None):
    """PW_NNAL.SuPix_query (PW_NNAL.py:883-941), `entropy`: the k super-pixels (slice, label) whose most uncertain scored
    voxel is the most uncertain.  Posteriors of the pool voxels as in batch_eval (kept on the device), keys |p - .5|
    (alq_score_entropy), their minimum per (slice, label) (alq_segment_min), and the k smallest finite entries of the table
    (alq_topk_uncertain: ties -> lower flat index z * n_labels + label).  Returns (qSuPix int64 [2, k] = slices; labels,
    PW_AL.get_SuPix_inds(overseg_img, qSuPix)).  Fewer than k scored super-pixels: ValueError (the reference's argsort would
    hand out unscored ones).  The reference's signature (expr, run, model, pool_lines, train_inds, overseg_img, method_name,
    sess) belongs to its per-run index-file API; here the pool is given as voxel indices, like CNN_query's.  `random` is not
    defined by the reference (its `qSuPix` is never assigned there).
    overseg_img: a host array (uploaded for the table, as ever), an int32 device tensor [H, W, S], or None: then the un-padded
    box of padded_imgs (every modality, padded by the patch radii) is over-segmented on the device - regions.oversegment with
    n_segments, compactness, T, min_size, mask (bool over the un-padded box) - and the table is built from labels that never left
    it; they are copied to the host once, at the end, for get_SuPix_inds."""
    from . import PW_AL
    from ._lib import check, ptr
    if method_name != 'entropy':
        raise NotImplementedError("SuPix_query method %r: only 'entropy' is defined (the reference leaves qSuPix unset for 'random')"
                                  % (method_name,))
    torch = sess.torch
    k = int(expr.pars['k'])
    if overseg_img is None:
        from . import regions
        r = patch_utils.patch_radii(expr.pars['patch_shape'])
        box = [np.asarray(v)[r[0]:np.asarray(v).shape[0] - r[0], r[1]:np.asarray(v).shape[1] - r[1], r[2]:np.asarray(v).shape[2] - r[2]]
               for v in padded_imgs]
        seg, counts = regions.oversegment(box, n_segments=n_segments, compactness=compactness, T=T, min_size=min_size, mask=mask, sess=sess,
                                          keep_on_device=True, with_counts=True)
        n_labels = int(counts.max().item()) + 1
    elif _is_device_tensor(overseg_img):
        seg, n_labels = overseg_img, int(overseg_img.max().item()) + 1
    else:
        seg = np.asarray(overseg_img)
        n_labels = int(seg.max()) + 1
    pool_inds = np.asarray(pool_inds, dtype=np.int64)
    vols = patch_utils.DeviceVolumes(sess, padded_imgs)
    p1 = PW_NN.posteriors_device(model, sess, padded_imgs, pool_inds, expr.pars['patch_shape'], expr.pars['ntb'], expr.pars['stats'],
                                 _vols=vols)
    n = int(p1.numel())
    sess.bind_stream()
    keys = sess.empty((n,), torch.float64)
    if n:
        check(sess.lib.alq_score_entropy(sess.ctx, ptr(p1), n, ptr(keys), None))
    table = _segment_min_device(sess, seg, pool_inds, keys, n_labels)
    nscored = int(torch.isfinite(table).sum().item())
    if nscored < k:
        raise ValueError('SuPix_query: %d super-pixels hold a scored voxel, k = %d' % (nscored, k))
    order = sess.topk_smallest(table.reshape(-1), k).cpu().numpy()
    qSuPix = np.array([order // n_labels, order % n_labels], dtype=np.int64)
    return qSuPix, PW_AL.get_SuPix_inds(seg.cpu().numpy() if _is_device_tensor(seg) else seg, qSuPix)


def draw_queries(qdist, prior, k, replacement=False):
    """PW_NNAL.draw_queries (PW_NNAL.py:1023-1039): draws from the query distribution, times a prior when one is given."""
    pies = qdist if len(prior) == 0 else qdist * prior
    return NNAL_tools.sample_query_dstr(pies, k, replacement)
