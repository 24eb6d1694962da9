"""Batched patch evaluation (reference: PW_NN.py:357-539) on the device."""
import numpy as np

from . import patch_utils

_CHUNK = 8192   # indices gathered per device pass (results do not depend on it)


def mc_dropout_args(model, x_feed_dict):
    """(keep_prob, dropout active?, seed) of one batch_eval call: `x_feed_dict = {model.keep_prob: p}` overrides
    keep_prob = 1 (PW_NN.py:516-521); an evaluation with dropout draws ONE seed from the global NumPy stream (masks are
    then keyed by the sample's position).  A rank of a sharded evaluation that holds nothing of a subject calls this
    alone, so that every rank's stream advances alike."""
    keep_prob = 1.
    for k, val in x_feed_dict.items():
        if k is getattr(model, 'keep_prob', None):
            keep_prob = float(val)
    mc = keep_prob < 1. and len(model.dropout_layers) > 0
    seed = int(np.random.randint(0, 2 ** 31 - 1)) if mc else 0
    return keep_prob, mc, seed


def _eval_passes(model, sess, img_dat, inds, patch_shape, batch_size, stats, drop, want_pred, want_feat, _vols, _first_sample):
    """The device part of batch_eval: gather + normalise (channel-index rule) + forward, one chunk of _CHUNK voxels at a
    time.  Yields (a, b, post [c, b-a], pred, feat) device tensors of inds[a:b]; `drop` = mc_dropout_args(...)."""
    keep_prob, mc, seed = drop
    if not isinstance(img_dat[0], np.ndarray):
        # PW_NN.py:429-444: paths -> load (NRRD) and zero-pad by the patch radii
        from . import nrrd_io
        rads = [int((patch_shape[i] - 1) / 2.) for i in range(3)]
        img_dat = [np.pad(nrrd_io.read(p)[0], ((rads[0], rads[0]), (rads[1], rads[1]), (rads[2], rads[2])), 'constant')
                   for p in img_dat]
    if int(batch_size) < 1:
        raise ValueError('batch_size must be positive')
    m = len(img_dat)
    inds = np.asarray(inds)
    n = len(inds)
    # _vols (not a reference argument): volumes a caller of this package has already uploaded for the same query
    vols = _vols if _vols is not None else patch_utils.DeviceVolumes(sess, img_dat)
    st = np.asarray(stats, dtype=np.float64)[:m]
    for a in range(0, n, _CHUNK):
        b = min(n, a + _CHUNK)
        t = vols.gather(inds[a:b], patch_shape, st, quirk=1)
        if mc:
            post, pred = model.forward_dropout_device(t, b - a, keep_prob, seed=seed, first_sample=_first_sample + a,
                                                      want_pred=want_pred)
            feat = None
        else:
            post, pred, feat = model.forward_device(t, b - a, want_pred, want_feat)
        yield a, b, post, pred, feat


def posteriors_device(model, sess, img_dat, inds, patch_shape, batch_size, stats, x_feed_dict={}, _vols=None, _first_sample=0,
                      out=None):
    """batch_eval(..., 'posteriors') without the host copy: the class-1 posteriors of `inds` as a float32 device tensor
    [n] (`out`, when given, is filled).  Same gather, statistics, passes and dropout draws as batch_eval, so the float64
    widening of this tensor is batch_eval's result bit for bit."""
    drop = mc_dropout_args(model, x_feed_dict)
    n = len(np.asarray(inds))
    if out is None:
        out = sess.empty((n,), sess.torch.float32)
    for a, b, post, _, _ in _eval_passes(model, sess, img_dat, inds, patch_shape, batch_size, stats, drop, False, False, _vols,
                                         _first_sample):
        out[a:b] = post[1]
    return out


_LABELLED = ('loss', 'hess_vecp')


def _labelled_batches(sess, img_dat, inds, patch_shape, batch_size, stats, mask, _vols):
    """The batches of the reference's labelled evaluation (PW_NN.py:446-451, :485-506): consecutive runs of `batch_size`
    indices (the rest as a last shorter one).  Yields (a, b, device patches, int32 labels): the patches gathered and
    normalised with the channel-index rule like every batch_eval variable, the labels mask[inds] with the two-class
    one-hot rule of :494-496 (0 -> class 0, 1 -> class 1, any other value -> an all-zero column, here label -1)."""
    if mask is None:
        # (the reference fails here too, unpacking get_patches' single result, PW_NN.py:486-492)
        raise NotImplementedError("batch_eval: 'loss' / 'hess_vecp' without `mask` - the labels are read from it")
    if int(batch_size) < 1:
        raise ValueError('batch_size must be positive')
    inds = np.asarray(inds)
    n = len(inds)
    m = len(img_dat)
    vols = _vols if _vols is not None else patch_utils.DeviceVolumes(sess, img_dat)
    st = np.asarray(stats, dtype=np.float64)[:m]
    r = patch_utils.patch_radii(patch_shape)
    orig = tuple(int(np.asarray(img_dat[0]).shape[a]) - 2 * r[a] for a in range(3))
    lab_all = np.asarray(mask)[np.unravel_index(inds, orig)]
    for a in range(0, n, int(batch_size)):
        b = min(n, a + int(batch_size))
        lab = np.where(lab_all[a:b] == 0, 0, np.where(lab_all[a:b] == 1, 1, -1)).astype(np.int32)
        yield a, b, vols.gather(inds[a:b], patch_shape, st, quirk=1), lab


def _eval_labelled(model, sess, img_dat, inds, patch_shape, batch_size, stats, var, mask, x_feed_dict, _vols, whole_set):
    """'loss' and 'hess_vecp' of batch_eval (PW_NN.py:467, :485-496, :532-535), one device call per reference batch."""
    torch = sess.torch
    for k, val in x_feed_dict.items():
        if k is getattr(model, 'keep_prob', None) and float(val) != 1.:
            raise NotImplementedError('%s at keep_prob < 1' % var)
    n = len(np.asarray(inds))
    if var == 'loss':
        vals = np.zeros(n)
        for a, b, t, lab in _labelled_batches(sess, img_dat, inds, patch_shape, batch_size, stats, mask, _vols):
            vals[a:b] = model.mean_loss(t, lab)
        return vals
    if not hasattr(model, 'v_placeholder'):
        raise AttributeError('model.v_placeholder is missing: call Influence.get_hess_vec_product(model, layers) first')
    idx = model.hess_layer_idx(model.Hess_layers)
    v = model.ravel_for_layers([x_feed_dict[h] for h in model.v_placeholder], idx)
    vd = sess.to_device(v, torch.float32)
    vals = np.zeros(n)                      # what the reference returns for an empty index list (PW_NN.py:463)
    acc = None
    for a, b, t, lab in _labelled_batches(sess, img_dat, inds, patch_shape, batch_size, stats, mask, _vols):
        labd = sess.to_device(lab, torch.int32)
        if whole_set:
            acc, _ = model.hess_vecp_device(t, b - a, labd, vd, idx, 1. / n, acc)
        else:
            hv, _ = model.hess_vecp_device(t, b - a, labd, vd, idx, 1. / (b - a))
            vals = hv                       # PW_NN.py:532-533: every batch overwrites `vals`
    if whole_set and acc is not None:
        vals = acc
    if isinstance(vals, np.ndarray):
        return vals
    return model.unflatten(vals.cpu().numpy(), idx)


def batch_eval(model, sess, img_dat, inds, patch_shape, batch_size, stats, varnames,
               mask=None, x_feed_dict={}, _vols=None, _first_sample=0, _whole_set=False):
    """PW_NN.batch_eval: evaluates `varnames` ('posteriors', 'prediction', 'feature_layer', 'loss', 'hess_vecp')
    of `model` on patches around voxels `inds` of the m padded modalities `img_dat`.

    'loss' and 'hess_vecp' (PW_NN.py:467, :485-496) take the labels from `mask` at `inds` as two-class one-hot columns and,
    unlike the other variables, depend on `batch_size`: they are evaluated per reference batch.  'loss' -> [n], every entry
    of a batch holding that batch's mean cross-entropy.  'hess_vecp' -> the list [HW, Hb, ...] over `model.Hess_layers`
    (Influence.get_hess_vec_product), the vector taken from the `model.v_placeholder` entries of `x_feed_dict`, float64 -
    OF THE LAST BATCH ONLY: the reference assigns `vals = batch_vals` in every batch (PW_NN.py:532-533), so the product of
    the Hessian of the last batch's mean loss is what its Newton-CG solve sees; mirrored literally.  `_whole_set = True`
    (not a reference argument) returns what the method means instead: the product with the Hessian of the mean loss over
    ALL of `inds`, accumulated over the batches on the device (alq_hess_vecp with loss_scale = 1 / n and accumulate).

    Returns a list of float64 arrays: 'posteriors' -> [n] probability of class 1
    (PW_NN.py:526-529), 'prediction' -> [n], 'feature_layer' -> [fdim, n].  Patches are
    normalised with the channel-index rule of PW_NN.py:503-506 (channel j < m with stats[j]).
    `x_feed_dict = {model.keep_prob: p}` (PW_NN.py:516-521) evaluates with dropout on the model's dropout layers.
    `_first_sample` (not a reference argument): the position of inds[0] in the caller's whole evaluation - dropout masks
    are keyed by it, so an evaluation cut into blocks (pool_shard.work_block) draws the masks of the uncut one.
    `batch_size` only bounds the reference's feed size; samples are independent, so the device
    path walks the same index order in larger chunks.
    """
    if not isinstance(varnames, list):
        varnames = [varnames]
    for v in varnames:
        if v not in ('posteriors', 'prediction', 'feature_layer') + _LABELLED:
            raise NotImplementedError("batch_eval variable %r is outside the scored path" % v)
    labelled = {v: _eval_labelled(model, sess, img_dat, inds, patch_shape, batch_size, stats, v, mask, x_feed_dict, _vols, _whole_set)
                for v in varnames if v in _LABELLED}
    if len(labelled) == len(varnames):
        return [labelled[v] for v in varnames]
    keep_prob, mc, seed = mc_dropout_args(model, x_feed_dict)
    if mc and 'feature_layer' in varnames:
        raise NotImplementedError('feature_layer at keep_prob < 1')
    want_pred = 'prediction' in varnames
    want_feat = 'feature_layer' in varnames
    n = len(np.asarray(inds))
    posts = np.zeros(n)
    preds = np.zeros(n)
    feats = np.zeros((model.feature_dim, n)) if want_feat else None
    for a, b, post, pred, feat in _eval_passes(model, sess, img_dat, inds, patch_shape, batch_size, stats, (keep_prob, mc, seed),
                                               want_pred, want_feat, _vols, _first_sample):
        posts[a:b] = post[1].cpu().numpy()
        if want_pred:
            preds[a:b] = pred.cpu().numpy()
        if want_feat:
            f = feat.cpu().numpy()
            if model._feature_perm is not None:
                f = f[:, model._feature_perm]
            feats[:, a:b] = f.T
    out = []
    for v in varnames:
        out.append(labelled[v] if v in labelled else {'posteriors': posts, 'prediction': preds, 'feature_layer': feats}[v])
    return out
