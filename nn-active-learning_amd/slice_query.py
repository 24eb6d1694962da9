"""Slice queries for fully-convolutional models: which axial slices of the unlabelled subjects to label next.

NOT in the reference.  Its FCN branch stops at whole (c, h, w, z) uncertainty volumes on the host
(eval_utils.full_slice_segment: 'MC-posterior', 'sigma', 'MC-sigma'; eval_utils.py:176-198) and takes the queried slices as
`slice_img_inds` in get_dat_for_FT (datasets/data_holders.py:360); the selection between the two lived in scripts that were
never published.  This module is that step: per-voxel uncertainty reduced to per-slice scores on the device
(csrc/sliceq.hip: alq_unc_accumulate, alq_slice_scores), and `query_slices`, whose result is the argument of get_dat_for_FT.

Per voxel, with h(p) = -sum_j p_j log p_j in fp64 (a term with p_j <= 0 is exactly 0):
  'entropy'     h(p) of one pass at keep_prob 1
  'MC-entropy'  h(mean_t p_t) over T dropout passes
  'BALD'        h(mean_t p_t) - mean_t h(p_t)
  'AU'          the log-variance map of an AU_4U model (`AU_vals`)
A slice's score is the mean over its ROI voxels.  `slice_scores_host` is the NumPy fp64 statement of both kernels."""
import numpy as np

from . import eval_utils

KINDS = {'entropy': 0, 'MC-entropy': 1, 'BALD': 2, 'AU': 3}          # ALQ_UNC_ENTROPY, _MC_ENTROPY, _BALD, _MEAN (alq.h)
MC_METHODS = ('MC-entropy', 'BALD')


# ------------------------------------------------------------------------------------------------ the host statement
def _plogp(p):
    """p log p in fp64, exactly 0 where p <= 0."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(p <= 0, 0., p * np.log(p))


def slice_scores_host(post_passes, kind, roi=None, au=None):
    """alq_unc_accumulate + alq_slice_scores in NumPy fp64.
    post_passes: [T, c, n_slices, V] posteriors of T passes ([c, n_slices, V]: one pass; None for 'AU'); kind: a key of KINDS
    ('entropy' reads pass 0); roi: [n_slices, V], a voxel counts where it is non-zero (None: all); au: [n_slices, V], the map
    of 'AU'.  Returns (sums float64 [n_slices], counts int64 [n_slices], abs_sums float64 [n_slices]): the per-slice sum over
    the ROI, the number of ROI voxels, and the sum of the absolute value of every term that entered - |p log p| of the mean
    posteriors, plus |p log p| / T of every pass for 'BALD'; |a| for 'AU' - which is what an error bound of the sum scales with."""
    if kind not in KINDS:
        raise ValueError('unknown kind %r' % (kind,))
    if kind == 'AU':
        val = np.asarray(au, dtype=np.float64)
        mag = np.abs(val)
    else:
        P = np.asarray(post_passes)
        if P.ndim == 3:
            P = P[None]
        T = P.shape[0]
        if kind == 'entropy':
            t = _plogp(P[0])
            val, mag = -t.sum(axis=0), np.abs(t).sum(axis=0)
        else:
            t = _plogp(P.astype(np.float64).sum(axis=0) / T)          # (the fp64 sum of fp32 values is exact)
            val, mag = -t.sum(axis=0), np.abs(t).sum(axis=0)
            if kind == 'BALD':
                sum_h, sum_a = np.zeros(val.shape), np.zeros(val.shape)
                for k in range(T):          # pass by pass, as the device accumulates
                    tk = _plogp(P[k])
                    sum_h = sum_h + (-tk.sum(axis=0))
                    sum_a = sum_a + np.abs(tk).sum(axis=0)
                val = val - sum_h / T
                mag = mag + sum_a / T
    inside = np.ones(val.shape, dtype=bool) if roi is None else np.asarray(roi).reshape(val.shape) != 0
    sums = np.where(inside, val, 0.).sum(axis=1)
    abs_sums = np.where(inside, mag, 0.).sum(axis=1)
    return sums, inside.sum(axis=1).astype(np.int64), abs_sums


# ------------------------------------------------------------------------------------------------ scores of one subject
def _check_model(model, method):
    if method not in KINDS:
        raise ValueError('unknown method %r (one of %s)' % (method, ', '.join(sorted(KINDS))))
    if not getattr(model, 'dense', False):
        raise NotImplementedError('slice queries are defined for a fully-convolutional model (1x1 conv head)')
    if method == 'AU' and not getattr(model, 'AU_4U', False):
        raise NotImplementedError("method 'AU' needs a model with an aleatoric-uncertainty head (AU_4U)")
    if method in MC_METHODS and not len(getattr(model, 'dropout_layers', ())):
        raise ValueError('method %r needs a model with a dropout layer' % (method,))


def _device_slices(sess, imgs):
    """The subject as float32 device [z, h, w, m] (the layout of a batch): a resident subject's own tensor, else one upload."""
    subject = getattr(imgs, 'subject', None)
    if subject is not None:
        return subject.vol
    vols = imgs if isinstance(imgs, (list, tuple)) else [imgs]
    vols = [np.asarray(v, dtype=np.float32) for v in vols]
    if any(v.ndim != 3 or v.shape != vols[0].shape for v in vols):
        raise ValueError('the images of a subject are (h, w, z) arrays of one shape, got %r' % ([v.shape for v in vols],))
    return sess.to_device(np.ascontiguousarray(np.stack(vols, axis=-1).transpose(2, 0, 1, 3)), sess.torch.float32)


def _device_roi(sess, roi, vol):
    """uint8 device [z, h, w] (None: all voxels)."""
    torch = sess.torch
    if roi is None:
        return None
    if isinstance(roi, str):
        if roi != 'nonzero':
            raise ValueError("roi is None, 'nonzero' or an (h, w, z) array, got %r" % (roi,))
        return (vol != 0).any(dim=-1).to(torch.uint8).contiguous()
    roi = np.asarray(roi)
    z, h, w = (int(v) for v in vol.shape[:3])
    if roi.shape != (h, w, z):
        raise ValueError('roi of shape %r for images of shape %r' % (roi.shape, (h, w, z)))
    return sess.to_device(np.ascontiguousarray((roi != 0).transpose(2, 0, 1)).astype(np.uint8), torch.uint8)


def device_slice_sums(model, sess, vol, method, roi=None, T=eval_utils.MC_PASSES, seed=0, batch=None, tap=None):
    """The per-slice sums and ROI counts of a subject on the device: (float64 [z], int64 [z]) device tensors.  vol: float32
    device [z, h, w, m]; roi: uint8 device [z, h, w] or None.  tap(a, b, k, x): called with every map the kernels consume -
    slices a .. b - 1, pass k, x the posteriors [c, (b - a) V] or the AU map - for tools and tests that restate the result."""
    torch = sess.torch
    z = int(vol.shape[0])
    if tuple(int(v) for v in vol.shape[1:]) != tuple(model.in_shape):
        raise ValueError('slices of shape %r for a model of input shape %r' % (tuple(vol.shape[1:]), tuple(model.in_shape)))
    if roi is not None and tuple(int(v) for v in roi.shape) != (z,) + tuple(model.out_map_shape):
        raise ValueError('a ROI of shape %r for %d output maps of shape %r' % (tuple(roi.shape), z, tuple(model.out_map_shape)))
    T, c, V = int(T), int(model.nclass), int(model.out_voxels)
    if method in MC_METHODS and T < 1:
        raise ValueError('T = %d passes' % T)
    batch = int(model.max_batch if batch is None else batch)
    if batch < 1:
        raise ValueError('batch = %d' % batch)
    kp = 1. - float(model.dropout_rate) if method in MC_METHODS else 1.
    scores = sess.empty((z,), torch.float64)
    counts = sess.empty((z,), torch.int64)
    if method in MC_METHODS:
        sum_p = sess.empty((c * min(batch, z) * V,), torch.float64)
        sum_h = sess.empty((min(batch, z) * V,), torch.float64) if method == 'BALD' else None
    for a in range(0, z, batch):
        b = min(z, a + batch)
        n = b - a
        x = vol[a:b]
        out = dict(roi=None if roi is None else roi[a:b], scores=scores[a:b], counts=counts[a:b])
        if method == 'entropy':
            post = model.forward_device(x, n)[0]
            if tap is not None:
                tap(a, b, 0, post)
            sess.slice_scores(KINDS[method], n, V, c, f32=post, **out)
        elif method == 'AU':
            au = model.forward_au_device(x, n, 1., want_output=False)[0].reshape(-1)
            if tap is not None:
                tap(a, b, 0, au)
            sess.slice_scores(KINDS[method], n, V, c, f32=au, **out)
        else:
            sp = sum_p[:c * n * V].view(c, n * V)
            sh = None if sum_h is None else sum_h[:n * V]
            for k in range(T):
                # the slice index is the sample id of the masks: a slice draws the same mask in every batching
                post = model.forward_dropout_device(x, n, kp, seed=int(seed) + k, first_sample=a)[0]
                if tap is not None:
                    tap(a, b, k, post)
                sess.unc_accumulate(post, sp, sh, first=k == 0)
            sess.slice_scores(KINDS[method], n, V, c, T=T, sum_p=sp, sum_h=sh, **out)
    return scores, counts


def slice_scores(model, sess, imgs, method, roi=None, T=eval_utils.MC_PASSES, seed=0, batch=None):
    """(mean score float64 [z], ROI voxels int64 [z]) of every axial slice of one subject; a slice with no ROI voxel scores -inf.
    imgs: one (h, w, z) array, a list of m of them (the input channels), or the images of a resident subject
    (`dat.tr_imgs[i]` after `load_images(sess)`: read where they lie, nothing is uploaded).  roi: None (all voxels), an
    (h, w, z) array (non-zero: inside) or 'nonzero' (voxels where any channel is non-zero).
    method: 'entropy' (one pass at keep_prob 1); 'MC-entropy' / 'BALD' (T passes at keep_prob = 1 - model.dropout_rate, pass t
    with seed `seed + t`; the masks are keyed by the slice index, so the scores do not depend on `batch`); 'AU' (the
    log-variance map of an AU_4U model).  Slices go through the model in ascending order, `batch` (default model.max_batch) at a
    time; the sums stay on the device and 8 z + 8 z bytes come back."""
    _check_model(model, method)
    vol = _device_slices(sess, imgs)
    sums, counts = device_slice_sums(model, sess, vol, method, _device_roi(sess, roi, vol), T, seed, batch)
    return mean_scores(sums.cpu().numpy(), counts.cpu().numpy())


def mean_scores(sums, counts):
    """sums / counts, -inf where a slice has no ROI voxel."""
    sums, counts = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.int64)
    out = np.full(sums.shape, -np.inf)
    np.divide(sums, counts, out=out, where=counts > 0)
    return out, counts


# ------------------------------------------------------------------------------------------------ the query
def pick_slices(scores, counts, k):
    """The k largest scores of a pool given per subject (lists of arrays [z_i]); ties go to the lower (subject, slice); a slice
    with count 0 is never chosen.  Returns one sorted int array per subject (empty where nothing was chosen)."""
    sizes = [len(s) for s in scores]
    flat = np.concatenate([np.asarray(s, dtype=np.float64) for s in scores]) if sizes else np.zeros(0)
    cnt = np.concatenate([np.asarray(v, dtype=np.int64) for v in counts]) if sizes else np.zeros(0, dtype=np.int64)
    k = int(k)
    if k < 0 or k > len(flat):
        raise ValueError('k = %d slices out of a pool of %d' % (k, len(flat)))
    eligible = np.where(cnt > 0)[0]
    if k > len(eligible):
        raise ValueError('k = %d slices, but only %d of the pool hold a ROI voxel' % (k, len(eligible)))
    order = eligible[np.argsort(-flat[eligible], kind='stable')][:k]          # stable: equal scores stay in (subject, slice) order
    return _split(np.sort(order), sizes)


def _split(flat_inds, sizes):
    ends = np.cumsum([0] + list(sizes))
    return [np.asarray(flat_inds[(flat_inds >= ends[i]) & (flat_inds < ends[i + 1])] - ends[i], dtype=np.int64) for i in range(len(sizes))]


def query_slices(model, sess, dat, method, k, roi='nonzero', T=eval_utils.MC_PASSES, seed=0):
    """The k slices to label next out of every slice of the unlabelled training subjects of a loaded
    datasets.data_holders.regular (`dat.tr_imgs[int(sum(dat.L_indic)):]`): those with the largest mean score of `method`
    (slice_scores; ties to the lower (subject, slice); a slice without a ROI voxel is never chosen), or - method 'random' - k
    of the pool drawn with np.random.permutation, nothing launched.  Returns `slice_img_inds`, one sorted int array per
    unlabelled subject: the argument of datasets.data_holders.get_dat_for_FT.  k larger than the pool: ValueError."""
    first = int(np.sum(dat.L_indic))
    pool = dat.tr_imgs[first:]
    sizes = [int(_depth(imgs)) for imgs in pool]
    k = int(k)
    if k < 0 or k > sum(sizes):
        raise ValueError('k = %d slices out of a pool of %d' % (k, sum(sizes)))
    if method == 'random':
        return _split(np.sort(np.random.permutation(sum(sizes))[:k]), sizes)
    _check_model(model, method)
    scores, counts = [], []
    for imgs in pool:
        s, n = slice_scores(model, sess, imgs, method, roi=roi, T=T, seed=seed)
        scores.append(s)
        counts.append(n)
    return pick_slices(scores, counts, k)


def _depth(imgs):
    shape = getattr(imgs, 'shape', None)          # a resident subject's images answer .shape = (H, W, Z)
    return shape[2] if shape is not None and len(shape) == 3 else np.shape(imgs[0])[2]
