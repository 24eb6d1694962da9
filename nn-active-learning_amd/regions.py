"""Plain NumPy restatement of the two region primitives of csrc/region.hip: the d x d local-variance map of
patch_utils.get_vars_2d (patch_utils.py:794-826) and the per-(slice, label) score minimum of PW_NNAL.superpix_scoring
(PW_NNAL.py:944-1021).  Host code: the reference of the kernel tests and of the tool, and the documentation of the formulas
(include/alq.h).  No scipy: the box sums are integer prefix sums, which is what scipy's float64 convolution of the uint64 image
equals wherever it is exact (check_variance_input)."""
import numpy as np

MAX_D = 65


def check_variance_input(img, d):
    """The precondition of the variance map, checked once where a volume is handed over: every value finite and >= 0, and
    trunc(max)^2 d^2 < 2^53.  Inside these limits scipy's float64 accumulation and the 64-bit integer sums are both exact;
    outside them the reference itself is inexact (or its uint64 cast wraps).  Raises ValueError."""
    d = int(d)
    if d < 1 or d > MAX_D:
        raise ValueError('window size %d outside [1, %d]' % (d, MAX_D))
    a = np.asarray(img)
    if a.size == 0:
        raise ValueError('empty image')
    if a.dtype.kind == 'f':
        if not np.all(np.isfinite(a)):
            raise ValueError('the variance map needs finite values (NaN or inf found)')
    elif a.dtype.kind not in 'iub':
        raise ValueError('the variance map needs a real-valued image, not %s' % a.dtype)
    lo, hi = a.min(), a.max()
    if lo < 0:
        raise ValueError('the variance map needs values >= 0 (np.uint64 wraps negatives): min = %r' % (lo,))
    t = int(np.trunc(hi))
    if t * t * d * d >= 2 ** 53:
        raise ValueError('trunc(max)^2 d^2 = %d^2 * %d^2 >= 2^53: the sums of squares are no longer exact in float64' % (t, d))


def _box_sum(a, d, axis):
    """sum over [x - d//2, x + (d-1)//2] along `axis`, clipped (zero fill); `a` uint64."""
    n = a.shape[axis]
    shp = list(a.shape)
    shp[axis] = 1
    c = np.concatenate([np.zeros(shp, dtype=np.uint64), np.cumsum(a, axis=axis, dtype=np.uint64)], axis=axis)
    x = np.arange(n)
    hi = np.minimum(x + (d - 1) // 2, n - 1) + 1
    lo = np.maximum(x - d // 2, 0)
    return np.take(c, hi, axis=axis) - np.take(c, lo, axis=axis)      # modular uint64: exact


def local_var2d_host(vol, d, rads=(0, 0, 0)):
    """The map of alq_local_var2d on the host.  `vol`: a 2-D image -> float64 [H, W]; a zero-padded 3-D volume -> float64
    [H, W, S] over the un-padded box vol[r0:D0-r0, r1:D1-r1, r2:D2-r2], every slice [:, :, z] filtered on its own."""
    d = int(d)
    a = np.asarray(vol)
    if a.ndim == 3:
        r = [int(v) for v in rads]
        a = a[r[0]:a.shape[0] - r[0], r[1]:a.shape[1] - r[1], r[2]:a.shape[2] - r[2]]
    elif a.ndim != 2:
        raise ValueError('2-D image or 3-D volume expected')
    t = np.trunc(a).astype(np.uint64) if a.dtype.kind == 'f' else a.astype(np.uint64)
    s1 = _box_sum(_box_sum(t, d, 0), d, 1)
    s2 = _box_sum(_box_sum(t * t, d, 0), d, 1)
    dd = float(d * d)
    ex = s1.astype(np.float64) / dd
    ex2 = s2.astype(np.float64) / dd
    return ex2 - ex * ex


def segment_min_host(labels, inds, scores, n_labels=None):
    """The table of alq_segment_min on the host: float64 [S, n_labels], +inf everywhere, then entry (z, l) = the minimum
    score of the scored voxels (raveled indices `inds` into `labels` [H, W, S]) of slice z with label l, 1 <= l < n_labels.
    n_labels defaults to labels.max() + 1."""
    labels = np.asarray(labels)
    inds = np.asarray(inds, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float64)
    if n_labels is None:
        n_labels = int(labels.max()) + 1
    S = labels.shape[2]
    table = np.full((S, int(n_labels)), np.inf)
    ok = (inds >= 0) & (inds < labels.size)
    lab = labels.reshape(-1)[inds[ok]].astype(np.int64)
    z = inds[ok] % S
    keep = (lab >= 1) & (lab < n_labels)
    np.minimum.at(table, (z[keep], lab[keep]), scores[ok][keep])
    return table
