"""Plain NumPy restatement of the region primitives of csrc/region.hip and csrc/ccl.hip: the d x d local-variance map of
patch_utils.get_vars_2d (patch_utils.py:794-826) and the per-(slice, label) score minimum of PW_NNAL.superpix_scoring
(PW_NNAL.py:944-1021).  Host code: the reference of the kernel tests and of the tool, and the documentation of the formulas
(include/alq.h).  No scipy in the first two: the box sums are integer prefix sums, which is what scipy's float64 convolution of
the uint64 image equals wherever it is exact (check_variance_input).  The component functions at the end (cc_label_host,
keep_largest_host, fill_holes_host) state alq_cc_label / alq_cc_keep_largest / alq_fill_holes through scipy.ndimage.  The
SLIC over-segmentation has a module of its own for its statement (slic.py); oversegment / slic_device at the end of this one are
its entry point and its device driver (alq_slic)."""
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


# ---- connected components, largest component, hole filling: the semantics of csrc/ccl.hip ------------------------------------
_CC_RANK = {6: 1, 18: 2, 26: 3}


def _as_volume(seg):
    a = np.asarray(seg)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise ValueError('2-D image or 3-D volume expected')
    return a


def cc_label_host(seg, connectivity=26, select_zero=False):
    """The labels of alq_cc_label on the host (scipy.ndimage.label; never on the product path): int32, for a selected voxel
    (!= 0; == 0 with select_zero) the smallest raveled index of its component, -1 elsewhere.  connectivity 6 / 18 / 26 =
    scipy's generate_binary_structure(3, 1 / 2 / 3); a 2-D image is the volume [H, W, 1]."""
    from scipy import ndimage
    a = _as_volume(seg)
    sel = (a == 0) if select_zero else (a != 0)
    lab, n = ndimage.label(sel, structure=ndimage.generate_binary_structure(3, _CC_RANK[int(connectivity)]))
    out = np.full(a.shape, -1, dtype=np.int32)
    if n:
        flat = lab.reshape(-1)
        _, first = np.unique(flat, return_index=True)              # first[l] = the first raveled index with label l (0 = background)
        if flat.min() != 0:                                        # no background voxel: label 1 is first[0]
            first = np.concatenate([[0], first])
        out = np.where(lab > 0, first[lab], -1).astype(np.int32)
    return out.reshape(np.asarray(seg).shape)


def keep_largest_host(seg, connectivity=26, skip_origin=True, with_info=False):
    """alq_cc_keep_largest on the host: uint8 mask of the largest component of the non-zero voxels; equal sizes -> the
    component whose first voxel comes first in C order; skip_origin: the component of voxel 0 is no candidate.  with_info:
    (mask, np.int64 [4] = candidates, winner's root or -1, its size, non-zero voxels).  No candidate: all zero."""
    a = np.asarray(seg)
    lab = cc_label_host(a, connectivity).reshape(-1)
    roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
    if skip_origin and lab[0] >= 0:
        keep = roots != lab[0]
        roots, sizes = roots[keep], sizes[keep]
    info = np.array([len(roots), -1, 0, int(np.count_nonzero(a))], dtype=np.int64)
    out = np.zeros(a.shape, dtype=np.uint8)
    if len(roots):
        w = int(np.argmax(sizes))                                  # the first maximum; roots ascend
        info[1], info[2] = roots[w], sizes[w]
        out = (lab == roots[w]).astype(np.uint8).reshape(a.shape)
    return (out, info) if with_info else out


def fill_holes_host(seg, with_info=False):
    """alq_fill_holes on the host: uint8 mask = scipy.ndimage.binary_fill_holes(seg) of the 3-D volume (default structure: the
    zero voxels are 6-connected, and a zero voxel next to any of the six faces is outside).  A 2-D image is the volume
    [H, W, 1], every voxel of which lies on a face: nothing is filled, as scipy has it for that 3-D array.  with_info:
    (mask, np.int64 [4] = enclosed background components, voxels filled, 0, 0)."""
    from scipy import ndimage
    a = _as_volume(seg)
    out = ndimage.binary_fill_holes(a != 0).astype(np.uint8)
    filled = (out != 0) & (a == 0)
    out = out.reshape(np.asarray(seg).shape)
    if not with_info:
        return out
    n = ndimage.label(filled)[1]                                   # default structure: face neighbours
    return out, np.array([n, int(filled.sum()), 0, 0], dtype=np.int64)


# ---- SLIC over-segmentation: slic.py states it, csrc/slic.hip runs it -------------------------------------------------------
def slic_device(sess, vol, gh, gw, w, T=10, min_size=0, mask=None, lo=None, scale=None, hwz=True, work=None):
    """alq_slic on a packed subject: `vol` float32 device tensor [Z, H, W, m] (alq_vol_pack), `mask` uint8 device tensor
    [Z, H, W] (255 = out) or None, lo / scale [m] host values.  -> (labels int32 device tensor, [H, W, S] with hwz else
    [S, H, W]; n_per_slice int32 device tensor [S]).  Stream-ordered: nothing is read back."""
    import ctypes as C
    from ._lib import check, ptr
    torch = sess.torch
    Z, H, W, m = (int(v) for v in vol.shape)
    dims = (C.c_int64 * 3)(H, W, Z)
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    if len(lo) != m or len(scale) != m:
        raise ValueError('slic: %d / %d quantisation values for %d channels' % (len(lo), len(scale), m))
    sess.bind_stream()
    labels = sess.empty((H, W, Z) if hwz else (Z, H, W), torch.int32)
    counts = sess.empty((Z,), torch.int32)
    if work is None:
        nbytes = int(sess.lib.alq_slic_work_bytes(dims, m, int(gh), int(gw)))
        work = sess.empty((max(nbytes, 8) // 8,), torch.int64)
    check(sess.lib.alq_slic(sess.ctx, ptr(vol), ptr(mask), dims, m,
                            (C.c_double * m)(*lo), (C.c_double * m)(*scale), int(gh), int(gw), float(w), int(T), int(min_size),
                            1 if hwz else 0, ptr(labels), ptr(counts), ptr(work)))
    return labels, counts


def _device_quant_range(sess, vol, mask):
    """slic.quant_range on a packed device subject (the minimum and maximum are float32 values: the same doubles)."""
    torch = sess.torch
    lo, scale = [], []
    for c in range(int(vol.shape[3])):
        a = vol[..., c]
        ok = torch.isfinite(a) if mask is None else (torch.isfinite(a) & (mask != 255))
        vals = a[ok]
        if int(vals.numel()) == 0:
            lo.append(0.0)
            scale.append(0.0)
            continue
        mn, mx = float(vals.min().item()), float(vals.max().item())
        lo.append(mn)
        scale.append(65535 / (mx - mn) if mx > mn else 0.0)
    return np.array(lo), np.array(scale)


def oversegment(vols_or_array, n_segments=100, compactness=0.1, T=10, min_size=0, mask=None, sess=None, keep_on_device=False,
                with_counts=False):
    """The SLIC over-segmentation of a subject (slic.py: skimage-LIKE arguments, not skimage's algorithm): int32 labels
    [H, W, S], 0 on out pixels and 1 .. n_z per slice; with_counts: (labels, n_per_slice int32 [S]).
    vols_or_array: a datasets.utils.ResidentSubject (already on the device), one volume [H, W, S], an array [m, H, W, S] or a
    list of m volumes; mask: bool [H, W, S], True = in.  gh, gw = slic.grid_for(H, W, n_segments), w =
    slic.spatial_weight(compactness, H, W, gh, gw), the quantisation range = the subject's finite in-mask minimum and maximum per
    channel.  Without a session this is slic.slic_host; with one the subject is packed (if it is not resident) and alq_slic runs
    it.  keep_on_device=True (needs a session): device tensors, nothing is copied back."""
    from . import slic
    resident = hasattr(vols_or_array, 'vol') and hasattr(vols_or_array, 'shape')
    if sess is None and resident:
        sess = vols_or_array.sess
    if sess is None:
        if keep_on_device:
            raise ValueError('oversegment: keep_on_device needs a session')
        mods = slic.as_modalities(vols_or_array)
        H, W, _ = mods[0].shape
        gh, gw = slic.grid_for(H, W, n_segments)
        out = slic.slic_host(mods, gh, gw, slic.spatial_weight(compactness, H, W, gh, gw), T, min_size, mask)
        return out if with_counts else out[0]
    torch = sess.torch
    if resident:
        vol = vols_or_array.vol
    else:
        from .datasets.utils import ResidentSubject
        vol = ResidentSubject.pack(sess, slic.as_modalities(vols_or_array)).vol
    Z, H, W, _ = (int(v) for v in vol.shape)
    d_mask = None
    if mask is not None:
        if hasattr(mask, 'data_ptr'):
            inm = mask.to(torch.bool)
        else:
            inm = torch.as_tensor(np.ascontiguousarray(np.asarray(mask, dtype=bool))).to(sess.device)
        if tuple(int(v) for v in inm.shape) != (H, W, Z):
            raise ValueError('oversegment: mask shape %r, subject %r' % (tuple(inm.shape), (H, W, Z)))
        d_mask = torch.where(inm, 0, 255).to(torch.uint8).permute(2, 0, 1).contiguous()
    gh, gw = slic.grid_for(H, W, n_segments)
    lo, scale = _device_quant_range(sess, vol, d_mask)
    labels, counts = slic_device(sess, vol, gh, gw, slic.spatial_weight(compactness, H, W, gh, gw), T, min_size, d_mask, lo, scale)
    if not keep_on_device:
        labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
    return (labels, counts) if with_counts else labels
