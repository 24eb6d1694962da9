"""Surface-distance metrics of a segmentation against a mask: Hausdorff distance (HD), its percentile form (HD95), average
symmetric surface distance (ASSD) and the modified Hausdorff distance of Dubuisson and Jain (MHD, iSeg-2017's measure).

This module is the NumPy statement of every device call of csrc/edt.hip (the *_host functions), the definition of the metrics
(`metrics`) and the public entry `surface_distances`, which runs either the statement (sess=None) or the device calls.

Definitions.  Volumes are [H, W, S] (an image [H, W] is a one-slice volume), spacing = (h, w, z) voxel sizes.
  * surface: a foreground voxel with a 6-neighbour that is background or outside the volume (`surface_host`); an axis of
    extent 1 has no neighbours.  Equal to seg & ~binary_erosion(seg, cross, border_value=0) on the squeezed array.
  * squared distance transform (`edt_sq_host`): g = 0 on a feature voxel, +inf elsewhere; then for the axes z, w, h in turn
        g[x] = min over x' of (g[x'] + s2 * float((x - x')**2)),  s2 = float64(s) * float64(s)
    with the product rounded, then the sum.  Rounding and + are monotone, so the result is the minimum over the feature
    voxels of ((s2z dz^2 + s2w dw^2) + s2h dh^2) in that association, bit for bit; the device kernels are held to equality.
  * with A the surface of the segmentation (n_a voxels), B that of the mask (n_b) and the directed distances
    d(a) = sqrt(edt_sq(B)[a]), d(b) = sqrt(edt_sq(A)[b]):
        HD    max of the two directed maxima (the square root of the exact maximum of d^2)
        HD95  max of the two directed q-percentiles (q = 95 by default), each np.percentile's linear interpolation between
              the order statistics floor and ceil of q / 100 * (n - 1).  This is the robust Hausdorff distance of DIRECTED
              quantiles; it is NOT MedPy's hd95, which pools both directions into one set before it takes the percentile.
        ASSD  (sum_ab + sum_ba) / (n_a + n_b)
        MHD   max(sum_ab / n_a, sum_ba / n_b)
    Both surfaces empty: every metric is 0.0; exactly one empty: every metric is inf."""
import math

import numpy as np


def _as3d(a):
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise ValueError('a volume [H, W, S] or an image [H, W] is expected, got shape %r' % (a.shape,))
    return a


def _spacing3(spacing):
    sp = [np.float64(s) for s in spacing]
    if len(sp) == 2:
        sp.append(np.float64(1.))
    if len(sp) != 3:
        raise ValueError('spacing has 2 or 3 entries')
    for s in sp:
        if not (np.isfinite(s) and s > 0):
            raise ValueError('spacing %r: every entry is finite and > 0' % (tuple(spacing),))
    return sp


def surface_host(seg, label=None):
    """The rule of alq_surface_mask: bool array of seg's shape."""
    seg = np.asarray(seg)
    fg = (seg != 0) if (label is None or label < 0) else (seg == label)
    surf = np.zeros(fg.shape, dtype=bool)
    for ax in range(fg.ndim):
        L = fg.shape[ax]
        if L <= 1:
            continue
        sl = [slice(None)] * fg.ndim
        for lo in (True, False):
            nb = np.zeros(fg.shape, dtype=bool)          # the neighbour's value, False outside the volume
            dst, src = list(sl), list(sl)
            dst[ax] = slice(1, None) if lo else slice(None, -1)
            src[ax] = slice(None, -1) if lo else slice(1, None)
            nb[tuple(dst)] = fg[tuple(src)]
            surf |= ~nb
    return fg & surf


def edt_sq_host(feat, spacing=(1., 1., 1.)):
    """The definition of alq_edt_sq (module text): float64 array of feat's shape.  O(n L) per axis, in whole-array steps."""
    feat = np.asarray(feat)
    f3 = _as3d(feat)
    sp = _spacing3(spacing)
    g = np.where(f3 != 0, 0.0, np.inf)
    for axis in (2, 1, 0):
        s2 = sp[axis] * sp[axis]
        L = g.shape[axis]
        out = g.copy()
        tmp = np.empty_like(g)
        for d in range(1, L):
            c = s2 * np.float64(d * d)
            if c >= out.max():      # exact: g >= 0, so no candidate at this distance or beyond is below c
                break
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(d, None), slice(None, -d)
            a, b = tuple(a), tuple(b)
            np.add(g[b], c, out=tmp[a])
            np.minimum(out[a], tmp[a], out=out[a])
            np.add(g[a], c, out=tmp[b])
            np.minimum(out[b], tmp[b], out=out[b])
        g = out
    return g.reshape(feat.shape)


def edt_sq_brute(feat, spacing=(1., 1., 1.)):
    """The single brute-force minimum over the feature voxels of ((s2z dz^2 + s2w dw^2) + s2h dh^2): what edt_sq_host equals
    bit for bit.  O(n * features): for small volumes (tests)."""
    feat = np.asarray(feat)
    f3 = _as3d(feat)
    sp = _spacing3(spacing)
    s2 = [s * s for s in sp]
    pts = np.argwhere(f3 != 0)
    H, W, S = f3.shape
    out = np.full(f3.shape, np.inf)
    hh, ww, zz = np.meshgrid(np.arange(H), np.arange(W), np.arange(S), indexing='ij')
    for i, j, k in pts:
        dz = (s2[2] * ((zz - k) ** 2).astype(np.float64))
        dw = (s2[1] * ((ww - j) ** 2).astype(np.float64))
        dh = (s2[0] * ((hh - i) ** 2).astype(np.float64))
        np.minimum(out, (dz + dw) + dh, out=out)
    return out.reshape(feat.shape)


def dist_stats_host(d2, mask):
    """The definition of alq_masked_dist_stats: np.float64 [4] = (count, sum of sqrt, max, min) of d2[mask != 0]."""
    v = np.asarray(d2, dtype=np.float64).ravel()[np.asarray(mask).ravel() != 0]
    if v.size == 0:
        return np.array([0.0, 0.0, -np.inf, np.inf])
    return np.array([float(v.size), float(np.sum(np.sqrt(v))), float(v.max()), float(v.min())])


def select_host(d2, mask, ranks):
    """The definition of alq_masked_select: the ranks[r]-th smallest of d2[mask != 0], NaN for a rank at or above the count."""
    v = np.sort(np.asarray(d2, dtype=np.float64).ravel()[np.asarray(mask).ravel() != 0])
    return np.array([v[r] if 0 <= r < v.size else np.nan for r in ranks], dtype=np.float64)


def percentile_ranks(n, q):
    """(floor, ceil, fraction) of the position q / 100 * (n - 1) in the sorted sample of n values."""
    pos = float(q) / 100. * (int(n) - 1)
    lo = int(math.floor(pos))
    hi = int(math.ceil(pos))
    return lo, hi, pos - lo


def interp_percentile(d2_lo, d2_hi, frac):
    """The percentile from the two selected squared distances: lo + (hi - lo) * frac on the square roots."""
    lo, hi = math.sqrt(d2_lo), math.sqrt(d2_hi)
    if frac == 0 or lo == hi:
        return lo
    return lo + (hi - lo) * frac


def metrics(stats_ab, stats_ba, order_ab, order_ba, q=95.):
    """The metrics from the reductions of the two directions.  stats_xy: (count, sum of distances, max d^2, min d^2) over the
    surface voxels of x against the distance map of y (dist_stats_host); order_xy: the two squared distances at the ranks
    percentile_ranks(count, q)[:2] of that direction (select_host), ignored for an empty direction.  a = segmentation, b = mask."""
    n_a, n_b = int(stats_ab[0]), int(stats_ba[0])
    res = {'n_seg': n_a, 'n_mask': n_b}
    if n_a == 0 or n_b == 0:
        v = 0.0 if n_a == n_b else float('inf')
        for k in ('HD', 'HD95', 'ASSD', 'MHD'):
            res[k] = v
        for d in ('seg_to_mask', 'mask_to_seg'):
            for k in ('mean', 'max', 'percentile'):
                res['%s_%s' % (k, d)] = v
        return res
    dirs = {}
    for name, st, od, n in (('seg_to_mask', stats_ab, order_ab, n_a), ('mask_to_seg', stats_ba, order_ba, n_b)):
        frac = percentile_ranks(n, q)[2]
        dirs[name] = (float(st[1]) / n, math.sqrt(float(st[2])), interp_percentile(float(od[0]), float(od[1]), frac))
        res['mean_' + name], res['max_' + name], res['percentile_' + name] = dirs[name]
    ab, ba = dirs['seg_to_mask'], dirs['mask_to_seg']
    res['HD'] = max(ab[1], ba[1])
    res['HD95'] = max(ab[2], ba[2])
    res['ASSD'] = (float(stats_ab[1]) + float(stats_ba[1])) / (n_a + n_b)
    res['MHD'] = max(ab[0], ba[0])
    return res


def _device_volume(vol, sess, shape, label):
    """-> (uint8 device tensor, shape [H, W, S]).  Device tensors are read in place; arrays are uploaded as their uint8 values
    when a label is asked for, else as the mask vol != 0 (post_processing._to_device)."""
    torch = sess.torch
    if isinstance(vol, torch.Tensor):
        shape = tuple(int(v) for v in (vol.shape if shape is None else shape))
        return vol, shape
    a = np.asarray(vol)
    if label is None or label < 0:
        a = a != 0
    elif a.size and not np.all((a >= 0) & (a <= 255) & (a == np.floor(a))):
        raise ValueError('a labelled volume holds integers 0 .. 255')
    return sess.to_device(a, torch.uint8), a.shape


def surface_distances(seg, mask, spacing=(1., 1., 1.), label=None, percentile=95., sess=None, shape=None):
    """Boundary metrics of `seg` against `mask` (module text): a dict with HD, HD95 (the `percentile`-th, 95 by default), ASSD,
    MHD, the surface voxel counts n_seg / n_mask and the directed mean_ / max_ / percentile_ values of seg_to_mask and
    mask_to_seg.  Foreground is != 0, or == label when a label is given.  `seg` / `mask`: arrays [H, W, S] or [H, W], or uint8
    device tensors with `shape` (read in place).  `spacing`: voxel sizes (h, w, z), two values for an image.
    sess=None evaluates the NumPy statement; with a DeviceSession the work is two alq_surface_mask, two alq_edt_sq, two
    alq_masked_dist_stats and two alq_masked_select calls - the volumes stay on the device, 32 + 16 bytes come back per
    direction.  HD, the counts and the selected order statistics are the same in both; the sums differ by rounding only.
    HD95 here is the maximum of the two DIRECTED percentiles, not MedPy's percentile of the pooled distances."""
    lab = None if (label is None or label < 0) else int(label)
    q = float(percentile)
    if not 0. <= q <= 100.:
        raise ValueError('percentile %r outside 0 .. 100' % (percentile,))
    if sess is None:
        a, b = _as3d(seg), _as3d(mask)
        if a.shape != b.shape:
            raise ValueError('shapes differ: %r, %r' % (a.shape, b.shape))
        sp = _spacing3(spacing)
        sa, sb = surface_host(a, lab), surface_host(b, lab)
        da, db = edt_sq_host(sa, sp), edt_sq_host(sb, sp)
        st_ab, st_ba = dist_stats_host(db, sa), dist_stats_host(da, sb)
        od_ab = select_host(db, sa, percentile_ranks(st_ab[0], q)[:2]) if st_ab[0] else None
        od_ba = select_host(da, sb, percentile_ranks(st_ba[0], q)[:2]) if st_ba[0] else None
        return metrics(st_ab, st_ba, od_ab, od_ba, q)
    d_a, shp_a = _device_volume(seg, sess, shape, lab)
    d_b, shp_b = _device_volume(mask, sess, shape, lab)
    shp_a, shp_b = (s + (1,) if len(s) == 2 else s for s in (shp_a, shp_b))
    if shp_a != shp_b:
        raise ValueError('shapes differ: %r, %r' % (shp_a, shp_b))
    sp = _spacing3(spacing)
    sa, sb = sess.surface_mask(d_a, shp_a, lab), sess.surface_mask(d_b, shp_a, lab)
    da, db = sess.edt_sq(sa, shp_a, sp), sess.edt_sq(sb, shp_a, sp)
    st_ab, st_ba = sess.masked_dist_stats(db, sa), sess.masked_dist_stats(da, sb)
    od_ab = sess.masked_select(db, sa, percentile_ranks(st_ab[0], q)[:2]) if st_ab[0] else None
    od_ba = sess.masked_select(da, sb, percentile_ranks(st_ba[0], q)[:2]) if st_ba[0] else None
    return metrics(st_ab, st_ba, od_ab, od_ba, q)
