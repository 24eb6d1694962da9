"""Whole-volume inference of a fully-convolutional model by overlapping tiles: the NumPy statement of csrc/tile.hip, fp32
operation by operation (no reference counterpart: the reference builds one model per image size).  The device functions equal
these bit for bit; `eval_utils.full_volume_segment` is the call site.

The lattice.  Along an axis of length D with tile t and stride s (1 <= s <= t): D <= t gives one tile at origin 0, which
overhangs the volume by t - D at the high end; otherwise there are ceil((D - t) / s) + 1 tiles at min(i s, D - t) - the last one
is clamped so that it ends with the volume.  Axes are ordered (Z, H, W) and tile (iz, ih, iw) has the index (iz nH + ih) nW + iw.

The blend.  Every tile's posteriors are weighted by a separable window w = (wz[lz] wh[lh]) ww[lw] and added into c sums and a
weight sum per voxel, in ascending tile index, every product and sum rounded to fp32 on its own; the result is the quotient.
The order is part of the definition: it makes the bytes independent of how the tiles are batched."""
import numpy as np

WINDOWS = ('uniform', 'triangle', 'gaussian')
MAX_C, MIN_C, MAX_M = 8, 2, 8


def lattice_origins(D, t, s):
    """The tile origins along one axis: int64 [n]."""
    D, t, s = int(D), int(t), int(s)
    if D < 1 or t < 1 or s < 1 or s > t:
        raise ValueError('axis of %d voxels, tile %d, stride %d: all at least 1 and the stride at most the tile' % (D, t, s))
    if D <= t:
        return np.zeros(1, dtype=np.int64)
    n = -(-(D - t) // s) + 1
    return np.minimum(np.arange(n, dtype=np.int64) * s, D - t)


def tile_counts(dims, tile, stride):
    return tuple(len(lattice_origins(D, t, s)) for D, t, s in zip(dims, tile, stride))


def tile_origins(dims, tile, stride):
    """The origins (oz, oh, ow) of every tile in index order: int64 [n tiles, 3]."""
    oz, oh, ow = (lattice_origins(D, t, s) for D, t, s in zip(dims, tile, stride))
    return np.stack([g.reshape(-1) for g in np.meshgrid(oz, oh, ow, indexing='ij')], axis=1)


def default_stride(tile):
    """Half a tile per axis, at least 1."""
    return tuple(max(int(t) // 2, 1) for t in tile)


def window(name, t):
    """The window table of an axis with tile t: float32 [t], computed in fp64 and rounded once.  'uniform': ones; 'triangle':
    min(l + 1, t - l), small integers (sums of them are exact); 'gaussian': exp(-0.5 ((l - (t - 1) / 2) / (t / 8))^2)."""
    t = int(t)
    l = np.arange(t, dtype=np.float64)
    if name == 'uniform':
        w = np.ones(t, dtype=np.float64)
    elif name == 'triangle':
        w = np.minimum(l + 1., t - l)
    elif name == 'gaussian':
        w = np.exp(-0.5 * ((l - (t - 1) / 2.) / (t / 8.)) ** 2)
    else:
        raise ValueError('window %r (one of %r)' % (name, WINDOWS))
    return w.astype(np.float32)


def gather_host(vol, tile, stride, first=0, n=None, fill=0.):
    """alq_tile_gather: vol float32 [Z, H, W, m] -> X [n, tz, th, tw, m], the tiles first .. first + n - 1; what lies outside the
    volume is `fill`."""
    vol = np.asarray(vol, dtype=np.float32)
    Z, H, W, m = vol.shape
    org = tile_origins((Z, H, W), tile, stride)
    n = len(org) - first if n is None else n
    tz, th, tw = (int(v) for v in tile)
    X = np.full((n, tz, th, tw, m), np.float32(fill), dtype=np.float32)
    for j in range(n):
        oz, oh, ow = (int(v) for v in org[first + j])
        src = vol[oz:oz + tz, oh:oh + th, ow:ow + tw]
        X[j, :src.shape[0], :src.shape[1], :src.shape[2]] = src
    return X


def blend_host(acc, post, tile, stride, wz, wh, ww, first=0, n=None):
    """alq_tile_blend on acc float32 [c + 1, Z, H, W] (updated in place and returned) with post float32 [c, n V].  The brute-force
    definition: every voxel meets ALL tiles of the lattice in index order; a tile counts where it covers the voxel (tested per
    axis: origin <= x < origin + t) and lies in first .. first + n - 1.  (The loop over the tiles is the outer one, the voxels of
    the volume are tested together: each voxel's additions still run in ascending tile index.)"""
    assert acc.dtype == np.float32 and acc.ndim == 4
    c = acc.shape[0] - 1
    Z, H, W = acc.shape[1:]
    tz, th, tw = (int(v) for v in tile)
    V = tz * th * tw
    org = tile_origins((Z, H, W), tile, stride)
    n = len(org) - first if n is None else n
    post = np.asarray(post, dtype=np.float32).reshape(c, n, tz, th, tw)
    wz, wh, ww = (np.asarray(v, dtype=np.float32) for v in (wz, wh, ww))
    assert wz.shape == (tz,) and wh.shape == (th,) and ww.shape == (tw,) and V * n == post[0].size
    z, h, w = np.arange(Z), np.arange(H), np.arange(W)
    for idx in range(len(org)):
        if not first <= idx < first + n:
            continue
        oz, oh, ow = (int(v) for v in org[idx])
        zs, hs, ws = z[(z >= oz) & (z < oz + tz)], h[(h >= oh) & (h < oh + th)], w[(w >= ow) & (w < ow + tw)]
        at = np.ix_(zs, hs, ws)
        lat = np.ix_(zs - oz, hs - oh, ws - ow)
        wt = (wz[zs - oz][:, None, None] * wh[hs - oh][None, :, None]) * ww[ws - ow][None, None, :]          # fp32, rounded twice
        for k in range(c):
            acc[k][at] = acc[k][at] + wt * post[k, idx - first][lat]
        acc[c][at] = acc[c][at] + wt
    return acc


def finalize_host(acc, hwz=False):
    """alq_tile_finalize: (q float32 [c, ...] = acc[k] / acc[c], label uint8 = the first maximum of q over k), in [Z, H, W] order or,
    with hwz, [H, W, Z].  The maximum is taken by strict comparison from class 0 up (a NaN never wins)."""
    c = acc.shape[0] - 1
    with np.errstate(divide='ignore', invalid='ignore'):
        q = acc[:c] / acc[c][None]
    best, label = q[0].copy(), np.zeros(q.shape[1:], dtype=np.uint8)
    for k in range(1, c):
        better = q[k] > best
        best = np.where(better, q[k], best)
        label[better] = k
    if hwz:
        q, label = np.ascontiguousarray(q.transpose(0, 2, 3, 1)), np.ascontiguousarray(label.transpose(1, 2, 0))
    return q, label


def segment_host(tile_post, dims, tile, stride, window_name='gaussian', hwz=True, ranges=None):
    """The whole statement after the forward passes: tile_post float32 [c, n tiles, tz, th, tw] (the model's posteriors of every
    tile) -> finalize_host of the blend over all tiles (`ranges`: the (first, n) cuts to blend in; None: one call)."""
    c = tile_post.shape[0]
    ntiles = tile_post.shape[1]
    wz, wh, ww = (window(window_name, t) for t in tile)
    acc = np.zeros((c + 1,) + tuple(int(d) for d in dims), dtype=np.float32)
    V = int(np.prod(tile))
    flat = np.ascontiguousarray(tile_post, dtype=np.float32).reshape(c, ntiles, V)
    for first, n in (ranges or [(0, ntiles)]):
        blend_host(acc, np.ascontiguousarray(flat[:, first:first + n]).reshape(c, n * V), tile, stride, wz, wh, ww, first, n)
    return finalize_host(acc, hwz)
