"""Max pooling as csrc/kernels.hip states it, restated in NumPy: the reference of tests/test_pool_host.py (which holds it to
oracle/tfops.max_pool_same and to torch autograd) and of tests/test_gpu_pool.py (which holds the pool kernels to it).

Max pooling selects and moves values and does no arithmetic, so everything here but the channel sums is exact: values,
arg-max bytes and routed cotangents are compared on equal bits.

Geometry (TF 'SAME', window == stride as build_model uses it): out = ceil(in / s), pad = max((out - 1) s + w - in, 0),
lo = pad // 2 (the odd cell goes to the end); the window of output o starts at o w - lo.  Tensors are [N, D, H, W, C]
(2-D: D = 1 and a window of [1, wy, wx]).
"""
import numpy as np

# The geometries of the case table: name -> (input size (H, W) or (D, H, W), window), and what each reaches
GEOMETRIES = {
    '8x8_w2': ((8, 8), [2, 2]),                  # canonical
    '7x5_w2': ((7, 5), [2, 2]),                  # overhanging last window
    '4x4_w3': ((4, 4), [3, 3]),                  # lo = 1
    '5x5_w3': ((5, 5), [3, 3]),                  # lo = 0, overhang
    '5x5_w4': ((5, 5), [4, 4]),                  # lo = 1, hi = 2
    '2x2_w3': ((2, 2), [3, 3]),                  # window larger than the tensor
    '1x1_w2': ((1, 1), [2, 2]),                  # window larger than the tensor
    '6x6x6_w222': ((6, 6, 6), [2, 2, 2]),        # canonical
    '5x7x3_w222': ((5, 7, 3), [2, 2, 2]),        # overhang on every axis
    '4x6x6_w122': ((4, 6, 6), [1, 2, 2]),        # anisotropic
    '7x7x7_w333': ((7, 7, 7), [3, 3, 3]),        # lo = 1
    '7x7x7_w666': ((7, 7, 7), [6, 6, 6]),        # 216 offsets: arg-max bytes above 127
}


def same_pads(in_size, w):
    """(out, lo, hi) of one axis, window == stride == w."""
    out = -(-in_size // w)
    pad = max((out - 1) * w + w - in_size, 0)
    lo = pad // 2
    return out, lo, pad - lo


def geometry(in_dhw, w):
    """(out_dhw, lo[3], hi[3])."""
    g = [same_pads(int(n), int(k)) for n, k in zip(in_dhw, w)]
    return tuple(a[0] for a in g), tuple(a[1] for a in g), tuple(a[2] for a in g)


def win3(w):
    """A window of 2 or 3 entries as [wz, wy, wx]."""
    w = [int(v) for v in w]
    return [1] * (3 - len(w)) + w


def pool_fwd(x, w):
    """x [N, D, H, W, C], w [3] -> (out [N, OD, OH, OW, C] of x's dtype, argmax uint8 of the same shape).  Cells outside the
    tensor never win; the first maximum in (dz, dy, dx) order wins (a later cell must be strictly greater); the byte is
    (dz wy + dy) wx + dx of the FULL window, also where part of it hangs over an edge.  A window with no finite cell above
    -inf keeps -inf and byte 0, like the kernels (cannot happen under SAME with finite inputs)."""
    x = np.asarray(x)
    N, D, H, W, C = x.shape
    wz, wy, wx = [int(v) for v in w]
    assert wz * wy * wx <= 256
    (OD, OH, OW), (lz, ly, lx), _ = geometry((D, H, W), w)
    out = np.full((N, OD, OH, OW, C), -np.inf, dtype=x.dtype)
    arg = np.zeros((N, OD, OH, OW, C), dtype=np.uint8)

    def span(d, k, lo, n_in, n_out):
        """The outputs o whose cell o k - lo + d lies inside [0, n_in): (slice of outputs, strided slice of inputs) or None."""
        o0 = max(0, -(-(lo - d) // k))
        o1 = min(n_out, (n_in - 1 + lo - d) // k + 1)
        if o1 <= o0:
            return None
        i0 = o0 * k - lo + d
        return slice(o0, o1), slice(i0, i0 + (o1 - o0 - 1) * k + 1, k)

    for dz in range(wz):
        sz = span(dz, wz, lz, D, OD)
        for dy in range(wy):
            sy = span(dy, wy, ly, H, OH)
            for dx in range(wx):
                sx = span(dx, wx, lx, W, OW)
                if sz is None or sy is None or sx is None:
                    continue
                v = x[:, sz[1], sy[1], sx[1]]
                cur = out[:, sz[0], sy[0], sx[0]]          # views: written in place
                bytes_ = arg[:, sz[0], sy[0], sx[0]]
                take = v > cur
                cur[take] = v[take]
                bytes_[take] = (dz * wy + dy) * wx + dx
    return out, arg


def pool_bwd(dout, argmax, in_shape, w, act=None, old=None):
    """dout, argmax [N, OD, OH, OW, C]; in_shape (D, H, W) -> din [N, D, H, W, C]: an input voxel receives the cotangent of
    its window iff its offset in the window equals the stored byte, else 0 (a voxel in no window: 0).
    old: the tensor already holds a skip consumer's part: old + g, one fp32 add (the kernels' accumulate = 1).
    act: the producer's activation, a ReLU mask on the finished cotangent: kept where act > 0, else +0."""
    dout = np.asarray(dout)
    N, OD, OH, OW, C = dout.shape
    D, H, W = [int(v) for v in in_shape]
    wz, wy, wx = [int(v) for v in w]
    og, lo, _ = geometry((D, H, W), w)
    assert og == (OD, OH, OW), (og, dout.shape)
    lz, ly, lx = lo
    iz, iy, ix = np.arange(D), np.arange(H), np.arange(W)
    oz, oy, ox = (iz + lz) // wz, (iy + ly) // wy, (ix + lx) // wx
    rz, ry, rx = (iz + lz) - oz * wz, (iy + ly) - oy * wy, (ix + lx) - ox * wx
    inside = (oz < OD)[:, None, None] & (oy < OH)[None, :, None] & (ox < OW)[None, None, :]
    cz, cy, cx = np.minimum(oz, OD - 1), np.minimum(oy, OH - 1), np.minimum(ox, OW - 1)
    widx = ((rz[:, None, None] * wy + ry[None, :, None]) * wx + rx[None, None, :])
    sel = np.ix_(np.arange(N), cz, cy, cx, np.arange(C))
    hit = (argmax[sel].astype(np.int64) == widx[None, :, :, :, None]) & inside[None, :, :, :, None]
    g = np.where(hit, dout[sel], dout.dtype.type(0))
    if old is not None:
        g = (np.asarray(old, dtype=dout.dtype) + g).astype(dout.dtype)
    if act is not None:
        g = np.where(np.asarray(act) > 0, g, dout.dtype.type(0))
    return g


def chan_sums64(t):
    """fp64 channel sums [N, D, H, W] of the exact terms, and the sums of their magnitudes (for the bound below)."""
    t64 = np.asarray(t, dtype=np.float64)
    return t64.sum(-1), np.abs(t64).sum(-1)


def sum_bound(abs_sum, C):
    """|fp32 sum of C terms in any order - exact sum| <= (C - 1) 2^-24 sum |terms| (to first order; every partial sum is at
    most sum |terms| and each of the C - 1 adds rounds once, relative error 2^-24)."""
    return (C - 1) * 2.0 ** -24 * np.asarray(abs_sum, dtype=np.float64)
