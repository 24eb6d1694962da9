"""Case tables and helpers of tests/test_tiled_host.py and tests/test_gpu_tiled.py (whole-volume inference by tiles:
nnal_amd/tiled.py is the statement, csrc/tile.hip the device)."""
import ctypes as C

import numpy as np

GUARD = 64          # elements either side of a guarded device buffer: 256 bytes of floats, so the payload keeps the 16-byte alignment


# Per-axis lattices (D, t, s) by what they exercise.
def axis_lattices(t):
    return {'overhang': (max(t - 2, 1), t, max(t // 2, 1)), 'one tile': (t, t, max(t // 2, 1)), 'two tiles': (t + 1, t, max(t // 2, 1)),
            'no overlap': (2 * t, t, t)}


CLAMPED = (11, 8, 4)          # origins 0 and 3: the last tile is clamped

# Blend / finalize cases: dims, tile, stride (Z, H, W each), classes, window, posterior table.
#   A  Z overhangs (3 < 4), H two tiles without overlap (12 = 2 x 6), W two tiles overlapping in t - 1 (6 = 5 + 1)
#   B  Z clamped last tile (11, 8, 4), H one tile (8 = 8), W two tiles overlapping in 7 (9 = 8 + 1)
#   C  Z no overlap (8 = 2 x 4), H and W general overlaps with a clamped last tile; N % 4 == 0 (the 16-byte finalize)
#   D  the clamped lattice on every axis, the largest tile
#   E  tile (2, 3, 2) at stride 1: 880 tiles, up to 12 tiles cover a voxel
#   F  a mixed tile, every axis with a clamped last tile
#   G  one tile that overhangs on every axis
#   H  one tile that fits exactly
BLEND_CASES = {
    'A': ((3, 12, 6), (4, 6, 5), (2, 6, 2), 2, 'gaussian', 'random'),
    'B': ((11, 8, 9), (8, 8, 8), (4, 4, 4), 3, 'triangle', 'random'),
    'C': ((8, 13, 11), (4, 6, 5), (4, 3, 2), 8, 'uniform', 'ties'),
    'D': ((11, 11, 11), (8, 8, 8), (4, 4, 4), 2, 'gaussian', 'zero plane'),
    'E': ((9, 13, 11), (2, 3, 2), (1, 1, 1), 3, 'triangle', 'ties'),
    'F': ((9, 13, 11), (5, 8, 6), (2, 4, 3), 2, 'uniform', 'random'),
    'G': ((3, 4, 2), (4, 6, 5), (2, 3, 2), 3, 'gaussian', 'random'),
    'H': ((4, 6, 5), (4, 6, 5), (2, 3, 2), 8, 'triangle', 'zero plane'),
}
RANGES = (1, 3, 7, None)          # tiles per blend call (None: all in one)

# Gather cases: dims, tile, stride, m, fill, (first, n) or None for all tiles.
GATHER_CASES = {
    'scalar rows tw=5 m=1': ((9, 13, 11), (4, 6, 5), (2, 3, 2), 1, 0., None),
    'scalar rows tw=5 m=2': ((9, 13, 11), (4, 6, 5), (2, 3, 2), 2, 0., None),
    'vector rows tw=8 m=2': ((9, 13, 16), (4, 6, 8), (2, 3, 4), 2, 0., None),
    'vector rows tw=5 m=4': ((9, 13, 11), (4, 6, 5), (2, 3, 2), 4, 0., None),
    'misaligned starts tw=8 m=1 s=3': ((9, 13, 19), (4, 6, 8), (2, 3, 3), 1, 0., None),
    'fill on z and w, whole pieces': ((3, 13, 6), (4, 6, 8), (2, 3, 4), 4, -7.5, None),
    'fill on w inside a piece': ((9, 4, 6), (4, 6, 8), (2, 3, 4), 1, 3.25, None),
    'first > 0': ((9, 13, 16), (4, 6, 8), (2, 3, 4), 2, 0., (5, 9)),
    'n = 1': ((9, 13, 16), (4, 6, 8), (2, 3, 4), 2, 0., (7, 1)),
    'n = 1, scalar': ((9, 13, 11), (4, 6, 5), (2, 3, 2), 1, 0., (11, 1)),
}


def posterior_table(rs, kind, c, n, V):
    """float32 [c, n V].  'random': normalised positive rows; 'ties': dyadic values 1/8, 1/4, 1/2 - windows of small integers give
    exact sums, hence exact ties between classes; 'zero plane': random with class 1 all zero."""
    if kind == 'ties':
        return rs.choice(np.array([0.125, 0.25, 0.5], dtype=np.float32), size=(c, n * V))
    p = rs.rand(c, n * V).astype(np.float64) + 0.01
    if kind == 'zero plane':
        p[1] = 0.
    return (p / p.sum(axis=0, keepdims=True)).astype(np.float32)


def cuts(ntiles, per):
    per = ntiles if per is None else per
    return [(a, min(per, ntiles - a)) for a in range(0, ntiles, per)]


def lattice(dims, tile, stride):
    from nnal_amd import _lib
    return _lib.TileLattice((C.c_int32 * 3)(*dims), (C.c_int32 * 3)(*tile), (C.c_int32 * 3)(*stride))


class Guarded(object):
    """A device tensor of `shape` inside a flat buffer with GUARD pattern-filled elements on either side."""

    def __init__(self, sess, shape, dtype, fill, init=None):
        torch = sess.torch
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=sess.device)
        self.t = self.full[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(init).to(sess.device))
        self.fill = fill

    def margins_intact(self):
        m = self.full.cpu().numpy()
        m = np.concatenate([m[:GUARD], m[-GUARD:]])
        return bool(np.all(np.isnan(m))) if isinstance(self.fill, float) and np.isnan(self.fill) else bool(np.all(m == self.fill))

    def numpy(self):
        return self.t.cpu().numpy()
