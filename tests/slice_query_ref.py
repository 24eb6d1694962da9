"""Shared by tests/test_slice_query_host.py and tests/test_gpu_slice_query.py: the inputs of the slice-query kernels, the bound of
the sums and the device calls on raw arrays (the reference of every check is nnal_amd.slice_query.slice_scores_host)."""
import ctypes as C

import numpy as np

KINDS = ('entropy', 'MC-entropy', 'BALD', 'AU')


def bound(m, abs_sums):
    """|device - host| <= (m + 8) 2^-52 abs_sums for a slice of m terms: the a-priori bound of an m-term fp64 sum in any order,
    (m - 1) 2^-53 sum |t| on either side, plus a few units in the last place per term for log, the product and / T on either side.
    HIP documents a maximum error of 1 ulp for the double-precision log, as glibc does: no wider per-term constant is needed."""
    return (np.asarray(m, dtype=np.float64) + 8) * 2. ** -52 * np.asarray(abs_sums, dtype=np.float64)


def terms(kind, n, c, T):
    """Terms of a slice of n ROI voxels."""
    return {'entropy': n * c, 'MC-entropy': n * c, 'BALD': n * (c * T + c), 'AU': n}[kind]


def softmax_posteriors(rs, T, c, n, V, scale):
    """float32 [T, c, n, V]: softmax over c of randn * scale, evaluated in fp32 as a network would (scale 30: saturated, classes
    underflow to 0)."""
    z = (rs.randn(T, c, n, V) * scale).astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def one_hot(rs, T, c, n, V):
    lab = rs.randint(0, c, size=(T, 1, n, V))
    return (lab == np.arange(c).reshape(1, c, 1, 1)).astype(np.float32)


def mixed_posteriors(rs, T, c, n, V):
    """Near-uniform, ordinary and saturated voxels side by side, a few set to exact 0 / 1 rows."""
    P = np.concatenate([softmax_posteriors(rs, T, c, n, V, s)[..., None] for s in (0.1, 3., 30.)], axis=-1)
    pick = rs.randint(0, 3, size=(1, 1, n, V))
    P = np.take_along_axis(P, np.broadcast_to(pick, (T, c, n, V))[..., None], axis=-1)[..., 0]
    hot = one_hot(rs, T, c, n, V)
    exact = rs.rand(1, 1, n, V) < 0.05
    return np.where(exact, hot, P).astype(np.float32)


def roi_cases(rs, n, V):
    """{name: uint8 [n, V] or None}: no ROI, 30 % at random, one slice all zero, one slice with a single voxel."""
    rand = (rs.rand(n, V) < 0.3).astype(np.uint8) * rs.randint(1, 256, size=(n, V)).astype(np.uint8)
    empty = np.ones((n, V), dtype=np.uint8)
    empty[n // 2] = 0
    single = rand.copy()
    single[n - 1] = 0
    single[n - 1, V // 2] = 7
    return {'none': None, 'random': rand, 'empty slice': empty, 'single voxel': single}


# ---------------------------------------------------------------------------------------------------- device calls on raw arrays
GUARD = 16          # elements in front of and behind every output


class Guarded(object):
    """A device tensor of `n` elements with GUARD elements of a known fill on either side."""

    def __init__(self, sess, n, dtype, fill):
        self.full = sess.torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=sess.device)
        self.t = self.full[GUARD:GUARD + n]
        self.fill = fill

    def margins_intact(self):
        m = self.full.cpu().numpy()
        m = np.concatenate([m[:GUARD], m[-GUARD:]])
        return bool(np.all(np.isnan(m))) if isinstance(self.fill, float) and np.isnan(self.fill) else bool(np.all(m == self.fill))


def geometry(lib, c, n, V):
    out = (C.c_int64 * 4)()
    assert lib.alq_slice_scores_geometry(c, n, V, out) == 0
    return dict(threads=out[0], sweep=out[1], cap=out[2], partials=out[3])


def device_scores(sess, kind, P=None, roi=None, au=None, T=None):
    """The two kernels on the arrays of slice_scores_host: (sums, counts) as NumPy, plus the guarded outputs (for the margin
    checks).  The sums start as NaN: `first` must leave none."""
    torch = sess.torch
    if kind == 'AU':
        n, V = au.shape
        c = 2
    else:
        if P.ndim == 3:
            P = P[None]
        c, n, V = P.shape[1:]
    R = n * V
    scores, counts = Guarded(sess, n, torch.float64, float('nan')), Guarded(sess, n, torch.int64, -77)
    d_roi = None if roi is None else sess.to_device(np.ascontiguousarray(roi, dtype=np.uint8).reshape(-1), torch.uint8)
    guards = [scores, counts]
    from nnal_amd.slice_query import KINDS as K
    if kind == 'AU':
        sess.slice_scores(K[kind], n, V, c, f32=sess.to_device(np.ascontiguousarray(au, np.float32).reshape(-1), torch.float32), roi=d_roi,
                          scores=scores.t, counts=counts.t)
    elif kind == 'entropy':
        sess.slice_scores(K[kind], n, V, c, f32=sess.to_device(np.ascontiguousarray(P[0]).reshape(c, R), torch.float32), roi=d_roi,
                          scores=scores.t, counts=counts.t)
    else:
        T = P.shape[0] if T is None else T
        sum_p = Guarded(sess, c * R, torch.float64, float('nan'))
        sum_h = Guarded(sess, R, torch.float64, float('nan')) if kind == 'BALD' else None
        guards += [sum_p] + ([sum_h] if sum_h is not None else [])
        for k in range(T):
            post = sess.to_device(np.ascontiguousarray(P[k]).reshape(c, R), torch.float32)
            sess.unc_accumulate(post, sum_p.t.view(c, R), None if sum_h is None else sum_h.t, first=k == 0)
        sess.slice_scores(K[kind], n, V, c, T=T, sum_p=sum_p.t.view(c, R), sum_h=None if sum_h is None else sum_h.t, roi=d_roi,
                          scores=scores.t, counts=counts.t)
    return scores.t.cpu().numpy(), counts.t.cpu().numpy(), guards
