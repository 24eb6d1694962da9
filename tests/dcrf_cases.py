"""Deterministic scenes for the dense-CRF tests (tests/test_dcrf_host.py, tests/test_gpu_dcrf.py) and their host references,
each computed once per process and handed out as read-only arrays.

scene(H, W, seed): an ellipse m, an image 2 m + 0.7 noise and class-1 posteriors sigmoid(3 (m - 0.5) + 1.5 noise) of which five
pixels are exactly 0 (the zero guard).  On the four HOST_SCENES (checked in test_dcrf_host.py): no pixel ends within 1e-2 of a
tie in fp64, the fp32 restatement gives the fp64 MAP, the CRF changes 16 - 20 % of the raw labels and cuts the error against m
from about 15 % to 2 - 6 %."""
import functools

import numpy as np

HOST_SCENES = ((40, 56, 3), (24, 40, 5), (64, 48, 7), (80, 48, 11))
# the device shapes [S, H, W] -> the scenes of their slices
GPU_SHAPES = {
    (1, 40, 56): ((40, 56, 3),),                                   # smaller than the appearance window in both axes
    (3, 83, 45): ((83, 45, 21), (83, 45, 22), (83, 45, 23)),       # taller than the window, ragged against the tile
    (2, 7, 5): ((7, 5, 31), (7, 5, 32)),                           # degenerate
    (1, 1, 33): ((1, 33, 41),),
}
# compat 5 and 10, sdims 2 and 3, schan 0.5 (niter 3 goes with them)
OTHER_PARAMS = dict(sdims_smooth=(2., 2.), sdims_app=(3., 3.), schan=0.5, compat_smooth=5., compat_app=10.)
OTHER_NITER = 3


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(H, W, seed):
    """(m bool, img float64, post float64) [H, W]; drawn in this order: image noise, posterior noise, the five zeros."""
    r = np.random.RandomState(seed)
    x, y = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    m = ((x - 0.45 * H) / (0.3 * H)) ** 2 + ((y - 0.55 * W) / (0.25 * W)) ** 2 < 1
    img = 2. * m + 0.7 * r.randn(H, W)
    post = 1. / (1. + np.exp(-(3. * (m - 0.5) + 1.5 * r.randn(H, W))))
    zeros = r.choice(H * W, min(5, H * W), replace=False)
    post.ravel()[zeros] = 0.
    return _frozen(m), _frozen(img), _frozen(post)


def _key(params):
    return tuple(sorted((params or {}).items()))


@functools.lru_cache(maxsize=None)
def _marginals(H, W, seed, dtype_name, window, niter, pkey):
    from nnal_amd import dcrf
    _, img, post = scene(H, W, seed)
    Q = dcrf.meanfield_host(post.copy(), img, np.dtype(dtype_name).type, window, niter, dict(pkey))
    return tuple(_frozen(q) for q in Q)


def marginals(H, W, seed, dtype=np.float64, window=None, niter=5, params=None):
    """meanfield_host of scene(H, W, seed): the tuple (Q_0, ..., Q_niter), each [2, H W] read-only."""
    return _marginals(H, W, seed, np.dtype(dtype).name, window, niter, _key(params))


def stacked(shape, what):
    """The `what` ('img' or 'post') planes of the scenes of GPU_SHAPES[shape] as one float32 [S, H, W] array (a fresh copy)."""
    k = {'img': 1, 'post': 2}[what]
    return np.stack([scene(*s)[k] for s in GPU_SHAPES[shape]]).astype(np.float32)


def q1_stack(shape, dtype, it, niter=5, params=None):
    """Q_1 after `it` iterations over the slices of a device shape: [S, H, W] in `dtype` (all pairs)."""
    S, H, W = shape
    return np.stack([marginals(*s, dtype=dtype, niter=niter, params=params)[it][1].reshape(H, W) for s in GPU_SHAPES[shape]])


def tolerance(shape, it, niter=5, params=None):
    """The issue's bound for the device's class-1 marginal after `it` iterations on a device shape:
    4 x max |Q_fp32 host - Q_fp64| + 1e-6 - the fp32 restatement's own deviation from fp64 on the same input (the factor covers
    another summation order and the hardware exp2) plus the cut-off allowance (the windows drop at most 1.5e-7, measured in
    fp64 on scene (80, 48, 11)).  -> (tol, the fp32 host's deviation)."""
    dev32 = float(np.abs(q1_stack(shape, np.float32, it, niter, params).astype(np.float64) - q1_stack(shape, np.float64, it, niter, params)).max())
    return 4. * dev32 + 1e-6, dev32
