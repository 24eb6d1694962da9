"""CPU references of the conv_transpose layer for tests/test_gpu_convt.py (and the table the host tests share with it).

`y[p] = sum_{q, t : s q + t - lo = p} x[q] W[t] + b` with `lo` the pad-before of the SAME strided conv the layer transposes
(oracle/tfops.py).  Everything here is channels-last and 3-D: a 2-D layer is the 3-D one with D = 1, k[0] = 1, s[0] = 1.
The fp64 functions are written from the definition, tap by tap, in numpy; the fp32 functions are the same operations through
torch (oracle/tfops.py, autograd) in float32: an independent fp32 implementation, the yardstick of the tolerances."""
from collections import OrderedDict

import numpy as np

from oracle import tfops

# tag -> input size (D, H, W), kernel and stride in the layer's own dimensionality (2 entries: the 2-D schema)
GEOMETRIES = OrderedDict([
    ('k2s2', dict(size=(3, 5, 4), k=[2, 2, 2], s=[2, 2, 2])),            # lo = 0, one tap per class: the common up-conv
    ('k3s2_ragged', dict(size=(3, 5, 6), k=[3, 3, 3], s=[2, 2, 2])),     # the canonical kernel on a non-cubic, odd volume
    ('k4s2', dict(size=(4, 3, 5), k=[4, 4, 4], s=[2, 2, 2])),            # lo = 1, two taps per class and dimension
    ('k3s3', dict(size=(2, 3, 4), k=[3, 3, 3], s=[3, 3, 3])),            # three classes per dimension, one tap each
    ('k5s2', dict(size=(3, 4, 4), k=[5, 5, 5], s=[2, 2, 2])),            # lo = 1, classes of 3 and 2 taps
    ('k3s1', dict(size=(3, 4, 5), k=[3, 3, 3], s=[1, 1, 1])),            # stride 1: one class, a flipped conv
    ('k234s2', dict(size=(3, 4, 5), k=[2, 3, 4], s=[2, 2, 2])),          # lo = 0 / 0 / 1, 1 / 1-2 / 2 taps per class
    ('2d_k3s2', dict(size=(1, 5, 7), k=[3, 3], s=[2, 2])),
    ('2d_k2s2', dict(size=(1, 5, 7), k=[2, 2], s=[2, 2])),
    ('2d_k4s2', dict(size=(1, 5, 7), k=[4, 4], s=[2, 2])),
    ('2d_k5s3', dict(size=(1, 4, 5), k=[5, 5], s=[3, 3])),
])


def three(v, fill=1):
    return [fill] * (3 - len(v)) + [int(a) for a in v]


def geometry(tag):
    """(input size (D, H, W), k and s as 3 entries, output size, lo per dimension, the layer's dimensionality)."""
    g = GEOMETRIES[tag]
    k3, s3 = three(g['k']), three(g['s'])
    out = tuple(n * s for n, s in zip(g['size'], s3))
    lo = [tfops.same_pads(o, k, s)[1] for o, k, s in zip(out, k3, s3)]
    return tuple(g['size']), k3, s3, out, lo, len(g['k'])


# ------------------------------------------------------------------------------------------ models (NN_extended schema)
def first_layer(Co, k, s, ops):
    """conv_transpose -> conv(4, 1x1) 'MA' -> fc(2): the conv_transpose reads the caller's x."""
    nd = len(k)
    return OrderedDict([('up', ['conv_transpose', [Co, list(k), list(s)], ops]), ('mix', ['conv', [4, [1] * nd], 'MA']),
                        ('fc', ['fc', [2]])]), ()


def below_conv(Ci, Co, k, s, ops, nd=None):
    """conv(Ci, 3^nd) 'MA' -> conv_transpose -> conv(4, 1x1) 'MA' -> fc(2) on a one-channel input."""
    nd = len(k) if nd is None else nd
    return OrderedDict([('low', ['conv', [Ci, [3] * nd], 'MA']), ('up', ['conv_transpose', [Co, list(k), list(s)], ops]),
                        ('mix', ['conv', [4, [1] * nd], 'MA']), ('fc', ['fc', [2]])]), ()


def unet_level(k, s):
    """One level of NET-C with another up-conv: enc and the conv_transpose are the two producers of dec's concat."""
    nd = len(k)
    k3 = [3] * nd
    return OrderedDict([('enc', ['conv', [8, k3], 'MA']), ('pool', ['pool', [2] * nd]), ('mid', ['conv', [16, k3], 'MA']),
                        ('up', ['conv_transpose', [8, list(k), list(s)], 'M']), ('dec', ['conv', [8, k3], 'MA']),
                        ('fc', ['fc', [2]])]), [[0, [4], 'con']]


# ------------------------------------------------------------------------------------------ fp64, from the definition
def _shifted(dy, k3, s3, lo, in_sp):
    """For every tap t (z outermost): dy[:, s q + t - lo, :] on the input grid q, zero outside the output volume."""
    dy = np.asarray(dy, np.float64)
    pad = [(0, 0)] + [(l, k + s) for l, k, s in zip(lo, k3, s3)] + [(0, 0)]
    dyp = np.pad(dy, pad)
    for tz in range(k3[0]):
        for ty in range(k3[1]):
            for tx in range(k3[2]):
                yield (tz, ty, tx), dyp[:, tz:tz + s3[0] * in_sp[0]:s3[0], ty:ty + s3[1] * in_sp[1]:s3[1], tx:tx + s3[2] * in_sp[2]:s3[2], :]


def bwd_data64(dy, W, s3, lo, in_sp, act=None):
    """din[n, q, ci] = sum_t sum_co dy[n, s q + t - lo, co] W[t, co, ci], times (act > 0) where the layer below has a ReLU.
    dy [N, *out, Co], W [kz, ky, kx, Co, Ci]."""
    W = np.asarray(W, np.float64)
    k3 = W.shape[:3]
    din = np.zeros((dy.shape[0],) + tuple(in_sp) + (W.shape[4],))
    for t, d in _shifted(dy, k3, s3, lo, in_sp):
        din += d @ W[t]
    return din if act is None else din * (np.asarray(act) > 0)


def wgrad64(a, dy, k3, s3, lo):
    """Per sample: dW[n, t, co, ci] = sum_q a[n, q, ci] dy[n, s q + t - lo, co] and db[n, co] = sum_p dy[n, p, co]."""
    a = np.asarray(a, np.float64)
    dW = np.zeros((a.shape[0],) + tuple(k3) + (dy.shape[-1], a.shape[-1]))
    for t, d in _shifted(dy, k3, s3, lo, a.shape[1:4]):
        dW[(slice(None),) + t] = np.einsum('nzyxo,nzyxi->noi', d, a)
    return dW, np.asarray(dy, np.float64).sum(axis=(1, 2, 3))


def forward_naive64(x, W, b, s3):
    """oracle.tfops.naive_conv_transpose_same: the loops of the definition."""
    return tfops.naive_conv_transpose_same(x, W, b, s3)


# ------------------------------------------------------------------------------------------ torch, either precision
def forward_torch(x, W, b, s3, dtype):
    import torch
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)  # noqa: E731
    return tfops.conv_transpose_same(t(x), t(W), t(b).reshape(-1), s3).numpy()


def bwd_data_torch(dy, W, s3, act, dtype):
    """The same sum as the SAME conv of stride s of dy with W read as [k.., in = Co, out = Ci] (what the layer transposes)."""
    import torch
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)  # noqa: E731
    din = tfops.conv_same(t(dy), t(W), torch.zeros(W.shape[-1], dtype=dtype), s3)
    if act is not None:
        din = din * (t(act) > 0).to(dtype)
    return din.numpy()


def wgrad_torch(a, dy, W, s3, dtype):
    """Per-sample dW, db by autograd through tfops.conv_transpose_same."""
    import torch
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)  # noqa: E731
    dWs, dbs = [], []
    for n in range(len(a)):
        Wt = t(W).clone().requires_grad_(True)
        bt = torch.zeros(W.shape[3], dtype=dtype, requires_grad=True)
        y = tfops.conv_transpose_same(t(a[n:n + 1]), Wt, bt, s3)
        gW, gb = torch.autograd.grad((y * t(dy[n:n + 1])).sum(), [Wt, bt])
        dWs.append(gW.numpy())
        dbs.append(gb.numpy())
    return np.stack(dWs), np.stack(dbs)


# ------------------------------------------------------------------------------------------ inputs
def exact_inputs(n, size, Ci, Co, k3, seed):
    """Small integers: x [n, *size, Ci] and W [*k, Co, Ci] in [-4, 4], b multiples of 0.5 in [-4, 4]; patch 0 all zero, patch 1
    non-zero in its eight corners only.  Every bf16 triple and fp16 pair holds such operands exactly and every partial sum
    of at most k^3 Ci <= 125 * 16 products of magnitude <= 16 is an integer (or half-integer) far below 2^24."""
    assert n >= 3
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, size=(n,) + tuple(size) + (Ci,)).astype(np.float32)
    x[0] = 0
    corners = np.zeros_like(x[1])
    for c in np.ndindex(2, 2, 2):
        idx = tuple(-1 if v else 0 for v in c)
        corners[idx] = rs.randint(1, 5, size=Ci) * rs.choice([-1, 1], size=Ci)
    x[1] = corners
    W = rs.randint(-4, 5, size=tuple(k3) + (Co, Ci)).astype(np.float32)
    b = (rs.randint(-8, 9, size=Co) * 0.5).astype(np.float32)
    return x, W, b


def first_stable_patches(om64, in_shape, seed, n, nscan, fragile_units):
    """The first n patches of the stream RandomState(seed).randn(nscan, *in_shape) whose fp64 evaluation has no fragile ReLU or
    max-pool decision (tests.test_gpu_hvp.fragile_units at ref64.DEFAULT_EPS); (patches, their positions in the stream)."""
    xs = np.random.RandomState(seed).randn(nscan, *in_shape).astype(np.float32)
    chosen = [i for i in range(nscan) if fragile_units(om64, xs[[i]]) == 0][:n]
    return xs[chosen], chosen
