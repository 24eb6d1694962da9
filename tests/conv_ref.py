"""CPU references of the plain stride-1 conv layer for tests/test_gpu_conv.py (and the table the host tests share with it).

`y[p] = sum_t x[p + t - lo] W[t] + b` with `lo` the pad-before of the SAME conv (oracle/tfops.same_pads: an even window pads
asymmetrically, lo = (k - 1) // 2 and the rest behind).  Everything here is channels-last and 3-D: a 2-D layer is the 3-D one with
D = 1, k[0] = 1.  The fp64 functions are written from the definition, tap by tap, in numpy; the fp32 functions are the same
operations through torch (oracle/tfops.py, autograd) in float32: an independent fp32 implementation, the yardstick of the
tolerances (tests/test_gpu_convt.py)."""
from collections import OrderedDict

import numpy as np

from oracle import tfops
from tests.convt_ref import three

# tag -> size (D, H, W), kernel in the layer's own dimensionality (2 entries: the 2-D schema), lo as 3 entries.  The smallest
# ragged volumes at which each branch of the plan code still exists.
GEOMETRIES = OrderedDict([
    ('k3_ragged', dict(size=(3, 5, 6), k=[3, 3, 3], lo=[1, 1, 1])),      # the canonical window off the cube; OW even: pair form at Co = 8
    ('k3_oddw', dict(size=(3, 4, 5), k=[3, 3, 3], lo=[1, 1, 1])),        # OW odd: no pair form at Co = 8
    ('k2', dict(size=(4, 3, 5), k=[2, 2, 2], lo=[0, 0, 0])),             # all padding behind; the flipped taps reach forward only
    ('k4_2d', dict(size=(1, 5, 7), k=[4, 4], lo=[0, 1, 1])),             # even, lo = 1 of 3, 16 taps
    ('k234', dict(size=(3, 4, 5), k=[2, 3, 4], lo=[0, 1, 1])),           # another k and lo per dimension, 24 taps
    ('k133', dict(size=(3, 5, 6), k=[1, 3, 3], lo=[0, 1, 1])),           # an in-plane window on a 3-D volume
    ('k311', dict(size=(4, 3, 5), k=[3, 1, 1], lo=[1, 0, 0])),           # a through-plane window only
    ('k1', dict(size=(3, 4, 5), k=[1, 1, 1], lo=[0, 0, 0])),             # one tap (CB = 32 at Ci = 32)
    ('k147', dict(size=(2, 5, 8), k=[1, 4, 7], lo=[0, 1, 3])),           # 28 taps = IG_MAXTAPS: legal for igemm, one over igemm2's 27
    ('k5_2d', dict(size=(1, 6, 7), k=[5, 5], lo=[0, 2, 2])),             # 25 taps in 2-D: the wide-2-D rule and ALQ_NO_WIDE2D_RULE
    ('k155_3d', dict(size=(2, 6, 7), k=[1, 5, 5], lo=[0, 2, 2])),        # the same 25 taps with ID = 2: the rule must not fire
    ('k15_2d', dict(size=(1, 4, 9), k=[1, 5], lo=[0, 0, 2])),            # a row window
    # igemm_build_plan's tile search at MD = 1, MH = 20, MW = 70: several patches per tile only when a tile covers a patch
    # (TY >= 32 and TX >= 128: more than 256 rows), so PT = 1; of the 256-row tiles, 8 x 32 (y, x) has the fewest - 3 x 3 = 9 tiles
    # (16 x 16: 2 x 5, 4 x 64: 5 x 2, 2 x 128: 10 x 1; 32 x 8 pays the factor 1.5 for TX < 16) - a middle tile along y and along x,
    # and ragged last tiles of 4 rows (16 .. 19) and 6 columns (64 .. 69)
    ('k3_tiles', dict(size=(1, 20, 70), k=[3, 3], lo=[0, 1, 1])),
])

MAX_TAPS = 28          # IG_MAXTAPS (csrc/alq_internal.h): the taps of one GEMM descriptor
MAXK_SMALL = 1024      # IG_MAXK_SMALL: the one K chunk of a layer whose Ci is no multiple of 8

# refused by alq_model_create: tag -> (size, k, s or None, Ci, the text behind "libalq error -4: ").  A conv's forward GEMM is one
# descriptor of all prod(k) taps, so - unlike a conv_transpose, whose forward classes hold ceil(k / s)^3 taps each - a window of
# more than 28 taps is refused as the first layer too.
REFUSED = OrderedDict([
    ('k4', dict(size=(4, 3, 5), k=[4, 4, 4], s=None, Ci=8, text='igemm: 64 taps unsupported')),
    ('k334', dict(size=(3, 4, 5), k=[3, 3, 4], s=None, Ci=8, text='igemm: 36 taps unsupported')),
    ('k6_2d', dict(size=(1, 6, 7), k=[6, 6], s=None, Ci=8, text='igemm: 36 taps unsupported')),
    ('k3_s2', dict(size=(3, 5, 6), k=[3, 3, 3], s=[2, 2, 2], Ci=8, text='layer %d: strided conv')),
    ('k3_s121', dict(size=(3, 5, 6), k=[3, 3, 3], s=[1, 2, 1], Ci=8, text='layer %d: strided conv')),
    ('k3_ci44', dict(size=(3, 4, 5), k=[3, 3, 3], s=None, Ci=44,
                     text='igemm: K = 27 taps x 44 channels exceeds the single-chunk limit 1024')),
])
# accepted at the single-chunk limit: K = 27 x 37 = 999 (KC = 1000) and 27 x 36 = 972, both <= 1024 with Ci % 8 != 0
SMALLC_LIMIT = [('k3_oddw', 37), ('k3_oddw', 36)]


def geometry(tag):
    """(size (D, H, W), k as 3 entries, lo per dimension from oracle.tfops.same_pads, the layer's dimensionality)."""
    g = GEOMETRIES[tag]
    k3 = three(g['k'])
    lo = [tfops.same_pads(n, k, 1)[1] for n, k in zip(g['size'], k3)]
    return tuple(g['size']), k3, lo, len(g['k'])


# ------------------------------------------------------------------------------------------ models (NN_extended schema)
def _conv(Co, k, ops, s=None):
    return ['conv', [Co, list(k)] + ([list(s)] if s is not None else []), ops]


def first_layer(Co, k, ops, s=None):
    """conv -> conv(4, 1x1) 'MA' -> fc(2): the conv under test ('cv') reads the caller's x."""
    nd = len(k)
    return OrderedDict([('cv', _conv(Co, k, ops, s)), ('mix', ['conv', [4, [1] * nd], 'MA']), ('fc', ['fc', [2]])]), ()


def below_conv(Ci, Co, k, ops, s=None):
    """conv(Ci, 3^nd) 'MA' -> conv under test ('cv') -> conv(4, 1x1) 'MA' -> fc(2) on a one-channel input."""
    nd = len(k)
    return OrderedDict([('low', ['conv', [Ci, [3] * nd], 'MA']), ('cv', _conv(Co, k, ops, s)),
                        ('mix', ['conv', [4, [1] * nd], 'MA']), ('fc', ['fc', [2]])]), ()


def skip_concat(k):
    """tests/test_gpu_parity.test_skip_concat_behind_a_relu_conv with the window k in place of 3x3x3 in the concat's consumer c3 and
    in c4: c3 reads [c1 | c2], two producers of 8 channels (the split concat; interleaved under ALQ_NO_SPLIT)."""
    k3 = [3, 3, 3]
    return OrderedDict([('c1', ['conv', [8, k3], 'MA']), ('c2', ['conv', [8, k3], 'MA']), ('c3', ['conv', [16, list(k)], 'MA']),
                        ('c4', ['conv', [8, list(k)], 'MA']), ('fc', ['fc', [2]])]), [[0, [2], 'con']]


def accumulating(k):
    """tests/test_gpu_parity.test_accumulating_conv_behind_a_skip_source with the window k in c2 - whose backward launch accumulates
    into the skip source's cotangent - c3 and the concat's consumer c4."""
    k3 = [3, 3, 3]
    return OrderedDict([('c1', ['conv', [8, k3], 'MA']), ('c2', ['conv', [16, list(k)], 'MA']), ('c3', ['conv', [8, list(k)], 'MA']),
                        ('c4', ['conv', [8, list(k)], 'MA']), ('fc', ['fc', [2]])]), [[0, [3], 'con']]


# ------------------------------------------------------------------------------------------ fp64, from the definition
def _w5(W):
    """A TF conv filter [k.., Ci, Co] of a 2-D or 3-D layer as [kz, ky, kx, Ci, Co]."""
    W = np.asarray(W)
    return W.reshape((1,) * (5 - W.ndim) + W.shape)


def _shifted(v, k3, off):
    """For every tap t (z outermost): v[:, p + off(t), :] on v's own grid p, zero outside the volume.  off[d] maps t[d] to the
    shift along d; shifts lie in [-(k - 1), k - 1]."""
    v = np.asarray(v, np.float64)
    sp = v.shape[1:4]
    vp = np.pad(v, [(0, 0)] + [(k - 1, k - 1) for k in k3] + [(0, 0)])
    for t in np.ndindex(*k3):
        o = [k3[d] - 1 + off[d](t[d]) for d in range(3)]
        yield t, vp[:, o[0]:o[0] + sp[0], o[1]:o[1] + sp[1], o[2]:o[2] + sp[2], :]


def forward_naive64(x, W, b):
    """oracle.tfops.naive_conv_same: the loops of the definition (x [N, D, H, W, Ci], W [kz, ky, kx, Ci, Co])."""
    return tfops.naive_conv_same(x, W, b)


def forward64(x, W, b, lo):
    """y[n, p, co] = sum_t sum_ci x[n, p + t - lo, ci] W[t, ci, co] + b[co], one shifted slab per tap."""
    W = np.asarray(W, np.float64)
    y = np.zeros(np.asarray(x).shape[:4] + (W.shape[4],))
    for t, xs in _shifted(x, W.shape[:3], [lambda a, l=l: a - l for l in lo]):
        y += xs @ W[t]
    return y + np.asarray(b, np.float64).reshape(-1)


def bwd_data64(dy, W, lo, act=None):
    """din[n, q, ci] = sum_t sum_co dy[n, q + lo - t, co] W[t, ci, co], times (act > 0) where the layer below has a ReLU.
    dy [N, D, H, W, Co], W [kz, ky, kx, Ci, Co]."""
    W = np.asarray(W, np.float64)
    din = np.zeros(np.asarray(dy).shape[:4] + (W.shape[3],))
    for t, d in _shifted(dy, W.shape[:3], [lambda a, l=l: l - a for l in lo]):
        din += d @ W[t].T
    return din if act is None else din * (np.asarray(act) > 0)


def wgrad64(a, dy, k3, lo):
    """Per sample: dW[n, t, ci, co] = sum_p a[n, p + t - lo, ci] dy[n, p, co] and db[n, co] = sum_p dy[n, p, co]."""
    dy = np.asarray(dy, np.float64)
    dW = np.zeros((len(dy),) + tuple(k3) + (np.asarray(a).shape[-1], dy.shape[-1]))
    for t, xs in _shifted(a, k3, [lambda v, l=l: v - l for l in lo]):
        dW[(slice(None),) + t] = np.einsum('nzyxi,nzyxo->nio', xs, dy)
    return dW, dy.sum(axis=(1, 2, 3))


# ------------------------------------------------------------------------------------------ torch, either precision
def _t(v, dtype):
    import torch
    return torch.as_tensor(np.asarray(v)).to(dtype)


def forward_torch(x, W, b, dtype):
    return tfops.conv_same(_t(x, dtype), _t(W, dtype), _t(b, dtype).reshape(-1)).numpy()


def bwd_data_torch(dy, W, act, dtype):
    """The cotangent of the input by autograd through tfops.conv_same, times (act > 0)."""
    import torch
    x = torch.zeros(tuple(np.asarray(dy).shape[:4]) + (W.shape[3],), dtype=dtype, requires_grad=True)
    y = tfops.conv_same(x, _t(W, dtype), torch.zeros(W.shape[4], dtype=dtype))
    din, = torch.autograd.grad((y * _t(dy, dtype)).sum(), [x])
    if act is not None:
        din = din * (_t(act, dtype) > 0).to(dtype)
    return din.numpy()


def wgrad_torch(a, dy, W, dtype):
    """Per-sample dW, db by autograd through tfops.conv_same."""
    import torch
    dWs, dbs = [], []
    for n in range(len(a)):
        Wt = _t(W, dtype).clone().requires_grad_(True)
        bt = torch.zeros(W.shape[4], dtype=dtype, requires_grad=True)
        y = tfops.conv_same(_t(a[n:n + 1], dtype), Wt, bt)
        gW, gb = torch.autograd.grad((y * _t(dy[n:n + 1], dtype)).sum(), [Wt, bt])
        dWs.append(gW.numpy())
        dbs.append(gb.numpy())
    return np.stack(dWs), np.stack(dbs)


# ------------------------------------------------------------------------------------------ inputs
def exact_inputs(n, size, Ci, Co, k3, seed):
    """tests.convt_ref.exact_inputs with the filter in a conv's layout: x [n, *size, Ci] and W [*k, Ci, Co] small integers,
    b multiples of 0.5; patch 0 all zero, patch 1 non-zero in its eight corners only."""
    from tests import convt_ref
    x, W, b = convt_ref.exact_inputs(n, size, Ci, Co, k3, seed)
    return x, np.ascontiguousarray(np.swapaxes(W, -1, -2)), b
