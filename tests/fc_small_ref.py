"""The skinny fully connected layer (cout <= 8) and the two-class head stated in NumPy fp64, and the case tables of
tests/test_gpu_fc_small.py (no device needed: tests/test_fc_small_ref_host.py checks all of this on the CPU).

Orders.  An activation is channels-last, [N, *spatial, C]; flattened as it lies in memory it is act[n, fm].  The reference
flattens with tf.transpose (all axes reversed) and a reshape, so a weight row W[o, :] is indexed by ft, the flatten order of
oracle.tfops.flatten_tf.  mem_of_tf(shape)[ft] = fm is read off flatten_tf itself (an arange pushed through it), not restated.

    logits[n, o]  = b[o] + sum_ft act[n, mem_of_tf[ft]] W[o, ft]
    din[n, fm]    = sum_o delta[n, o] W[o, tf_of_mem[fm]]            (masked: times act[n, fm] > 0)
    dsum[n, v]    = sum_c din[n, v, c]                                 (per voxel, after the mask)
    dW[n, o, ft]  = delta[n, o] act[n, mem_of_tf[ft]],  db[n, o] = delta[n, o]
    byte j of a patch's sign bytes: bit k = act[n, 4 j + k] > 0, k = 0 .. 3
"""
from collections import OrderedDict, namedtuple

import numpy as np

FC_SLICE = 8192          # elements one workgroup of the forward kernel reduces (csrc/kernels.hip)
FC_BITS_PG = 8           # patches per group of fc_small_dsum_bits_kernel
EXACT_BOUND = 2.0 ** 24  # every partial sum below it: fp32 (and the fp64 block sums) hold it exactly, in any order


# ------------------------------------------------------------------------------------------ orders
def mem_of_tf(shape):
    """shape = (*spatial, C) of one patch -> int64 [F]: the memory index of the element the reference's flatten puts at ft."""
    import torch
    from oracle import tfops
    F = int(np.prod(shape))
    x = torch.arange(F, dtype=torch.int64).reshape((1,) + tuple(shape))
    return tfops.flatten_tf(x)[:, 0].numpy()


def w_mem(W, shape):
    """W [c, F] in the reference's order -> [c, F] in activation-memory order (what d_Wp holds)."""
    W = np.asarray(W)
    out = np.empty_like(W)
    out[:, mem_of_tf(shape)] = W
    return out


# ------------------------------------------------------------------------------------------ the statement
def logits64(act, W, b, shape, relu=False):
    """act [N, *shape] (or [N, F] in memory order), W [c, F] in the reference's order, b [c] or [c, 1] -> [N, c]."""
    a = np.asarray(act, np.float64).reshape(len(act), -1)
    z = a[:, mem_of_tf(shape)] @ np.asarray(W, np.float64).T + np.asarray(b, np.float64).reshape(1, -1)
    return np.maximum(z, 0.) if relu else z


def din64(delta, W, shape, act=None):
    """The input cotangent [N, F] in memory order; masked by act > 0 where act is given."""
    d = np.asarray(delta, np.float64) @ w_mem(np.asarray(W, np.float64), shape)
    return d if act is None else d * (np.asarray(act).reshape(len(d), -1) > 0)


def chansum64(din, C):
    """Per-voxel channel sums [N, vox] of a cotangent [N, F] in memory order."""
    return np.asarray(din, np.float64).reshape(len(din), -1, C).sum(-1)


def wgrad64(act, delta, shape):
    """Per-sample dW [N, c, F] in the reference's order and db [N, c, 1]."""
    a = np.asarray(act, np.float64).reshape(len(act), -1)[:, mem_of_tf(shape)]
    d = np.asarray(delta, np.float64)
    return d[:, :, None] * a[:, None, :], d[:, :, None].copy()


def sign_bytes(act):
    """uint8 [N, F / 4]: bit k of byte j = act[n, 4 j + k] > 0."""
    s = (np.asarray(act).reshape(len(act), -1, 4) > 0).astype(np.uint8)
    return s[..., 0] | (s[..., 1] << 1) | (s[..., 2] << 2) | (s[..., 3] << 3)


def bits_dsum64(act, wv_mem, C=8):
    """What fc_small_dsum_bits_kernel writes: dsum[n, v] = sum_c [act[n, v, c] > 0] wv[v, c], wv = W0 - W1 in memory order."""
    a = np.asarray(act).reshape(len(act), -1, C) > 0
    return (a * np.asarray(wv_mem, np.float64).reshape(1, -1, C)).sum(-1)


def softmax64(z):
    """[N, c] -> posteriors [N, c] in fp64 (shifted by the row maximum) and the first maximum of every row."""
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p, np.argmax(z, axis=1)


# ------------------------------------------------------------------------------------------ torch fp32 twins (the e_32 of the bars)
def logits_torch(act, W, b, shape, dtype):
    import torch
    a = torch.tensor(np.asarray(act).reshape(len(act), -1)[:, mem_of_tf(shape)], dtype=dtype)
    return (a @ torch.tensor(np.asarray(W), dtype=dtype).t() + torch.tensor(np.asarray(b).reshape(1, -1), dtype=dtype)).numpy()


def din_torch(delta, W, shape, act, dtype):
    import torch
    d = (torch.tensor(np.asarray(delta), dtype=dtype) @ torch.tensor(w_mem(np.asarray(W), shape), dtype=dtype)).numpy()
    return d if act is None else d * (np.asarray(act).reshape(len(d), -1) > 0).astype(d.dtype)


def chansum_torch(din, C, dtype):
    import torch
    return torch.tensor(np.asarray(din), dtype=dtype).reshape(len(din), -1, C).sum(-1).numpy()


def wgrad_torch(act, delta, shape, dtype):
    import torch
    a = torch.tensor(np.asarray(act).reshape(len(act), -1)[:, mem_of_tf(shape)], dtype=dtype)
    d = torch.tensor(np.asarray(delta), dtype=dtype)
    return (d[:, :, None] * a[:, None, :]).numpy(), d[:, :, None].numpy().copy()


# ------------------------------------------------------------------------------------------ integer inputs
def _hash(n, seed):
    """n well-mixed 32-bit words (a fixed integer hash of the index: no two rows or columns of a table drawn from it agree)."""
    v = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    for _ in range(2):
        v = ((v ^ (v >> np.uint64(15))) * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
        v = ((v ^ (v >> np.uint64(12))) * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    return (v ^ (v >> np.uint64(15))).astype(np.int64)


def exact_fc_inputs(n, shape, c, seed, xmax=4, wmax=8):
    """x [n, *shape] integers in [-xmax, xmax] (patch 0 all zero, patch 1 non-zero in its first and last element only),
    W [c, F] integers in [-wmax, wmax] that differ from row to row and from column to column, b [c] multiples of 0.5."""
    F = int(np.prod(shape))
    x = (_hash(n * F, seed) % (2 * xmax + 1) - xmax).astype(np.float32).reshape((n,) + tuple(shape))
    x[0] = 0
    if n > 1:
        x[1] = 0
        x[1].reshape(-1)[[0, -1]] = (xmax, -xmax + 1) if F > 1 else (xmax,)
    W = (_hash(c * F, seed + 1) % (2 * wmax + 1) - wmax).astype(np.float32).reshape(c, F)
    b = ((_hash(c, seed + 2) % 9 - 4) * 0.5).astype(np.float32)
    return x, W, b


def assert_exact(act, W, b, shape=None):
    """The condition under which bit equality is owed: sum_f |act W| + |b| < 2^24 bounds every partial sum any summation
    order could form; all terms are multiples of 0.5.  act in memory order with W in memory order (shape None), or W in the
    reference's order with `shape`."""
    a = np.abs(np.asarray(act, np.float64).reshape(len(act), -1))
    Wm = np.abs(np.asarray(W, np.float64) if shape is None else w_mem(np.asarray(W, np.float64), shape))
    bound = (a @ Wm.T + np.abs(np.asarray(b, np.float64).reshape(1, -1))).max()
    assert bound < EXACT_BOUND, bound
    for t in (act, W, b):
        assert np.all(np.asarray(t, np.float64) * 2 == np.round(np.asarray(t, np.float64) * 2))
    if not all(np.all(np.asarray(t) == np.round(t)) for t in (act, W, b)):      # halves take one more bit
        assert bound < EXACT_BOUND / 2, bound
    return bound


# ------------------------------------------------------------------------------------------ case tables
# first-layer models fc(F -> c) on in_shape: F over both load paths (F % 4), one slice, exactly one slice, a one-element and a
# four-element last slice, three slices and a fourth of one element; c spread over 1 .. 8 (c = 1 is refused at model creation)
First = namedtuple('First', 'tag in_shape c')
FIRST = [First('F%d-c%d' % (F, c), (1, 1, F), c) for F, c in
         ((1, 2), (3, 3), (4, 8), (1023, 5), (1024, 2), (8188, 7), (8192, 4), (8193, 6), (8196, 2), (16388, 3), (24577, 8), (1024, 1))]
FIRST += [First('3x4x5x2-c3', (3, 4, 5, 2), 3), First('5x7x3-c2', (5, 7, 3), 2), First('5x7x3-c5', (5, 7, 3), 5)]      # the flatten order
WIDE = First('F1024-c9', (1, 1, 1024), 9)       # the boundary: the general engines, no fc_small launch
HIDDEN_F = 1024                                 # fc(F -> 8 | 1, 'MA') -> fc(2)
BATCHES = (1, 3, 5)                             # under max_batch = 4: one ragged pass, two passes with a ragged last


def slices(F):
    return -(-F // FC_SLICE)


def first_model(c):
    return OrderedDict([('fc', ['fc', [c[2]]])])


def hidden_model(h=8):
    return OrderedDict([('hid', ['fc', [h], 'MA']), ('fc', ['fc', [2]])])


def hidden_inputs(n, seed):
    """Integer inputs of the skinny hidden chain: the hidden layer's outputs stay small enough for the head to be exact."""
    x, W, b = exact_fc_inputs(n, (1, 1, HIDDEN_F), 8, seed, xmax=2, wmax=4)
    W2 = (_hash(16, seed + 3) % 9 - 4).astype(np.float32).reshape(2, 8)
    b2 = np.array([0.5, -1.5], np.float32)
    return x, W, b, W2, b2


# below-conv models conv(8, 3^nd, 'MA') -> conv(C, 3^nd, ops) [-> pool(2)] -> fc(c) on ragged volumes, float inputs
Below = namedtuple('Below', 'tag size C ops pool c form')
BELOW = [
    Below('C4-c2', (3, 5, 6), 4, 'MA', False, 2, 'G1'),
    Below('C8-c3', (3, 5, 6), 8, 'MA', False, 3, 'G2'),
    Below('C8-c2-2d', (5, 6), 8, 'MA', False, 2, 'G2'),
    Below('C16-c5', (2, 3, 5), 16, 'MA', False, 5, 'G4'),
    Below('C16-c2', (2, 3, 5), 16, 'MA', False, 2, 'G4'),
    Below('C32-c8', (3, 2, 3), 32, 'MA', False, 8, 'G8'),
    Below('C32-c2', (3, 2, 3), 32, 'MA', False, 2, 'G8'),
    Below('C12-c2', (3, 5, 6), 12, 'MA', False, 2, 'G0'),
    Below('C20-c5', (2, 3, 5), 20, 'MA', False, 5, 'G0'),
    Below('C6-c2-5x5x6', (5, 5, 6), 6, 'MA', False, 2, 'G0'),           # F = 900: the 16-byte path, C % 4 != 0
    Below('C6-c2-scalar', (5, 5, 3), 6, 'MA', False, 2, 'scalar'),      # F = 450: F % 4 == 2
    Below('C6-c3-scalar-2d', (5, 5), 6, 'MA', False, 3, 'scalar'),      # F = 150
    Below('C8-c2-M', (3, 5, 6), 8, 'M', False, 2, 'G2'),
    Below('C8-c2-pool', (4, 5, 6), 8, 'MA', True, 2, 'G0'),
]


def below_F(c):
    sp = tuple(-(-v // 2) for v in c.size) if c.pool else tuple(c.size)
    return int(np.prod(sp)) * c.C, sp


def below_model(c):
    nd = len(c.size)
    ld = OrderedDict([('low', ['conv', [8, [3] * nd], 'MA']), ('cv', ['conv', [c.C, [3] * nd], c.ops])])
    if c.pool:
        ld['pool'] = ['pool', [2] * nd]
    ld['fc'] = ['fc', [c.c]]
    return ld


# the two-class bits head conv(8, 3^nd, 'MA') -> conv(8, 3^nd, 'MA') -> fc(2), F % 1024 == 0
BITS_GEOMS = OrderedDict([('4x4x8', (4, 4, 8)), ('8x16', (8, 16)), ('8x12x12', (8, 12, 12)), ('16x16x16', (16, 16, 16))])
BITS_N = (1, 7, 8, 9)
# heads that must NOT take the bits: (tag, size, channels of the head conv, classes, head conv is the first parameter layer)
NO_BITS = [('F1000', (5, 5, 5), 8, 2, False), ('C16', (4, 4, 8), 16, 2, False), ('c3', (4, 4, 8), 8, 3, False), ('first', (4, 4, 8), 8, 2, True)]


def bits_model(nd, C=8, c=2, first=False):
    ld = OrderedDict() if first else OrderedDict([('low', ['conv', [8, [3] * nd], 'MA'])])
    ld['cv'] = ['conv', [C, [3] * nd], 'MA']
    ld['fc'] = ['fc', [c]]
    return ld


def bits_exact_inputs(n, size, seed, negative=False):
    """Integer inputs and weights of a bits-head model: x in {0, 1} (patch 0 all zero, patch 1 all one), conv weights in
    {-1, 0, 1} and zero conv biases - patch 0 is exactly zero behind both convs (the all-zero pattern), the others are mixed;
    `negative`: the head conv's weights and bias all -1, so that every pre-activation of every patch is negative (the
    all-negative pattern).  The head's W in [-2, 2].  Returns x [n, *size, 1] and the parameters in TF layouts."""
    nd = len(size)
    vox = int(np.prod(size))
    x = (_hash(n * vox, seed) % 2).astype(np.float32).reshape((n,) + tuple(size) + (1,))
    x[0] = 0
    if n > 1:
        x[1] = 1
    k = (3,) * nd
    W0 = (_hash(27 * 8, seed + 1)[:int(np.prod(k)) * 8] % 3 - 1).astype(np.float32).reshape(k + (1, 8))
    W1 = (_hash(27 * 64, seed + 2)[:int(np.prod(k)) * 64] % 3 - 1).astype(np.float32).reshape(k + (8, 8))
    b0 = np.zeros(8, np.float32)
    b1 = np.zeros(8, np.float32)
    if negative:
        W1, b1 = -np.ones_like(W1), -np.ones(8, np.float32)
    Wf = (_hash(2 * vox * 8, seed + 3) % 5 - 2).astype(np.float32).reshape(2, vox * 8)
    bf = np.array([[1.5], [-0.5]], np.float32)
    return x, OrderedDict([('low', [W0, b0]), ('cv', [W1, b1]), ('fc', [Wf, bf])])


def bits_exact_acts(x, pars):
    """fp64 activations of both convs of a bits-head model on integer inputs (exact: every value is a small integer)."""
    from oracle import tfops
    from tests import conv_ref
    nd = x.ndim - 2
    x5 = np.asarray(x, np.float64).reshape((len(x),) + (1,) * (3 - nd) + x.shape[1:])
    acts = []
    for nme in ('low', 'cv'):
        W, b = pars[nme]
        W5 = np.asarray(W, np.float64).reshape((1,) * (3 - nd) + W.shape)
        lo = [tfops.same_pads(s, kk, 1)[1] for s, kk in zip(x5.shape[1:4], W5.shape[:3])]
        x5 = np.maximum(conv_ref.forward64(x5, W5, b, lo), 0.)
        acts.append(x5.reshape((len(x),) + x.shape[1:-1] + (W.shape[-1],)))
    return acts
