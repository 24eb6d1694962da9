"""NET-C's fused layer launches at 32^3, one fp64 statement per launch (no device needed: tests/test_netc_ref_host.py holds all of this
on the CPU, tests/test_gpu_netc_launches.py holds the launches to it).

LAUNCHES is the table of what the default Fisher pass of netspec.net_c() at (32, 32, 32, 1) runs, read from csrc/passes.hip: per
launch its name, source file, the alq_model_engine_info index and value that prove it ran, what it reads and what it leaves in
memory, both as (layer, what) pairs.  Layers: 0 enc1, 1 pool1, 2 enc2, 3 pool2, 4 bott, 5 up1, 6 dec1, 7 up2, 8 dec2, 9 fc.
`what`: 'out' the activation [n, D, H, W, C], 'sign' its sign field as bool (exactly act > 0), 'argmax' a pool's bytes, 'osum' the
channel sums of the output, 'amax' the per-patch maxima a launch was asked for, 'dout' the cotangent of the layer's output (masked
where the layer has a ReLU), 'dsum' its channel sums, 'headsign' the sign bytes the head keeps of dec2's output.

Every launch is  inputs -> a (one linear contraction with the layer's weights) -> y -> finish (bias, ReLU, masks, pools, sums):
Launch.core gives a (the weights are the layer's: `weights`), Launch.finish the stored outputs.  reference() runs that in fp64
(torch fp64 on oracle.tfops, tests.pool_ref and NumPy), bars() gives the derived bar of check B on y, emulate() the same contraction
on np.float16 pairs (f16_pair.h::f16_pair_split) or bf16 triples.  compose() chains the references from x: the integers check A expects.  bwd_bounds() is the host twin of
passes.hip::bwd_bounds with the per-slice norms of weight_layout.h::conv_bwd_l1_slices.

The bar of check B, per element of y (x the launch's input, w its weights, K terms per element):

    bar = sum |dx| |w| + sum |x| |dw| + sum |lo_x lo_w| + 2^-24 (M - 1) sum |x w| + 2^-24 |y|

  fp16 pair (f16_pair_split: x 2^e = h + l 2^-shift, both rounded to nearest): |dx| <= 2^-22 |x| + f_x, f_x = 2^(-25 - shift - e_x)
    the absolute resolution where the lo piece is an fp16 subnormal (Launch.shift: 11 in d3d.hip, t3d8b.hip and e3d.hip, whose
    bounds are loose by orders of magnitude; 0 elsewhere, and where a file has both forms); e_x = 14 - ex for a
    bound in [2^(ex - 1), 2^ex) (sweep_common.h::sw_patch_exp), per patch, of the bound the launch actually used; e_w =
    f16_pair_exp of the layer's weights.  |lo| <= 2^-11 |.| + 2^(-25 - e): the dropped product is 2^-22 |x w| + 2^-11 (f_x |w| + f_w |x|) + f_x f_w.
  bf16 triple: three pieces hold the 24 bits of an fp32 number, |dx| <= 2^-24 |x| (no floor in the range of the tests); the three
    dropped products (m l, l m, l l) are below 2^-24 |x w|.
  M, the fp32 additions into one accumulator: every kernel here contracts with the 16 x 16 x 32 MFMA, so a product passes through
    the sum of its own instruction (at most 32 terms, any order) and then through the chain of accumulator updates: at most
    pieces (ceil(K / 32) + 2) of them (pieces = 3 products of an fp16 pair, 6 of a bf16 triple; + 2: K slots padded per tap), + 2
    for the bias and the merge of a second accumulator: M = pieces (ceil(K / 32) + 2) + 32 + 2.
  2^-24 |y|: the one rounding of the stored fp32 result.
Masks, routing through an arg-max and slices only select: they apply to the bar as to the value.  Channel sums are held by
tests.test_gpu_pool._assert_sums against the launch's own stored tensor; where that tensor is not stored (dsum of enc2 and enc1 from
e3d.hip) the sum bound of tests.pool_ref is added to the routed bar of the terms (e3d_extra).
"""
from collections import OrderedDict, namedtuple

import numpy as np

from oracle import netspec, tfops
from tests import pool_ref, scale_ref
from tests.fc_small_ref import _hash, w_mem

ENC1, POOL1, ENC2, POOL2, BOTT, UP1, DEC1, UP2, DEC2, FC = range(10)
NAMES = ['enc1', 'pool1', 'enc2', 'pool2', 'bott', 'up1', 'dec1', 'up2', 'dec2', 'fc']
IN_SHAPE = (32, 32, 32, 1)
SIZE = {ENC1: 32, POOL1: 16, ENC2: 16, POOL2: 8, BOTT: 8, UP1: 16, DEC1: 16, UP2: 32, DEC2: 32}
CH = {ENC1: 8, POOL1: 8, ENC2: 16, POOL2: 16, BOTT: 32, UP1: 16, DEC1: 16, UP2: 8, DEC2: 8}
W2 = [2, 2, 2]
ENGINE_BOUND = 2.0 ** 22      # an fp16 pair under a bound below 2^22 holds every integer
ACC_BOUND = 2.0 ** 24
MUTATIONS = ('tap', 'chan', 'plane', 'tie', 'ge')


def net():
    ld, sk = netspec.net_c()
    assert list(ld) == NAMES
    return ld, sk


# ------------------------------------------------------------------------------------------ the linear maps, fp64
def _t(a, dtype=np.float64):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype))


def _vjp(fn, shape, d):
    import torch
    x = torch.zeros(shape, dtype=d.dtype, requires_grad=True)
    g, = torch.autograd.grad(fn(x), x, grad_outputs=d)
    return g.numpy()


def lin(kind, a, W, dtype=np.float64):
    """y of one contraction, no bias.  'conv': 3x3x3 SAME, W [3, 3, 3, Ci, Co]; 'convT': stride 2, W [3, 3, 3, Co, Ci]; 'conv_bwd' /
    'convT_bwd': a is the cotangent of that layer's output, y the cotangent of its input.  dtype = np.float32: the fp32 yardstick."""
    import torch
    at, Wt = _t(a, dtype), _t(W, dtype)
    zero = torch.zeros((), dtype=at.dtype)
    n, sp = len(at), tuple(at.shape[1:4])
    if kind == 'conv':
        return tfops.conv_same(at, Wt, zero).numpy()
    if kind == 'convT':
        return tfops.conv_transpose_same(at, Wt, zero, W2).numpy()
    if kind == 'conv_bwd':
        return _vjp(lambda x: tfops.conv_same(x, Wt, zero), (n,) + sp + (W.shape[3],), at)
    assert kind == 'convT_bwd', kind
    return _vjp(lambda x: tfops.conv_transpose_same(x, Wt, zero, W2), (n,) + tuple(v // 2 for v in sp) + (W.shape[4],), at)


# the tap a mutation leaves out on the face x = last (it reads one voxel inwards), and the axis of W the contraction runs over
_TAP = {'conv': (1, 1, 0), 'conv_bwd': (1, 1, 2), 'convT': (1, 1, 1), 'convT_bwd': (1, 1, 1)}
_KAXIS = {'conv': 3, 'conv_bwd': 4, 'convT': 4, 'convT_bwd': 3}


def lin_mut(kind, a, W, mut):
    """lin under a mutation of the contraction: 'plane' input plane z = 1 is plane 2; 'tap' one tap left out on the face x = last;
    'kchan' one contracted channel left out in the plane z = 0."""
    a, W = np.asarray(a, np.float64), np.asarray(W, np.float64)
    if mut == 'plane':
        a = a.copy()
        a[:, 1] = a[:, 2]
    y = lin(kind, a, W)
    if mut in ('tap', 'kchan'):
        Wm = W.copy()
        if mut == 'tap':
            Wm[_TAP[kind]] = 0
            y[:, :, :, -1] = lin(kind, a, Wm)[:, :, :, -1]
        else:
            Wm[(slice(None),) * _KAXIS[kind] + (0,)] = 0
            y[:, 0] = lin(kind, a, Wm)[:, 0]
    return y


def csum(t, mut=None):
    """Channel sums [n, D, H, W]; 'chan': the last channel is left out."""
    t = np.asarray(t, np.float64)
    return t[..., :-1].sum(-1) if mut == 'chan' else t.sum(-1)


def pool2(x, tie=False):
    """2x2x2 max pool; tie: the LAST maximum of a window wins (the mutation)."""
    if not tie:
        return pool_ref.pool_fwd(x, W2)
    x = np.asarray(x)
    out = np.full((len(x),) + tuple(v // 2 for v in x.shape[1:4]) + (x.shape[4],), -np.inf, x.dtype)
    arg = np.zeros(out.shape, np.uint8)
    for b, (dz, dy, dx) in enumerate(np.ndindex(2, 2, 2)):
        v = x[:, dz::2, dy::2, dx::2]
        take = v >= out
        out[take], arg[take] = v[take], b
    return out, arg


def positive(t, mut=None):
    return np.asarray(t) >= 0 if mut == 'ge' else np.asarray(t) > 0


def head_wv(P):
    """W0 - W1 of the head in activation-memory order [32, 32, 32, 8]: one fp32 subtraction (weights.hip::head_wv)."""
    Wm = w_mem(np.asarray(P['fc'][0], np.float32), (32, 32, 32, 8))
    return (Wm[0] - Wm[1]).astype(np.float64).reshape(32, 32, 32, 8)


# ------------------------------------------------------------------------------------------ the launches
Launch = namedtuple('Launch', 'name file info inputs outputs layer kind split scale core finish muts shift')


def _bias(P, layer):
    return np.asarray(P[NAMES[layer]][1], np.float64).reshape(-1)


def _relu_outputs(layer, y, P, mut, amax):
    out = np.maximum(y + _bias(P, layer), 0.)
    r = OrderedDict([((layer, 'out'), out), ((layer, 'sign'), positive(out, mut)), ((layer, 'osum'), csum(out, mut))])
    if amax:
        r[(layer, 'amax')] = np.abs(out).reshape(len(out), -1).max(1)
    return r


def _f3d_finish(y, T, P, mut):
    r = _relu_outputs(ENC2, y, P, mut, False)
    pooled, arg = pool2(r[(ENC2, 'out')], tie=mut == 'tie')
    r.update({(POOL2, 'out'): pooled, (POOL2, 'argmax'): arg, (POOL2, 'osum'): csum(pooled, mut)})
    return r


def _convt_finish(layer):
    def finish(y, T, P, mut):
        out = y + _bias(P, layer)
        return OrderedDict([((layer, 'out'), out), ((layer, 'osum'), csum(out, mut)), ((layer, 'amax'), np.abs(out).reshape(len(out), -1).max(1))])
    return finish


def _c3b_core(T, P):
    return T[(FC, 'headsign')] * head_wv(P)[None]


def _c3b_finish(y, T, P, mut):
    """channels 8 .. 15: up2's cotangent, stored and summed; channels 0 .. 7: masked by enc1's signs and only summed - enc1's PARTIAL
    dsum, which e3d.hip completes (key (ENC1, 'dsum_part'): not in memory after the pass)."""
    d7 = y[..., 8:]
    return OrderedDict([((UP2, 'dout'), d7), ((UP2, 'dsum'), csum(d7, mut)), ((ENC1, 'dsum_part'), csum(y[..., :8] * T[(ENC1, 'sign')], mut))])


def _masked_finish(layer, mask_layer):
    def finish(y, T, P, mut):
        d = y * T[(mask_layer, 'sign')]
        return OrderedDict([((layer, 'dout'), d), ((layer, 'dsum'), csum(d, mut))])
    return finish


def _d3b_finish(y, T, P, mut):
    d5 = y[..., 16:]
    return OrderedDict([((ENC2, 'dout'), y[..., :16]), ((UP1, 'dout'), d5), ((UP1, 'dsum'), csum(d5, mut))])


def e3d_delta2(T):
    """enc2's masked cotangent: pool2 backward through its arg-max, plus the skip half, under enc2's ReLU mask."""
    routed = pool_ref.pool_bwd(np.asarray(T[(POOL2, 'dout')], np.float64), T[(POOL2, 'argmax')], (16, 16, 16), W2)
    return (np.asarray(T[(ENC2, 'dout')], np.float64) + routed) * T[(ENC2, 'sign')]


def e3d_route(g, T):
    """conv backward result g [n, 16^3, 8] -> [n, 32^3, 8]: the enc1 mask (the sign of the pooled value IS enc1's sign at the arg-max)
    and pool1 backward."""
    return pool_ref.pool_bwd(np.asarray(g, np.float64) * T[(POOL1, 'sign')], T[(POOL1, 'argmax')], (32, 32, 32), W2)


def _e3d_finish(y, T, P, mut):
    part = reference(BY_NAME['c3d_bwd7'], T, P)[(ENC1, 'dsum_part')]      # the dec2 slice, recomputed from the head's sign bytes
    return OrderedDict([((ENC2, 'dsum'), csum(e3d_delta2(T), mut)), ((ENC1, 'dsum'), csum(e3d_route(y, T), mut) + part)])


def _cat(T, a, b):
    return np.concatenate([np.asarray(T[a], np.float64), np.asarray(T[b], np.float64)], -1)


FWD_MUTS, BWD_MUTS = ('tap', 'chan', 'plane', 'ge'), ('tap', 'chan', 'plane')
LAUNCHES = [
    Launch('f3d_fwd', 'f3d.hip', (12, 1), [(POOL1, 'out')],
           [(ENC2, 'out'), (ENC2, 'sign'), (ENC2, 'osum'), (POOL2, 'out'), (POOL2, 'argmax'), (POOL2, 'osum')],
           ENC2, 'conv', 'f16', 'measured', lambda T, P: T[(POOL1, 'out')], _f3d_finish, FWD_MUTS + ('tie',), 0),
    Launch('bott_fwd', 'igemm4.hip', (6, 1), [(POOL2, 'out')], [(BOTT, 'out'), (BOTT, 'sign'), (BOTT, 'osum')],
           BOTT, 'conv', 'bf16', None, lambda T, P: T[(POOL2, 'out')], lambda y, T, P, mut: _relu_outputs(BOTT, y, P, mut, False), FWD_MUTS, 0),
    Launch('t3d_fwd_up1', 't3d.hip', (7, 2), [(BOTT, 'out')], [(UP1, 'out'), (UP1, 'osum')],
           UP1, 'convT', 'bf16', None, lambda T, P: T[(BOTT, 'out')], _convt_finish(UP1), BWD_MUTS, 0),
    Launch('d3d_fwd', 'd3d.hip', (10, 1), [(ENC2, 'out'), (UP1, 'out')], [(DEC1, 'out'), (DEC1, 'sign'), (DEC1, 'osum')],
           DEC1, 'conv', 'f16', 'derived', lambda T, P: _cat(T, (ENC2, 'out'), (UP1, 'out')), lambda y, T, P, mut: _relu_outputs(DEC1, y, P, mut, False), FWD_MUTS, 11),
    Launch('t3d_fwd_up2', 't3d.hip', (7, 2), [(DEC1, 'out')], [(UP2, 'out'), (UP2, 'osum'), (UP2, 'amax')],
           UP2, 'convT', 'bf16', None, lambda T, P: T[(DEC1, 'out')], _convt_finish(UP2), BWD_MUTS, 0),
    Launch('c3d_bwd7', 'c3d.hip', (13, 7), [(FC, 'headsign'), (ENC1, 'sign')], [(UP2, 'dout'), (UP2, 'dsum')],
           DEC2, 'conv_bwd', 'f16', 'wv', _c3b_core, _c3b_finish, BWD_MUTS, 0),
    Launch('t3d_bwd_up2', 't3d.hip', (8, 2), [(UP2, 'dout'), (DEC1, 'sign')], [(DEC1, 'dout'), (DEC1, 'dsum')],
           UP2, 'convT_bwd', 'f16', 'static', lambda T, P: T[(UP2, 'dout')], _masked_finish(DEC1, DEC1), BWD_MUTS, 0),
    Launch('d3d_bwd', 'd3d.hip', (11, 1), [(DEC1, 'dout')], [(ENC2, 'dout'), (UP1, 'dout'), (UP1, 'dsum')],
           DEC1, 'conv_bwd', 'f16', 'static', lambda T, P: T[(DEC1, 'dout')], _d3b_finish, BWD_MUTS, 11),
    Launch('t3d8_bwd_up1', 't3d8b.hip', (8, 2), [(UP1, 'dout'), (BOTT, 'sign')], [(BOTT, 'dout'), (BOTT, 'dsum')],
           UP1, 'convT_bwd', 'f16', 'static', lambda T, P: T[(UP1, 'dout')], _masked_finish(BOTT, BOTT), BWD_MUTS, 11),
    Launch('bott_bwd', 'igemm4.hip', (9, 1), [(BOTT, 'dout')], [(POOL2, 'dout')],
           BOTT, 'conv_bwd', 'f16', 'static', lambda T, P: T[(BOTT, 'dout')], lambda y, T, P, mut: OrderedDict([((POOL2, 'dout'), y)]), ('tap', 'kchan', 'plane'), 0),
    Launch('e3d_bwd', 'e3d.hip', (17, 2), [(ENC2, 'dout'), (POOL2, 'dout'), (POOL2, 'argmax'), (ENC2, 'sign'), (POOL1, 'argmax'), (POOL1, 'sign'),
                                          (FC, 'headsign'), (ENC1, 'sign')], [(ENC2, 'dsum'), (ENC1, 'dsum')],
           ENC2, 'conv_bwd', 'f16', 'static', lambda T, P: e3d_delta2(T), _e3d_finish, BWD_MUTS, 11),
]
BY_NAME = OrderedDict((l.name, l) for l in LAUNCHES)
# the engine-info indices every GPU test asserts (value): the launches above and the forms of the c3d / e3d kernels
ENGINE_INFO = OrderedDict([(7, 2), (8, 2), (9, 1), (10, 1), (11, 1), (12, 1), (13, 7), (17, 2), (19, 2)])
# the constant-folded igemm4 launches of bott leave no index of their own: bott_fwd is proved by (6, 1) - the pass ran its fp16-pair
# launches on derived bounds, i.e. the default route - and by the sign field (what = 12) of layer 4, which only an igemm4 launch
# writes (passes.hip::fwd_conv_gemm: signs_ready only under ROUTE_IGEMM4); bott_bwd by (9, 1): e3d.hip reads what it wrote.


def weights(l, P):
    return np.asarray(P[NAMES[l.layer]][0], np.float64)


def reference(l, T, P, mut=None):
    """The launch's stored outputs in fp64 from its stored inputs."""
    kmut = mut if mut in ('tap', 'plane', 'kchan') else None
    return l.finish(lin_mut(l.kind, l.core(T, P), weights(l, P), kmut), T, P, mut)


# ------------------------------------------------------------------------------------------ scales, bounds
def frexp_exp(v):
    """ex with v in [2^(ex - 1), 2^ex); 0 for v = 0."""
    return np.frexp(np.asarray(v, np.float64))[1]


def pair_exp(bound):
    """sw_patch_exp: 14 - ex, at most 96, and 0 for a zero bound."""
    b = np.asarray(bound, np.float64)
    return np.where(b > 0, np.minimum(14 - frexp_exp(b), 96), 0)


def bwd_l1_parts(W, transposed, split):
    """(bwd_l1, part[0], part[1]) of weight_layout.h: max over the input channels of sum_{tap, co} |W|, over all of them and per slice."""
    a = np.abs(np.asarray(W, np.float64))
    per_ci = a.sum(axis=(0, 1, 2, 3)) if transposed else a.sum(axis=(0, 1, 2, 4))
    if not split:
        return float(per_ci.max()), 0., 0.
    return float(per_ci.max()), float(per_ci[:split].max()), float(per_ci[split:].max())


def bwd_bounds(P):
    """passes.hip::bwd_bounds for NET-C: the static bound on every layer's output cotangent under the unit cotangent, float32 sums."""
    ld, sk = net()
    src2 = scale_ref.skip_src_of(ld, sk)
    types = scale_ref.layer_types(ld)
    b = np.zeros(10, np.float32)
    b[FC] = 1.
    for i in range(9, 0, -1):
        bound = float(b[i])
        part = (0., 0.)
        if types[i] == 'fc':
            inb = float(np.abs(head_wv(P)).max().astype(np.float32))
        elif types[i] == 'pool':
            inb = bound
        else:
            l1, p0, p1 = bwd_l1_parts(P[NAMES[i]][0], types[i] == 'conv_transpose', CH[src2[i]] if src2[i] >= 0 else 0)
            inb, part = l1 * bound, (p0, p1)
        for dst, pl1 in ((i - 1, part[1]),) + (((src2[i], part[0]),) if src2[i] >= 0 else ()):
            v = pl1 * bound if pl1 > 0 and inb > 0 else inb
            b[dst] = np.float32(b[dst] + np.float32(v * (1.0 + 1e-6)))
    return b.astype(np.float64)


def derived_bounds(P, amax0):
    """[layers, n]: kernels.hip::fwd_bounds_kernel from enc1's measured maxima."""
    ld, sk = net()
    return scale_ref.l1_chain(P, ld, sk, np.asarray(amax0, np.float64), False)


def scale_bound(l, T, P, S=None):
    """The bound [n] the launch takes its fp16-pair scale from (None: bf16 triples).  S: what the device returned (what = 15 / 16 / 18)
    as dict(amax0 [n], derived [layers, n], static [layers]); None: the host twins."""
    n = len(T[l.inputs[0]])
    if l.scale is None:
        return None
    if l.scale == 'wv':
        return np.full(n, np.abs(head_wv(P)).max())
    amax0 = S['amax0'] if S else np.abs(np.asarray(T[(ENC1, 'out')])).reshape(n, -1).max(1)
    if l.scale == 'measured':      # (f3d.hip reads the derived bound of pool1's output: enc1's measured maximum, passed on by the pool)
        return np.asarray(S['derived'][POOL1] if S else amax0, np.float64)
    if l.scale == 'derived':
        d = S['derived'] if S else derived_bounds(P, amax0)
        return np.maximum(d[ENC2], d[UP1])
    st = S['static'] if S else bwd_bounds(P)
    return np.full(n, st[{'t3d_bwd_up2': UP2, 'd3d_bwd': DEC1, 't3d8_bwd_up1': UP1, 'bott_bwd': BOTT, 'e3d_bwd': ENC2}[l.name]])


def weight_exp(W):
    return int(14 - frexp_exp(np.abs(W).max()))


def terms(l, T, P):
    """(K, sum |x w|, sum |w|, sum |x|) per element of y."""
    a, W = np.abs(np.asarray(l.core(T, P), np.float64)), np.abs(weights(l, P))
    K = 27 * W.shape[_KAXIS[l.kind]]
    return K, lin(l.kind, a, W), lin(l.kind, np.ones_like(a), W), lin(l.kind, a, np.ones_like(W))


def additions(K, pieces):
    return pieces * (-(-K // 32) + 2) + 32 + 2


def bars(l, T, P, S=None, y=None):
    """The derived bar on y (module docstring), [n, D, H, W, C]."""
    K, xw, sw, sx = terms(l, T, P)
    y = np.abs(lin(l.kind, l.core(T, P), weights(l, P)) if y is None else y)
    if l.split == 'bf16':
        return 2. ** -24 * (3 + additions(K, 6) - 1) * xw + 2. ** -24 * y
    fx = 2. ** (-25. - pair_exp(scale_bound(l, T, P, S))).reshape((-1, 1, 1, 1, 1))
    fw = 2. ** (-25. - weight_exp(weights(l, P)))
    rep = 2 * 2. ** -22 * xw + 2. ** -l.shift * (fx * sw + fw * sx)
    lolo = 2. ** -22 * xw + 2. ** -11 * (fx * sw + fw * sx) + K * fx * fw
    return rep + lolo + 2. ** -24 * (additions(K, 3) - 1) * xw + 2. ** -24 * y


def output_bars(l, by, T):
    """The bar on y carried to the stored float tensors that are selections of y (slices, masks); the channel sums are not here."""
    if l.name == 'c3d_bwd7':
        return {(UP2, 'dout'): by[..., 8:]}
    if l.name == 'd3d_bwd':
        return {(ENC2, 'dout'): by[..., :16], (UP1, 'dout'): by[..., 16:]}
    if l.name in ('t3d_bwd_up2', 't3d8_bwd_up1'):
        k = l.outputs[0]
        return {k: by * T[(k[0], 'sign')]}
    if l.name == 'e3d_bwd':
        return {}
    return {l.outputs[0]: by}      # (a ReLU is 1-Lipschitz, a bias add is inside M)


def e3d_extra(T, P, S=None):
    """The bars of e3d.hip's two sums, whose terms are not stored: (bar of enc2's dsum, bar of enc1's dsum).  enc2: 16 terms, each one
    fp32 add of two stored numbers.  enc1: the routed bar of the contraction (its input carries the rounding of that add: 2^-24 sum
    |x w| more), 8 routed terms and the partial, and the partial's own bar: c3d_bwd7's contraction under enc1's mask, 8 terms."""
    le, lc = BY_NAME['e3d_bwd'], BY_NAME['c3d_bwd7']
    d2 = np.abs(e3d_delta2(T))
    bar2 = 2. ** -24 * d2.sum(-1) + pool_ref.sum_bound(d2.sum(-1), 16)
    K, xw, _, _ = terms(le, T, P)
    g = lin(le.kind, le.core(T, P), weights(le, P))
    routed_bar = e3d_route(bars(le, T, P, S, y=g) + 2. ** -24 * xw, T).sum(-1)
    routed = np.abs(e3d_route(g, T)).sum(-1)
    yc = lin(lc.kind, lc.core(T, P), weights(lc, P))
    m0 = T[(ENC1, 'sign')]
    part_bar = (bars(lc, T, P, S, y=yc)[..., :8] * m0).sum(-1) + pool_ref.sum_bound(np.abs(yc[..., :8] * m0).sum(-1), 8)
    part = np.abs((yc[..., :8] * m0).sum(-1))
    return bar2, routed_bar + part_bar + pool_ref.sum_bound(routed + part, 9)


# ------------------------------------------------------------------------------------------ the split, emulated
def split_f16(v, e, shift=0, drop_lo=False):
    """f16_pair_split on np.float16: v 2^e = h + l 2^-shift (fp32 arithmetic, both pieces rounded to nearest even); returns (h, l 2^-shift)."""
    ws = np.ldexp(np.asarray(v, np.float32), e).astype(np.float32)
    h = ws.astype(np.float16)
    lo = np.ldexp(ws - h.astype(np.float32), shift).astype(np.float16)
    return h.astype(np.float64), np.ldexp((np.zeros_like(lo) if drop_lo else lo).astype(np.float64), -shift)


def split_bf16(v, drop_lo=False):
    """Three bf16 pieces (round to nearest even on the upper 16 bits, the remainder exact in fp32); drop_lo: the leading piece alone."""
    r = np.asarray(v, np.float32).copy()
    out = []
    for _ in range(3):
        u = r.view(np.uint32)
        piece = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)
        out.append(piece.astype(np.float64))
        r = (r - piece).astype(np.float32)
    return out[:1] if drop_lo else out


def emulate(l, T, P, S=None, drop_lo=False):
    """y of the launch from the split pieces of its input (as fp32) and weights, products and sums in fp64: what the representation
    alone costs.  drop_lo: only the leading piece of the input is kept."""
    a, W = np.asarray(l.core(T, P), np.float32), weights(l, P).astype(np.float32)
    if l.split == 'bf16':
        xs, ws = split_bf16(a, drop_lo), split_bf16(W)
        keep = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]
        return sum(lin(l.kind, xs[i], ws[j]) for i, j in keep if i < len(xs))
    ex, ew = pair_exp(scale_bound(l, T, P, S)), weight_exp(W)
    xh, xl = split_f16(a, ex.reshape((-1, 1, 1, 1, 1)).astype(np.int32), l.shift, drop_lo)
    wh, wl = split_f16(W, ew, l.shift)
    y = lin(l.kind, xh, wh) + lin(l.kind, xh, wl) + (0. if drop_lo else lin(l.kind, xl, wh))
    return y * 2. ** (-(ex + ew).astype(np.float64)).reshape((-1, 1, 1, 1, 1))


# ------------------------------------------------------------------------------------------ from x: what check A expects
def compose(x, P, mut=None, at=None):
    """Every tensor of the table from the patches x [n, 32, 32, 32, 1] in fp64; mut: the mutation the launch named `at` runs under."""
    x = np.asarray(x, np.float64).reshape((-1,) + IN_SHAPE)
    T = OrderedDict()
    e1 = np.maximum(lin('conv', x, P['enc1'][0]) + _bias(P, ENC1), 0.)      # direct.hip: input only
    T[(ENC1, 'out')], T[(ENC1, 'sign')] = e1, e1 > 0
    T[(POOL1, 'out')], T[(POOL1, 'argmax')] = pool2(e1)
    T[(POOL1, 'sign')] = T[(POOL1, 'out')] > 0
    for l in LAUNCHES:
        if l.name == 'c3d_bwd7':      # c3d_fwd: input only - the head's sign bytes are the signs of dec2's output
            d2 = lin('conv', _cat(T, (ENC1, 'out'), (UP2, 'out')), P['dec2'][0]) + _bias(P, DEC2)
            T[(DEC2, 'out')] = np.maximum(d2, 0.)
            T[(FC, 'headsign')] = d2 > 0
        T.update(reference(l, T, P, mut if l.name == at else None))
    return T


# ------------------------------------------------------------------------------------------ the integer model of check A
def ternary(shape, seed, keep256):
    """{-1, 0, 1}, kept where a second hash allows: keep256 / 256 of the entries (finer than tests.side_ref._ternary)."""
    h = _hash(int(np.prod(shape)), seed)
    return ((h % 3 - 1) * (((h >> 9) % 256) < keep256)).astype(np.float32).reshape(shape)


HEAD_SCALE = 2.0 ** -6      # the head's integers times a power of two: products stay exact, the logits moderate


def integer_pars(seed, dens):
    """dens: layer name -> keep256.  Conv / conv_transpose weights in {-1, 0, 1} and zero biases; the head in [-2, 2] HEAD_SCALE."""
    ld, sk = net()
    pars = OrderedDict()
    for j, (name, wshape, bshape) in enumerate(netspec.param_shapes(ld, IN_SHAPE, sk)):
        if name == 'fc':
            h = _hash(int(np.prod(wshape)), seed + 100)
            W = ((h % 5 - 2) * (((h >> 9) % 256) < dens[name])).astype(np.float32).reshape(wshape) * np.float32(HEAD_SCALE)
            b = np.array([1., -1.], np.float32).reshape(bshape) * np.float32(HEAD_SCALE)
        else:
            W, b = ternary(wshape, seed + 1 + j, dens[name]), np.zeros(bshape, np.float32)
        pars[name] = [W, b]
    return pars


def integer_x(n, seed):
    x = (_hash(n * 32 ** 3, seed) % 2).astype(np.float32).reshape((n,) + IN_SHAPE)
    x[0], x[1] = 0, 1
    return x


def exactness(l, T, P):
    """The three conditions under which the launch owes equality, as (integers, scale bound / 2^22, accumulator bound / 2^24): its
    inputs and weights are integers (the head's in units of HEAD_SCALE), the bound its fp16-pair scale comes from lies within 22
    bits of that unit, and the absolute sum of the terms of every accumulator - the contraction and the channel sums - within 24."""
    unit = HEAD_SCALE if l.kind.endswith('_bwd') else 1.
    a, W = np.asarray(l.core(T, P), np.float64) / unit, weights(l, P)
    ints = bool(np.all(a == np.round(a)) and np.all(W == np.round(W)))
    b = scale_bound(l, T, P)
    sb = 0. if b is None else float(np.max(b)) / unit / ENGINE_BOUND
    _, xw, _, _ = terms(l, T, P)
    acc = float(xw.max()) / unit
    if l.name == 'e3d_bwd':      # the sums run over routed terms and the partial
        lc = BY_NAME['c3d_bwd7']
        acc = max(acc, float((np.abs(e3d_route(xw, T)).sum(-1) + terms(lc, T, P)[1][..., :8].sum(-1)).max()) / unit)
    else:
        acc = max(acc, float(xw.sum(-1).max()) / unit)
    return ints, sb, acc / ACC_BOUND


# keep256 per layer at the start: enc1 has 27 weights per channel and needs half of them to keep its channels alive on x in {0, 1}
START_DENS = [('enc1', 128), ('enc2', 32), ('bott', 16), ('up1', 16), ('dec1', 16), ('up2', 32), ('dec2', 32), ('fc', 16)]


def alive_channels(T):
    """Per stored activation: the share of its channels that are non-zero somewhere."""
    return {k: float(np.asarray(v).reshape(-1, np.asarray(v).shape[-1]).any(0).mean()) for k, v in T.items() if k[1] == 'out'}


def integer_model(n=3, seed=5, max_tries=24):
    """(x, pars, T, dens): bott, up1 and dec1 - the layers whose norms enc2's static cotangent bound is a product of - are thinned
    (the one of the largest bound contribution first, to 3/4) until every launch of the table meets `exactness`; the seed advances
    until no stored tensor of the table is all zero and dec2 keeps mixed signs.  Deterministic."""
    x = integer_x(n, seed)
    dens = OrderedDict(START_DENS)
    for _ in range(max_tries):
        P = integer_pars(seed, dens)
        st = bwd_bounds(P) / HEAD_SCALE
        if st[ENC2] >= ENGINE_BOUND or st[BOTT] >= ENGINE_BOUND:
            l1 = {nme: bwd_l1_parts(P[nme][0], nme == 'up1', 0)[0] for nme in ('bott', 'up1', 'dec1')}
            nme = max((v, k) for k, v in l1.items() if dens[k] > 1)[1]
            dens[nme] = max(1, dens[nme] * 3 // 4)
            continue
        T = compose(x, P)
        live = all(np.any(np.asarray(v) != 0) for k, v in T.items()) and min(alive_channels(T).values()) >= 0.75
        share = float(T[(FC, 'headsign')][1:].mean())
        if live and 0.05 <= share <= 0.95:
            return x, P, T, dens
        seed += 1000
        x = integer_x(n, seed)
    raise AssertionError('no integer NET-C found')
