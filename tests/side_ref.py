"""The Fisher pass's side-sum reductions stated in NumPy fp64, the dispatch of their kernels restated on the host, and the case
tables of tests/test_gpu_side_sums.py (no device needed: tests/test_side_ref_host.py checks all of this on the CPU).

A Fisher pass keeps, per parameterised layer, the channel sums of the layer's input (asum; asum2 for the second producer of a
concat) and of its pre-activation cotangent under the unit cotangent (dsum), and reduces them to one number per patch:

    conv / fc        S[n] = sum_x dsum[n, x] (1 + sum_t (asum + asum2)[n, x + t - lo])         zero outside the volume
    conv_transpose   S[n] = sum_q (asum + asum2)[n, q] sum_t dsum[n, s q + t - lo] + sum_p dsum[n, p]

(csrc/kernels.hip: k_boxdot_conv / k_boxdot_convT; an fc layer is the 1x1x1 window on one voxel).  fisher_finalize_kernel and
reduce_Asum_kernel turn S and the posteriors into g0, g1, A, trace and Asum.  Everything here is 3-D, [N, D, H, W]: a 2-D layer is
the 3-D one with D = 1, k[0] = 1, s[0] = 1.  lo is the pad-before of oracle.tfops.same_pads.
"""
from collections import OrderedDict, namedtuple

import numpy as np

from oracle import tfops
from tests import conv_ref, convt_ref
from tests.convt_ref import three
from tests.fc_small_ref import EXACT_BOUND, _hash

BOX_SLAB = 1024            # voxels per workgroup of the plain forms (csrc/kernels.hip)
LDS_LIMIT = 48 * 1024      # bytes of LDS a tiled form may take
COL_WINDOWS = ((3, 3, 3), (1, 3, 3), (1, 5, 5))      # the instantiations of boxdot_conv_col_kernel
ENGINE_BOUND = 2.0 ** 22   # values the layer engines compute: an fp16 pair holds 22 bits of an integer


# ------------------------------------------------------------------------------------------ the reductions
def _f64(a, absolute):
    a = np.asarray(a, np.float64)
    return np.abs(a) if absolute else a


def _conv_sum(dsum, asum, asum2, k3, lo, absolute=False, drop=None):
    d = _f64(dsum, absolute)
    a = _f64(asum, absolute) + (0. if asum2 is None else _f64(asum2, absolute))
    assert d.shape == a.shape and d.ndim == 4, (d.shape, a.shape)
    ap = np.pad(a, [(0, 0)] + [(l, k - 1 - l) for l, k in zip(lo, k3)])
    D, H, W = d.shape[1:]
    box = np.zeros_like(d)
    for t in np.ndindex(*k3):
        box += ap[:, t[0]:t[0] + D, t[1]:t[1] + H, t[2]:t[2] + W]
    if drop is not None:      # one tap of one voxel left out: what a kernel with a wrong border does
        x, t = drop
        src = tuple(x[i] + t[i] - lo[i] for i in range(3))
        assert all(0 <= s < n for s, n in zip(src, (D, H, W))), 'the dropped tap lies outside the volume'
        box[(slice(None),) + tuple(x)] -= a[(slice(None),) + src]
    return (d * (1. + box)).reshape(len(d), -1).sum(1)


def _convT_sum(dsum, asum, asum2, k3, s3, lo, absolute=False, drop=None):
    d = _f64(dsum, absolute)
    a = _f64(asum, absolute) + (0. if asum2 is None else _f64(asum2, absolute))
    sp = a.shape[1:]
    assert d.shape[1:] == tuple(n * s for n, s in zip(sp, s3)), (d.shape, a.shape, s3)
    dp = np.pad(d, [(0, 0)] + [(l, k + s) for l, k, s in zip(lo, k3, s3)])
    box = np.zeros_like(a)
    for t in np.ndindex(*k3):
        box += dp[:, t[0]:t[0] + s3[0] * sp[0]:s3[0], t[1]:t[1] + s3[1] * sp[1]:s3[1], t[2]:t[2] + s3[2] * sp[2]:s3[2]]
    if drop is not None:
        q, t = drop
        p = tuple(s3[i] * q[i] + t[i] - lo[i] for i in range(3))
        assert all(0 <= v < n for v, n in zip(p, d.shape[1:])), 'the dropped tap lies outside the volume'
        box[(slice(None),) + tuple(q)] -= d[(slice(None),) + p]
    return (a * box).reshape(len(a), -1).sum(1) + d.reshape(len(d), -1).sum(1)


def boxdot_conv64(dsum, asum, asum2, k3, lo, drop=None):
    """S[n] of a conv (or, with k3 = (1, 1, 1) on one voxel, an fc) layer; fields [N, D, H, W].  drop = (x, t): the tap t of the
    voxel x is left out (the argument that one wrong border tap changes the number)."""
    return _conv_sum(dsum, asum, asum2, k3, lo, drop=drop)


def boxdot_convT64(dsum, asum, asum2, k3, s3, lo, drop=None):
    """S[n] of a conv_transpose layer; dsum on the output grid [N, s D, s H, s W], asum on the input grid.  drop = (q, t)."""
    return _convT_sum(dsum, asum, asum2, k3, s3, lo, drop=drop)


def abs_terms(dsum, asum, asum2, k3, lo, s3=None):
    """The same sum over absolute values (conv / fc: s3 None): what a rounding error of the fp32 additions is relative to."""
    if s3 is None:
        return _conv_sum(dsum, asum, asum2, k3, lo, absolute=True)
    return _convT_sum(dsum, asum, asum2, k3, s3, lo, absolute=True)


def additions(g, with_asum2):
    """M of the float bar: the fp32 additions a form makes per box at the most - the taps, twice with a second source, and for a
    conv_transpose the prod(s) terms of the own-sum and the one rounding of asum + asum2."""
    m = int(np.prod(g['k3'])) * (2 if with_asum2 else 1)
    return m + (int(np.prod(g['s3'])) + 1 if g['type'] == 'conv_transpose' else 0)


def layer_S64(g, dsum, asum, asum2, drop=None):
    if g['type'] == 'conv_transpose':
        return boxdot_convT64(dsum, asum, asum2, g['k3'], g['s3'], g['lo'], drop)
    return boxdot_conv64(dsum, asum, asum2, g['k3'], g['lo'], drop)


def layer_abs(g, dsum, asum, asum2):
    return abs_terms(dsum, asum, asum2, g['k3'], g['lo'], g['s3'] if g['type'] == 'conv_transpose' else None)


# ------------------------------------------------------------------------------------------ finalisation
def finalize64(S, p0f, p1f, sizes, diag_load, p1_branch=None, g=None):
    """fisher_finalize_kernel and reduce_Asum_kernel: S [N, L] fp64, p0f / p1f the fp32 posteriors, sizes [L].
    s0 = float32(p1f s), s1 = float32(-p0f s), g = s / size in fp64; p = p1_branch or p1f decides the branch: p < 1e-6 -> p = 0 and
    g1 = 0, p > 1 - 1e-6 -> p = 1 and g0 = 0; A = (1 - p) g0 g0^T + p g1 g1^T + diag_load I.  Returns a dict with g0, g1 [N, L],
    A [N, L, L], trace [N], Asum [L, L] and A_abs / trace_abs / Asum_abs, the sums of the absolute terms of each.  g = (g0, g1):
    A, trace and Asum are formed from these (the kernel's own fp64 outputs) instead of the ones derived from S."""
    S = np.asarray(S, np.float64)
    N, L = S.shape
    p0 = np.asarray(p0f, np.float32).astype(np.float64).reshape(N, 1)
    p1 = np.asarray(p1f, np.float32).astype(np.float64).reshape(N, 1)
    sizes = np.asarray(sizes, np.float64).reshape(1, L)
    p = (p1 if p1_branch is None else np.asarray(p1_branch, np.float32).astype(np.float64).reshape(N, 1)).copy()
    low, high = p < 1e-6, p > 1. - 1e-6
    p[low], p[high] = 0., 1.
    g0 = (p1 * S).astype(np.float32).astype(np.float64) / sizes
    g1 = (-p0 * S).astype(np.float32).astype(np.float64) / sizes
    g0 = np.where(high, 0., g0)
    g1 = np.where(low, 0., g1)
    if g is not None:
        g0, g1 = (np.asarray(v, np.float64).reshape(N, L) for v in g)
    t0 = (1. - p)[:, :, None] * (g0[:, :, None] * g0[:, None, :])
    t1 = p[:, :, None] * (g1[:, :, None] * g1[:, None, :])
    eye = diag_load * np.eye(L)[None]
    A = t0 + t1 + eye
    A_abs = np.abs(t0) + np.abs(t1) + np.abs(eye)
    ii = np.arange(L)
    return dict(g0=g0, g1=g1, A=A, trace=A[:, ii, ii].sum(1), Asum=A.sum(0), A_abs=A_abs, trace_abs=A_abs[:, ii, ii].sum(1),
                Asum_abs=A_abs.sum(0), low=low[:, 0], high=high[:, 0])


# ------------------------------------------------------------------------------------------ the dispatch, restated
def _tile_bytes(zs, H, W, k3):
    return (zs + k3[0] - 1) * (H + k3[1] - 1) * (W + k3[2] - 1) * 4


def boxdot_zs(D, H, W, k3):
    zs = min(max(4096 // (H * W), 1), D)
    while zs > 1 and _tile_bytes(zs, H, W, k3) > LDS_LIMIT:
        zs -= 1
    return zs


def boxdot_use_lds(D, H, W, k3):
    return D * H * W >= 512 and _tile_bytes(boxdot_zs(D, H, W, k3), H, W, k3) <= LDS_LIMIT


def boxdot_convT_out_ok(ID, IH, IW, k3, s3):
    ivox = ID * IH * IW
    shape = k3[1] == 3 and k3[2] == 3 and s3[1] == 2 and s3[2] == 2 and ((k3[0] == 3 and s3[0] == 2) or (k3[0] == 1 and s3[0] == 1 and ID == 1))
    return shape and IW % 2 == 0 and ivox % 4 == 0 and ivox * 4 <= LDS_LIMIT


def expected_form(typ, grid, k3, s3=None):
    """(form, slabs, z planes per slab or None for slabs of BOX_SLAB voxels) of a layer: typ 'conv', 'conv_transpose' or 'fc'; grid
    the volume the reduction runs over (a conv's output, a conv_transpose's INPUT grid).  k_boxdot_conv / k_boxdot_convT and
    boxdot_conv_slabs / boxdot_convT_slabs of csrc/kernels.hip."""
    D, H, W = grid
    if typ == 'fc':
        return 'plain', 1, None
    if typ == 'conv':
        if boxdot_use_lds(D, H, W, k3):
            zs = boxdot_zs(D, H, W, k3)
            col = tuple(k3) in COL_WINDOWS and W % 4 == 0      # and 16-byte aligned fields: FORMS_UNREACHABLE
            return ('col<%d,%d,%d>' % tuple(k3) if col else 'lds'), -(-D // zs), zs
        return 'plain', -(-(D * H * W) // BOX_SLAB), None
    assert typ == 'conv_transpose', typ
    if boxdot_convT_out_ok(D, H, W, k3, s3):
        zs = min(max(4096 // (H * s3[1] * W * s3[2]), 1), D * s3[0])
        return 'convT_out<3,2>', -(-(D * s3[0]) // zs), zs
    return 'convT_plain', -(-(D * H * W) // BOX_SLAB), None


FORMS = ('plain', 'lds', 'col<3,3,3>', 'col<1,3,3>', 'col<1,5,5>', 'convT_plain', 'convT_out<3,2>')


def layers_of(ld, sk, in_shape):
    """Per parameterised layer of an NN_extended model: name, type, layer index, the grid of its reduction, the grid of dsum, k3,
    s3, lo, the layer indices of its producers (-1: the caller's x; None: no second producer) and its expected form."""
    nd = len(in_shape) - 1
    sp = [1] * (3 - nd) + [int(v) for v in in_shape[:-1]]
    out = []
    for i, (name, spec) in enumerate(ld.items()):
        typ = spec[0]
        src2 = next((s for s, dsts, kind in sk if i in dsts), None)
        if typ == 'conv':
            k3 = three(spec[1][1])
            g = dict(grid=tuple(sp), dgrid=tuple(sp), k3=k3, s3=[1, 1, 1], lo=[tfops.same_pads(n, k, 1)[1] for n, k in zip(sp, k3)])
        elif typ == 'conv_transpose':
            k3, s3 = three(spec[1][1]), three(spec[1][2])
            o = [n * s for n, s in zip(sp, s3)]
            g = dict(grid=tuple(sp), dgrid=tuple(o), k3=k3, s3=s3, lo=[tfops.same_pads(n, k, s)[1] for n, k, s in zip(o, k3, s3)])
            sp = o
        elif typ == 'pool':
            sp = [-(-n // s) for n, s in zip(sp, three(spec[1]))]
            continue
        else:
            assert typ == 'fc', typ
            g = dict(grid=(1, 1, 1), dgrid=(1, 1, 1), k3=[1, 1, 1], s3=[1, 1, 1], lo=[0, 0, 0])
        g.update(name=name, type=typ, layer=i, src=i - 1, src2=src2, pidx=len(out))
        g['form'], g['nslab'], g['planes'] = expected_form(typ, g['grid'], g['k3'], g['s3'])
        out.append(g)
    return out


# ------------------------------------------------------------------------------------------ the fp64 oracle's fields
def oracle_fields(ld, sk, in_shape, pars, x):
    """OracleModel(dtype=float64) on x: per parameterised layer the fields (dsum, asum, asum2) as the device keeps them
    ([N, D, H, W]; asum2 None without a second producer), factored_ref's S64 [N, L], the posteriors [2, N], the sizes and the
    details of tests.factored_ref.factored_unit_scores."""
    import torch
    from oracle.model import OracleModel
    from tests import factored_ref
    om = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
    det = {}
    p, S, sizes = factored_ref.factored_unit_scores(om, np.asarray(x, np.float64), det)
    n = len(x)
    fields = []
    for g in layers_of(ld, sk, in_shape):
        t = g['pidx']
        if g['type'] == 'fc':
            fields.append((det['dsum'][t].reshape(n, 1, 1, 1), det['asum'][t].reshape(n, 1, 1, 1), None))
            continue
        a = np.asarray(x, np.float64) if g['layer'] == 0 else det['out'][g['src']]
        a2 = None if g['src2'] is None else det['out'][g['src2']].sum(-1).reshape((n,) + g['grid'])
        fields.append((det['dsum'][t].reshape((n,) + g['dgrid']), a.sum(-1).reshape((n,) + g['grid']), a2))
    return dict(fields=fields, S=S, p=p, sizes=sizes, det=det, om=om)


# ------------------------------------------------------------------------------------------ integer models
def _ternary(shape, seed, dens16):
    """{-1, 0, 1}, kept where a second hash allows: dens16 sixteenths of the entries."""
    n = int(np.prod(shape))
    h = _hash(n, seed)
    w = (h % 3 - 1) * (((h >> 9) % 16) < dens16)
    return w.astype(np.float32).reshape(shape)


def _integer_pars(ld, sk, in_shape, seed, dens, head_scale=1.):
    from oracle import netspec
    pars = OrderedDict()
    shapes = netspec.param_shapes(ld, in_shape, sk)
    for j, (name, wshape, bshape) in enumerate(shapes):
        if j == len(shapes) - 1:      # the head: W in [-2, 2], an integer bias
            h = _hash(int(np.prod(wshape)), seed + 100)
            W = ((h % 5 - 2) * (((h >> 9) % 16) < dens[j])).astype(np.float32).reshape(wshape) * np.float32(head_scale)
            b = np.array([1., -1.], np.float32).reshape(bshape) * np.float32(head_scale)
        else:
            W, b = _ternary(wshape, seed + 1 + j, dens[j]), np.zeros(bshape, np.float32)
        pars[name] = [W, b]
    return pars


def _layer_op(g, spec, W, b):
    """The layer's linear map as a torch function of its input (channels last; an fc layer takes [F, N])."""
    if g['type'] == 'conv':
        return lambda a: tfops.conv_same(a, W, b)
    if g['type'] == 'conv_transpose':
        return lambda a: tfops.conv_transpose_same(a, W, b, spec[1][2])
    return lambda a: W @ a + b


def exactness(ld, sk, in_shape, pars, x, head_scale=1.):
    """The condition under which bit equality is owed (tests.fc_small_ref.assert_exact), through the fp64 oracle: every activation,
    cotangent, channel sum and box sum of every patch is an integer, and the sum of the absolute values of the terms of each -
    a bound on every partial sum of any summation order - stays below 2^24 (2^22 for what a layer engine computes: an fp16 pair
    holds 22 bits).  Returns (the oracle_fields record, the largest bound over 2^24, the positive share of the head conv's units
    over the patches that are not all zero); raises AssertionError where a value is no integer.  head_scale: the power of two the
    head's integers are multiplied by (below); the logits, every cotangent and S are integers after division by it."""
    import torch
    o = oracle_fields(ld, sk, in_shape, pars, x)
    det, geoms = o['det'], layers_of(ld, sk, in_shape)
    n = len(x)
    sc = 1. / head_scale
    assert np.log2(sc) == np.round(np.log2(sc)) and sc >= 1.
    for arrs, f in ((det['out'][:-1], 1.), (det['out'][-1:], sc), (det['delta'], sc), (det['asum'], 1.), (det['dsum'], sc), ([o['S']], sc)):
        for a in arrs:
            assert np.all(a * f == np.round(a * f)), 'not an integer'
    worst = 0.
    t64 = lambda v: torch.as_tensor(np.abs(np.asarray(v, np.float64)))  # noqa: E731
    for g, (dsum, asum, asum2) in zip(geoms, o['fields']):
        i, t = g['layer'], g['pidx']
        a = np.asarray(x, np.float64) if i == 0 else det['out'][i - 1]
        if g['src2'] is not None:
            a = np.concatenate([det['out'][g['src2']], a], axis=-1)
        if g['type'] == 'fc' and a.ndim > 2:
            a = tfops.flatten_tf(torch.as_tensor(a)).numpy()
        W, b = (t64(v) for v in pars[g['name']])
        av = t64(a).requires_grad_(True)
        fwd = _layer_op(g, ld[g['name']], W, b)(av)
        worst = max(worst, float(fwd.detach().max()) * (sc if t == len(geoms) - 1 else 1.) / ENGINE_BOUND)
        if t > 0:      # the cotangent handed down; twice: a skip source collects two of them
            back, = torch.autograd.grad((fwd * t64(det['delta'][t])).sum(), [av])
            worst = max(worst, 2. * sc * float(back.max()) / ENGINE_BOUND)
        worst = max(worst, sc * float(np.abs(det['delta'][t]).sum(0 if g['type'] == 'fc' else -1).max()) / ENGINE_BOUND,
                    float(np.abs(a).sum(0 if g['type'] == 'fc' else -1).max()) / ENGINE_BOUND,
                    sc * float(layer_abs(g, dsum, asum, asum2).max()) / EXACT_BOUND)
    head = [g for g in geoms if g['type'] != 'fc'][-1]
    pre = det['pre'][head['pidx']]
    live = [j for j in range(n) if np.asarray(x[j]).any()]
    share = float((pre[live] > 0).mean()) if live else 0.
    return o, worst, share


def integer_model(ld, sk, in_shape, n, seed, max_tries=40, head_scale=1.):
    """x in {0, 1} (patch 0 all zero, patch 1 all one), conv / conv_transpose weights in {-1, 0, 1}, zero conv biases, a head in
    [-2, 2]: the pattern of tests.fc_small_ref.bits_exact_inputs for any model.  The weights of the layer with the largest
    fan-in are made sparser (halved density) until `exactness` holds; then the seed is advanced until the head conv keeps mixed
    signs (20 % .. 80 % of its units positive) and every layer's S is non-zero on some patch.  Deterministic.  head_scale, a
    power of two <= 1, multiplies the head's W and b: every product stays exact, the logits - and with them the posteriors -
    stay moderate, and the cotangents and S are integers times head_scale (the finalisation model).  Returns (x, pars, the
    oracle_fields record)."""
    from oracle import netspec
    assert n >= 3
    x = (_hash(n * int(np.prod(in_shape)), seed) % 2).astype(np.float32).reshape((n,) + tuple(in_shape))
    x[0], x[1] = 0, 1
    shapes = netspec.param_shapes(ld, in_shape, sk)
    fan = [float(np.prod(w[:-1])) if len(w) > 2 else float(w[1]) for _, w, _ in shapes]
    dens = [16] * len(shapes)
    for _ in range(max_tries):
        pars = _integer_pars(ld, sk, in_shape, seed, dens, head_scale)
        o, worst, share = exactness(ld, sk, in_shape, pars, x, head_scale)
        if worst >= 1.:
            j = int(np.argmax([f * d if d > 1 else 0. for f, d in zip(fan, dens)]))
            assert dens[j] > 1, 'no exact integer model: every layer is as sparse as it gets'
            dens[j] //= 2
            continue
        L = o['S'].shape[1]
        alive = np.abs(o['S']).max(0) > 0
        if 0.2 <= share <= 0.8 and alive[:L - 1].all():      # (the head's own S is 0: its two cotangents cancel)
            o['worst'], o['share'], o['dens'] = worst, share, list(dens)
            return x, pars, o
        seed += 1000
    raise AssertionError('no integer model with mixed signs found')


# ------------------------------------------------------------------------------------------ case tables
# tag -> kind ('conv', 'convT' or 'concat'), the input volume of the layer under test (2 entries: the 2-D schema), its window,
# stride, environment around model creation, and what the layer under test must reach: (form, slabs, planes per slab)
Case = namedtuple('Case', 'tag kind size k s env form nslab planes')


def _c(tag, kind, size, k, s, form, nslab, planes, env=None):
    return Case(tag, kind, tuple(size), list(k), None if s is None else list(s), env or {}, form, nslab, planes)


CASES = [
    # plain conv: below 512 voxels, or a tile over the LDS limit
    _c('plain-4x3x5-k3', 'conv', (4, 3, 5), [3, 3, 3], None, 'plain', 1, None),
    _c('plain-3x5x6-k2', 'conv', (3, 5, 6), [2, 2, 2], None, 'plain', 1, None),             # even window, lo = 0: all padding behind
    _c('plain-112x112-k5', 'conv', (112, 112), [5, 5], None, 'plain', 13, None),            # 116 x 116 x 4 B > 48 KB; 12544 = 12 x 1024 + 256
    # column form
    _c('col333-8x12x12', 'conv', (8, 12, 12), [3, 3, 3], None, 'col<3,3,3>', 1, 8),         # 36 columns, z split over 7 thread groups
    _c('col333-16x16x16', 'conv', (16, 16, 16), [3, 3, 3], None, 'col<3,3,3>', 1, 16),      # exactly 256 columns
    _c('col333-12x20x20', 'conv', (12, 20, 20), [3, 3, 3], None, 'col<3,3,3>', 2, 10),      # second slab of 2 planes, ZS % 4 != 0
    _c('col333-4x4x512', 'conv', (4, 4, 512), [3, 3, 3], None, 'col<3,3,3>', 4, 1),         # zs 2 -> 1 under the LDS limit
    _c('col133-24x24', 'conv', (24, 24), [3, 3], None, 'col<1,3,3>', 1, 1),
    _c('col133-40x40', 'conv', (40, 40), [3, 3], None, 'col<1,3,3>', 1, 1),                 # 400 columns > 256
    _c('col155-24x24', 'conv', (24, 24), [5, 5], None, 'col<1,5,5>', 1, 1),
    # LDS form
    _c('lds-8x9x9-k3', 'conv', (8, 9, 9), [3, 3, 3], None, 'lds', 1, 8),                    # W % 4 != 0
    _c('lds-8x8x8-k2', 'conv', (8, 8, 8), [2, 2, 2], None, 'lds', 1, 8),
    _c('lds-8x8x8-k1', 'conv', (8, 8, 8), [1, 1, 1], None, 'lds', 1, 8),
    _c('lds-8x9x9-k133', 'conv', (8, 9, 9), [1, 3, 3], None, 'lds', 1, 8),                  # an in-plane window on a 3-D volume
    _c('col133-8x8x8', 'conv', (8, 8, 8), [1, 3, 3], None, 'col<1,3,3>', 1, 8),             # the same window at W % 4 == 0: 8 planes, KZ = 1
    # a concat consumer (asum2) through the column and the LDS form, split and interleaved concat
    _c('cat-col333-8x12x12', 'concat', (8, 12, 12), [3, 3, 3], None, 'col<3,3,3>', 1, 8),
    _c('cat-col333-8x12x12-nosplit', 'concat', (8, 12, 12), [3, 3, 3], None, 'col<3,3,3>', 1, 8, {'ALQ_NO_SPLIT': '1'}),
    _c('cat-lds-8x12x12-k2', 'concat', (8, 12, 12), [2, 2, 2], None, 'lds', 1, 8),
    _c('cat-lds-8x12x12-k2-nosplit', 'concat', (8, 12, 12), [2, 2, 2], None, 'lds', 1, 8, {'ALQ_NO_SPLIT': '1'}),
    # conv_transpose, output-side form
    _c('tout-4x4x4', 'convT', (4, 4, 4), [3, 3, 3], [2, 2, 2], 'convT_out<3,2>', 1, 8),
    _c('tout-2x2x4', 'convT', (2, 2, 4), [3, 3, 3], [2, 2, 2], 'convT_out<3,2>', 1, 4),
    _c('tout-6x6x6', 'convT', (6, 6, 6), [3, 3, 3], [2, 2, 2], 'convT_out<3,2>', 1, 12),
    _c('tout-8x10x10', 'convT', (8, 10, 10), [3, 3, 3], [2, 2, 2], 'convT_out<3,2>', 2, 10),  # two slabs, the second of 6 planes
    _c('tout-4x6-2d', 'convT', (4, 6), [3, 3], [2, 2], 'convT_out<3,2>', 1, 1),
    # plain conv_transpose at 3x3x3 stride 2: ivox % 4 != 0, and the odd widths the output-side form cannot walk
    _c('tplain-3x5x6', 'convT', (3, 5, 6), [3, 3, 3], [2, 2, 2], 'convT_plain', 1, None),
    _c('tplain-5x7-2d', 'convT', (5, 7), [3, 3], [2, 2], 'convT_plain', 1, None),
    _c('tplain-oddw-4x4x3', 'convT', (4, 4, 3), [3, 3, 3], [2, 2, 2], 'convT_plain', 1, None),
    _c('tplain-oddw-2x2x5', 'convT', (2, 2, 5), [3, 3, 3], [2, 2, 2], 'convT_plain', 1, None),
    _c('tplain-oddw-4x5-2d', 'convT', (4, 5), [3, 3], [2, 2], 'convT_plain', 1, None),
    # plain conv_transpose, other geometry (tests.convt_ref.GEOMETRIES)
    _c('tplain-k2s2', 'convT', convt_ref.GEOMETRIES['k2s2']['size'], [2, 2, 2], [2, 2, 2], 'convT_plain', 1, None),
    _c('tplain-2d_k4s2', 'convT', convt_ref.GEOMETRIES['2d_k4s2']['size'][1:], [4, 4], [2, 2], 'convT_plain', 1, None),
]
CASE_IDS = [c.tag for c in CASES]
# the odd-width conv_transpose cases: S is wrong on them without the IW % 2 == 0 term of boxdot_convT_out_ok
ODD_WIDTH = [c.tag for c in CASES if '-oddw-' in c.tag]
UNDER_TEST = {'conv': 'cv', 'convT': 'up', 'concat': 'c3'}


def model_of(c):
    """(layer dict, skips, input shape) of a case: conv(8, 3^nd) -> layer under test -> conv(4, 1x1) -> fc(2), or the skip-concat
    model of tests.conv_ref whose c3 reads two producers."""
    if c.kind == 'conv':
        ld, sk = conv_ref.below_conv(8, 8, c.k, 'MA')
    elif c.kind == 'convT':
        ld, sk = convt_ref.below_conv(8, 8, c.k, c.s, 'M')
    else:
        ld, sk = conv_ref.skip_concat(c.k)
    return ld, sk, tuple(c.size) + (1,)


def under_test(c):
    ld, sk, in_shape = model_of(c)
    return next(g for g in layers_of(ld, sk, in_shape) if g['name'] == UNDER_TEST[c.kind])


# the finalisation models: one tiny conv model, and 15 tiny fc layers in front of the head (L = 16: L L = 256 entries, exactly
# the block of reduce_Asum_kernel)
FIN_N = (1, 63, 64, 65, 129)      # FIN_BLOCK = 64: one, one, one full, two and three blocks of Apart
P1_BRANCH = [0., 5e-7, 1e-6, 0.5, 1. - 1e-6, 1. - 5e-7, 1.]


def fin_model():
    ld, sk = conv_ref.below_conv(8, 8, [3, 3, 3], 'MA')
    return ld, sk, (4, 4, 4, 1)


def l16_model(width=8):
    ld = OrderedDict([('f%d' % i, ['fc', [width], 'MA']) for i in range(15)] + [('fc', ['fc', [2]])])
    return ld, (), (1, 1, 12)


# ------------------------------------------------------------------------------------------ records, computed once and shared
N = 5                      # patches per case: two passes under max_batch = 4, the last one ragged
FIN_SCALE = 2.0 ** -8      # the head of the finalisation model
_CACHE = {}


def integer_case(c):
    """(layer dict, skips, input shape, x, pars, oracle record, layers) of a case's integer model; never modified."""
    key = ('int', c.tag)
    if key not in _CACHE:
        ld, sk, in_shape = model_of(c)
        x, pars, o = integer_model(ld, sk, in_shape, N, 7 + CASE_IDS.index(c.tag))
        _CACHE[key] = (ld, sk, in_shape, x, pars, o, layers_of(ld, sk, in_shape))
    return _CACHE[key]


def float_case(c):
    """The same with he_init weights (bias_std = 0.05) and normal x."""
    from oracle import netspec
    key = ('float', c.tag)
    if key not in _CACHE:
        ld, sk, in_shape = model_of(c)
        seed = 900 + CASE_IDS.index(c.tag)
        pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
        x = np.random.RandomState(seed + 1000).randn(N, *in_shape).astype(np.float32)
        _CACHE[key] = (ld, sk, in_shape, x, pars, None, layers_of(ld, sk, in_shape))
    return _CACHE[key]


def fin_case(n):
    """The finalisation model on n patches: the first n of one stream of max(FIN_N) patches, one set of weights."""
    if 'fin' not in _CACHE:
        ld, sk, in_shape = fin_model()
        x, pars, o = integer_model(ld, sk, in_shape, max(FIN_N), 4242, head_scale=FIN_SCALE)
        _CACHE['fin'] = (ld, sk, in_shape, x, pars, o)
    ld, sk, in_shape, x, pars, o = _CACHE['fin']
    return ld, sk, in_shape, x[:n], pars, o


def l16_case(n=65):
    from oracle import netspec
    if 'l16' not in _CACHE:
        ld, sk, in_shape = l16_model()
        pars = netspec.he_init(ld, in_shape, seed=1616, skips=sk, bias_std=0.05)
        x = np.random.RandomState(1617).randn(n, *in_shape).astype(np.float32)
        _CACHE['l16'] = (ld, sk, in_shape, x, pars)
    return _CACHE['l16']
