"""What the tests of alq_hess_vecp (csrc/hvp.hip, its driver in csrc/grads.hip) share: the fp64 oracle of the product, the fp64
bar with its yardstick, and the table of cases.  CPU only; no test in this file (tests/test_hvp_cases_host.py proves the
conditions below for every case, tests/test_gpu_hvp.py runs the cases on the device).

Truth: `torch.autograd.grad(..., create_graph=True)` twice through `OracleModel(..., dtype=torch.float64)._graph` (oracle_hv).
Per parameter array k, from the truth alone (yardsticks()):
  Hv64_k   the product on the batch;  h_n its sample-by-sample evaluation with the same loss_scale;
  u64_k  = max |sum_rev h_n - Hv64_k|: the truth's own fp64 noise under another summation order (samples in reverse);
  G_k    = max over entries of sum_n |h_n|: the gross magnitude, >= max |Hv64_k|, which does not shrink when samples cancel;
  e32_k  = max |Hv32_k - Hv64_k|, Hv32 the same through the fp32 OracleModel;
  b64_k  = 2^-38 G_k: the bar (bars64).  2^-38 is the geometric middle of what one fp32 rounding leaves (2^-24) and fp64
           (2^-53).  G_k == 0: the array must be exactly zero.
The bar means something only where (conditions(), conditions on the chosen inputs, settled by the oracle alone)
  noise margin     b64_k >= 64 u64_k: the truth's own rounding is far below the bar;
  discrimination   b64_k <= e32_k / 1024: the bar separates an fp64 evaluation from an fp32 one;
  decision margin  no fragile ReLU or pool decision at EPS_TIGHT = 2e-5, five times ref64.DEFAULT_EPS (the fp32 forward pass,
                   whose decisions the product is evaluated on, is 3e-6 off on values of 6: DESIGN.md).
Seeds were searched on the CPU; no sample is skipped.
"""
import functools
from collections import OrderedDict

import numpy as np

from oracle import netspec
from oracle.model import OracleModel
from tests.test_gpu_lsum import net_3d_skip, net_wide_fc

N = 5               # odd and below a wave
EPS = 4e-6          # ref64.DEFAULT_EPS (asserted in test_gpu_hvp.test_hv_vs_fp64)
EPS_TIGHT = 2e-5
B64 = 2. ** -38
MAX_BATCH = 8
PARTIAL_DOUBLES = 1 << 22      # hvp_wgrad_partial_doubles: the slab partials of one weight product


# ------------------------------------------------------------------------------------------ the oracle
def fragile_units(om64, x, eps=EPS):
    """Number of fragile ReLU / max-pool decisions of the fp64 evaluation of every sample: |ReLU input| <= eps * rms of the
    layer's pre-activation of the sample; the two largest inputs of a pool window within eps * rms of the pool's input, maximum
    positive (the rule of alq_ref64_scores restated on the oracle's pre-activations)."""
    import torch
    import torch.nn.functional as F
    import oracle.model as omod
    from oracle import tfops
    count = [0]
    real_relu, real_pool = torch.relu, tfops.max_pool_same

    def per_sample_rms(t, sample_axis):
        t2 = t.detach() ** 2
        dims = [d for d in range(t.dim()) if d != sample_axis]
        return torch.sqrt(t2.mean(dim=dims, keepdim=True))

    def relu(t):
        ax = 1 if t.dim() == 2 else 0                   # fc activations are [features, N]
        count[0] += int((t.detach().abs() <= eps * per_sample_rms(t, ax)).sum())
        return real_relu(t)

    def pool(t, window, strides):
        out = real_pool(t, window, strides)
        nd = t.dim() - 2
        xc = tfops._to_cf(t.detach())
        flat = []
        for d in reversed(range(nd)):
            _, lo, hi = tfops.same_pads(t.shape[1 + d], list(window)[d], list(strides)[d])
            flat += [lo, hi]
        xp = F.pad(xc, flat, value=float('-inf'))
        fn = F.max_pool2d if nd == 2 else F.max_pool3d
        best, idx = fn(xp, list(window), list(strides), return_indices=True)
        shp = xp.shape
        x2 = xp.reshape(shp[0], shp[1], -1).clone()
        x2.scatter_(2, idx.reshape(shp[0], shp[1], -1), float('-inf'))
        second = fn(x2.reshape(shp), list(window), list(strides))
        rms = per_sample_rms(t, 0).reshape(-1, *([1] * (nd + 1)))
        count[0] += int(((best > 0) & ((best - second) <= eps * rms)).sum())
        return out

    torch.relu, tfops.max_pool_same = relu, pool
    try:
        with torch.no_grad():
            om64._graph(om64._as_input(x))
    finally:
        torch.relu, tfops.max_pool_same = real_relu, real_pool
    assert omod.torch.relu is real_relu
    return count[0]


tight = functools.partial(fragile_units, eps=EPS_TIGHT)      # the predicate for convt_ref.first_stable_patches


def oracle_hv(om, x, labels, v_list, names, loss_scale):
    """Double-backward through the oracle: H v over the variables of the layers `names`, H the Hessian of
    loss_scale * sum_n CE (labels outside [0, c) add nothing); list [HW, Hb, ...] of float64 arrays."""
    import torch
    z = om._graph(om._as_input(x))['output']                 # [c, N]
    c = z.shape[0]
    lab = np.asarray(labels)
    y = np.zeros((c, len(lab)))
    for n, l in enumerate(lab):
        if 0 <= l < c:
            y[l, n] = 1.
    logp = z - torch.logsumexp(z, dim=0, keepdim=True)
    loss = -(torch.as_tensor(y).to(z.dtype) * logp).sum() * torch.tensor(float(np.float32(loss_scale))).to(z.dtype)
    plist = [p for nme in names for p in om.params[nme]]
    grads = torch.autograd.grad(loss, plist, create_graph=True)
    dot = sum((g * torch.as_tensor(np.asarray(v, dtype=np.float32)).to(z.dtype).reshape(g.shape)).sum() for g, v in zip(grads, v_list))
    hv = torch.autograd.grad(dot, plist, allow_unused=True)
    return [np.zeros(tuple(p.shape)) if h is None else h.detach().numpy().astype(np.float64) for p, h in zip(plist, hv)]


# ------------------------------------------------------------------------------------------ the yardstick and the bar
def yardsticks(om64, om32, x, labels, v, names, loss_scale, hv64=None, hv32=None):
    """dict(hv64, hv32, u64, G, e32, b64), the last four one figure per array (module docstring)."""
    x, labels = np.asarray(x), np.asarray(labels)
    if hv64 is None:
        hv64 = oracle_hv(om64, x, labels, v, names, loss_scale)
    if hv32 is None:
        hv32 = oracle_hv(om32, x, labels, v, names, loss_scale)
    rev = [np.zeros_like(a) for a in hv64]
    gross = [np.zeros_like(a) for a in hv64]
    for n in reversed(range(len(x))):
        for s, g, h in zip(rev, gross, oracle_hv(om64, x[[n]], labels[[n]], v, names, loss_scale)):
            s += h
            g += np.abs(h)
    G = [float(g.max()) for g in gross]
    return dict(hv64=hv64, hv32=hv32, u64=[float(np.abs(s - a).max()) for s, a in zip(rev, hv64)], G=G,
                e32=[float(np.abs(a32 - a).max()) for a32, a in zip(hv32, hv64)], b64=[B64 * g for g in G])


def bars64(y):
    """Per array: 2^-38 G_k, from a record of yardsticks()."""
    return list(y['b64'])


def conditions(y, om64, x, arrays=None):
    """The violations of the three conditions of the module docstring, as a list of strings (empty: bars64 applies)."""
    bad = []
    arrays = arrays or ['array %d' % k for k in range(len(y['b64']))]
    for nme, u, G, e32, b in zip(arrays, y['u64'], y['G'], y['e32'], y['b64']):
        if not G > 0:
            bad.append('%s: G == 0, the bar is exact equality and separates nothing' % nme)
            continue
        if not b >= 64 * u:
            bad.append('%s: noise margin: b64 %.3e < 64 u64 %.3e' % (nme, b, u))
        if not b <= e32 / 1024:
            bad.append('%s: discrimination: b64 %.3e > e32 %.3e / 1024' % (nme, b, e32))
    frag = tight(om64, x)
    if frag:
        bad.append('decision margin: %d fragile units at %g' % (frag, EPS_TIGHT))
    return bad


def figures(tag, y, arrays=None):
    """One printed line per array: u64, G, e32, b64 and the two margins."""
    arrays = arrays or ['array %d' % k for k in range(len(y['b64']))]
    for nme, u, G, e32, b in zip(arrays, y['u64'], y['G'], y['e32'], y['b64']):
        print('%s %s: u64 %.3e  G %.3e  e32 %.3e  b64 %.3e  b64/u64 %.3g  e32/b64 %.3g'
              % (tag, nme, u, G, e32, b, b / max(u, 1e-300), e32 / max(b, 1e-300)))


def hold64(tag, got, y, arrays=None):
    """Prints e(device) and e(device) / b64 per array, then asserts e(device) <= b64 (exact zero where G == 0) on all of them.
    Returns the largest e(device) / b64."""
    arrays = arrays or ['array %d' % k for k in range(len(y['b64']))]
    assert len(got) == len(y['hv64']) == len(arrays), (tag, len(got), len(y['hv64']))
    bad, worst = [], 0.
    for nme, a, a64, b in zip(arrays, got, y['hv64'], y['b64']):
        assert a.dtype == np.float64 and a.shape == a64.shape, (tag, nme)
        e = float(np.abs(a - a64).max())
        print('%s %s: e(device) %.3e  b64 %.3e  e(device) / b64 %.3e' % (tag, nme, e, b, e / b if b > 0 else float(e > 0)))
        worst = max(worst, e / b if b > 0 else float(e > 0))
        if not e <= b:
            bad.append((nme, e, b))
    assert not bad, (tag, 'above the fp64 bar', bad)
    return worst


# ------------------------------------------------------------------------------------------ the nets
def net_pool_route():
    """3-D conv, a SAME pool with the non-cubic window (1, 2, 2), then a second pool (2, 2, 1)."""
    return OrderedDict([('conv1', ['conv', [4, [3, 3, 3]], 'MA']), ('pool1', ['pool', [1, 2, 2]]), ('pool2', ['pool', [2, 2, 1]]),
                        ('fc', ['fc', [3]])])


def net_pool_w3():
    """3-D conv and a SAME pool of window 3 whose padding starts in front of the volume (lo = 1 on every axis of (7, 7, 4))."""
    return OrderedDict([('conv1', ['conv', [4, [3, 3, 3]], 'MA']), ('pool1', ['pool', [3, 3, 3]]), ('fc', ['fc', [3]])])


def net_no_relu():
    """A conv and an fc layer without ReLU (ops 'M') in the middle of the net, between ReLU layers (2-D, NN_extended schema)."""
    k = [3, 3]
    return OrderedDict([('conv1', ['conv', [6, k], 'MA']), ('conv2', ['conv', [5, k], 'M']), ('conv3', ['conv', [4, k], 'MA']),
                        ('fc1', ['fc', [12], 'MA']), ('fc2', ['fc', [10], 'M']), ('fc3', ['fc', [8], 'MA']), ('fc4', ['fc', [3]])])


def net_fc_geom():
    """conv -> fc(ReLU) -> fc(ReLU) -> head: on a (3, 4, 5) input the first fc reads D, H, W, C = 3, 4, 5, 2, the second (1, 1, 1, F)."""
    return OrderedDict([('conv1', ['conv', [2, [3, 3, 3]], 'MA']), ('fc1', ['fc', [7], 'MA']), ('fc2', ['fc', [6], 'MA']), ('fc3', ['fc', [4]])])


def net_fc_wide():
    """conv -> a wide fc layer (768 = 2 x 4 x 8 x 12 inputs, 256 units: the streaming GEMM's shape, packed on the device) -> head."""
    return OrderedDict([('conv1', ['conv', [12, [3, 3, 3]], 'MA']), ('fc1', ['fc', [256], 'MA']), ('fc2', ['fc', [3]])])


def net_labels(c):
    """conv -> pool -> a head of c classes (NN.CNN schema)."""
    return OrderedDict([('conv1', [6, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [c, 'fc'])])


def net_slab_cap():
    """1x1 conv 1 -> 64, then the 5x5 conv 64 -> 64 whose weight product has M = 102,400 entries, two-class head.  Neither conv has
    a ReLU and there is no pool: 46 x 46 x 64 units per sample leave no input with the decision margin (none in 80 seeds), and
    the slab walk of hvp_wgrad_kernel does not depend on them - both terms of the product are still on."""
    return OrderedDict([('conv1', ['conv', [64, [1, 1]], 'M']), ('conv2', ['conv', [64, [5, 5]], 'M']), ('fc', ['fc', [2]])])


def _mixed_labels(c):
    """7 samples, labels -1 and c mixed among valid ones."""
    def f(rs, n):
        lab = rs.randint(0, c, size=n).astype(np.int32)
        lab[[0, 5]] = -1
        lab[2] = c
        return lab
    return f


def _table():
    """name -> dict(ld, in_shape, sk, wseed, xseed, n, labels): weights he_init(seed=wseed, bias_std=0.05), everything else
    from RandomState(xseed).  The first four are the nets of test_gpu_lsum._nets() that the first issue named plus a two-class
    3-D net (fused two-class head)."""
    ld4, sk4 = net_3d_skip(4)
    ld2, sk2 = net_3d_skip(2)
    rows = [('neta_c3', netspec.net_a(nclass=3), (20, 20, 1), (), 71, 17, N, None),
            ('net3d_skip_c4', ld4, (8, 8, 8, 1), sk4, 73, 19, N, None),
            ('wide_fc_c5', net_wide_fc(5), (8, 8, 1), (), 74, 20, N, None),
            ('net3d_skip_c2', ld2, (8, 8, 8, 1), sk2, 77, 36, N, None),
            ('pool_route', net_pool_route(), (5, 7, 6, 2), (), 81, 1, N, None),
            ('pool_w3', net_pool_w3(), (7, 7, 4, 2), (), 82, 1, N, None),
            ('no_relu', net_no_relu(), (6, 5, 2), (), 83, 1, N, None),
            ('fc_geom', net_fc_geom(), (3, 4, 5, 1), (), 84, 1, N, None),
            ('fc_wide', net_fc_wide(), (2, 4, 8, 1), (), 85, 1, N, None),
            ('labels_c2', net_labels(2), (6, 6, 1), (), 86, 1, 7, _mixed_labels(2)),
            ('labels_c21', net_labels(21), (6, 6, 1), (), 87, 1, 7, _mixed_labels(21)),
            ('slab_cap', net_slab_cap(), (46, 46, 1), (), 88, 1, N, None),
            ('one_sample', net_pool_route(), (5, 7, 6, 2), (), 81, 1, 1, None),
            ('full_batch', ld4, (8, 8, 8, 1), sk4, 73, 5, MAX_BATCH, None)]
    return OrderedDict((r[0], dict(zip(('ld', 'in_shape', 'sk', 'wseed', 'xseed', 'n', 'labels'), r[1:]))) for r in rows)


TABLE = _table()
FOUR_NETS = list(TABLE)[:4]
_CASES = {}


def case(name):
    """Weights, inputs, labels, a vector, both oracles and their products of one case: computed once, shared, never modified."""
    if name in _CASES:
        return _CASES[name]
    import torch
    t = TABLE[name]
    ld, in_shape, sk, n = t['ld'], t['in_shape'], t['sk'], t['n']
    pars = netspec.he_init(ld, in_shape, seed=t['wseed'], skips=sk, bias_std=0.05)
    rs = np.random.RandomState(t['xseed'])
    x = rs.randn(n, *in_shape).astype(np.float32)
    names = list(pars.keys())
    c = np.asarray(pars[names[-1]][0]).shape[0]
    labels = t['labels'](rs, n) if t['labels'] else rs.randint(0, c, size=n).astype(np.int32)
    v = [rs.randn(*np.asarray(a).shape).astype(np.float32) for nme in names for a in pars[nme]]
    om64 = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
    om32 = OracleModel(ld, in_shape, pars, skips=sk)
    d = dict(name=name, ld=ld, in_shape=in_shape, sk=sk, pars=pars, x=x, labels=labels, v=v, names=names, om64=om64, om32=om32, c=c, n=n,
             arrays=[nme + s for nme in names for s in ('/W', '/b')],
             hv64=oracle_hv(om64, x, labels, v, names, 1. / n), hv32=oracle_hv(om32, x, labels, v, names, 1. / n))
    _CASES[name] = d
    return d


_YARDS = {}


def yard(name, chosen=None, v=None, key=None):
    """yardsticks() of a case of the table, over the layers `chosen` (default: all) and the vector `v` (a list over the chosen
    layers' arrays; default: the case's own): computed once per (name, chosen, key), `key` naming another vector."""
    d = case(name)
    k = (name, tuple(chosen) if chosen else None, key)
    if k not in _YARDS:
        full = chosen is None and v is None
        names = d['names'] if chosen is None else list(chosen)
        vs = v if v is not None else [d['v'][2 * d['names'].index(nme) + q] for nme in names for q in (0, 1)]
        _YARDS[k] = yardsticks(d['om64'], d['om32'], d['x'], d['labels'], vs, names, 1. / d['n'],
                               d['hv64'] if full else None, d['hv32'] if full else None)
        _YARDS[k]['arrays'] = [nme + s for nme in names for s in ('/W', '/b')]
    return _YARDS[k]


def labelled_only(name):
    """(positions of the samples whose label lies in [0, c), yardsticks of the batch of those samples alone under the loss_scale of
    the whole case): the other side of test_gpu_hvp.test_unlabelled_rows."""
    d = case(name)
    keep = [i for i, l in enumerate(d['labels']) if 0 <= l < d['c']]
    k = (name, None, 'labelled only')
    if k not in _YARDS:
        _YARDS[k] = yardsticks(d['om64'], d['om32'], d['x'][keep], d['labels'][keep], d['v'], d['names'], 1. / d['n'])
        _YARDS[k]['arrays'] = d['arrays']
    return keep, _YARDS[k]


def symmetry_u(d):
    """The second vector of test_gpu_hvp.test_symmetry (yard(..., v=u, key='u'))."""
    rs = np.random.RandomState(31)
    return [rs.randn(*a.shape).astype(np.float32) for a in d['v']]


def subsets(name):
    """Every layer alone and "all but layer t" for every t, as lists of layer names in the net's order."""
    names = case(name)['names']
    return [[nme] for nme in names] + [[o for o in names if o != nme] for nme in names]


# ------------------------------------------------------------------------------------------ whole models of other test files
def whole_tight(d):
    """For a whole-model record of the form tests/test_gpu_convt.whole_record builds: the patches the fp64 bar is applied on - the
    record's own where they have the decision margin, else the first d['n'] of the same stream (tests/convt_ref.first_stable_patches
    over 16 n patches) that have it -, their yardsticks and the violations of the three conditions; dict(x, chosen, y, bad).  The
    labels and the vector are the record's.  Computed once per record."""
    if 'hv_tight' not in d:
        from tests import convt_ref
        n, x, chosen = d['n'], d['x'], None
        if tight(d['om64'], x) != 0:
            x, chosen = convt_ref.first_stable_patches(d['om64'], d['in_shape'], d['seed'] + 1000, n, 16 * n, tight)
        if len(x) < n:
            d['hv_tight'] = dict(x=None, chosen=chosen, y=None, bad=['only %d of %d patches with the decision margin' % (len(x), n)])
        else:
            y = yardsticks(d['om64'], d['om32'], x, d['labels'], d['v'], d['names'], 1. / n)
            d['hv_tight'] = dict(x=x, chosen=chosen, y=y, bad=conditions(y, d['om64'], x, d['arrays']))
    return d['hv_tight']


# ------------------------------------------------------------------------------------------ launch rules restated
def wgrad_slabs(rows, M):
    """k_hvp_wgrad's rule: (nslab, rows per slab) of a weight product of M entries over `rows` (sample, voxel) rows."""
    nslab = min(max(rows // 256, 1), max(max(PARTIAL_DOUBLES, M) // M, 1), 65535)
    rps = -(-rows // nslab)
    return -(-rows // rps), rps


def conv_products(name):
    """Per conv / conv_transpose layer of a case: (layer name, rows, voxels of one sample of the walked grid, M, nslab, rows per
    slab, which of the three limits set nslab).  The walked grid is the conv's output, the conv_transpose's input."""
    from nnal_amd.device_host import translate_layers, tf_param_shapes
    from nnal_amd._lib import ALQ_CONV, ALQ_CONVT, ALQ_POOL
    d = case(name)
    layers = translate_layers(d['ld'], d['in_shape'], d['sk'])
    shapes = {nme: w for nme, w, _ in tf_param_shapes(layers, d['in_shape'])}
    nd = len(d['in_shape']) - 1
    spatial = list(d['in_shape'][:-1])
    out = []
    for ly in layers:
        if ly['type'] == ALQ_POOL:
            spatial = [-(-a // b) for a, b in zip(spatial, ly['s'][3 - nd:])]
        elif ly['type'] in (ALQ_CONV, ALQ_CONVT):
            vox = int(np.prod(spatial))          # a conv keeps the grid; a conv_transpose walks its input
            if ly['type'] == ALQ_CONVT:
                spatial = [a * b for a, b in zip(spatial, ly['s'][3 - nd:])]
            rows, M = d['n'] * vox, int(np.prod(shapes[ly['name']]))
            nslab, rps = wgrad_slabs(rows, M)
            limit = 'rows' if nslab == max(rows // 256, 1) else 'cap'
            if max(PARTIAL_DOUBLES, M) // M < rows // 256:
                limit = 'cap'
            out.append((ly['name'], rows, vox, M, nslab, rps, limit))
    return out
