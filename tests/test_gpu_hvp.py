"""Exact Hessian-vector products on the device (alq_hess_vecp, csrc/hvp.hip), their host interface and the influence solver
on top of them, against torch double-backward through the fp64 oracle (GPU box).

Truth: `torch.autograd.grad(..., create_graph=True)` twice through `OracleModel(..., dtype=torch.float64)._graph`.
Yardstick: the same through the fp32 OracleModel, an independent fp32 implementation.  Per parameter array
e = max |Hv - Hv64|, and the bar is e(device) <= 2 e(fp32 oracle) + 6e-8 mean |Hv64 entry| (the bar of test_gpu_lsum: factor 2
for another summation order, the floor one fp32 rounding of a typical entry).

The product is discontinuous where a ReLU input or a max-pool near-tie lies within fp32 rounding of its boundary; the
seeds below were searched on the CPU so that the fp64 evaluation of every sample of every net has NO fragile decision at
ref64.DEFAULT_EPS (rule of alq_ref64_scores restated on the oracle's pre-activations: |ReLU input| <= eps * rms of the
layer's pre-activation of the sample; the two largest inputs of a pool window within eps * rms of the pool's input, maximum
positive).  The tests assert that and skip no sample.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests.test_gpu_lsum import net_3d_skip, net_wide_fc  # noqa: E402

N = 5          # odd and below a wave
EPS = 4e-6     # ref64.DEFAULT_EPS (asserted in test_hv_vs_fp64)


def _hv_nets():
    """(name, layer dict, input shape, skips, weight seed, input seed): the nets of test_gpu_lsum._nets() that the issue names
    plus a two-class 3-D net (fused two-class head); seeds with no fragile unit in fp64 (module docstring)."""
    ld4, sk4 = net_3d_skip(4)
    ld2, sk2 = net_3d_skip(2)
    return [('neta_c3', netspec.net_a(nclass=3), (20, 20, 1), (), 71, 17),
            ('net3d_skip_c4', ld4, (8, 8, 8, 1), sk4, 73, 19),
            ('wide_fc_c5', net_wide_fc(5), (8, 8, 1), (), 74, 20),
            ('net3d_skip_c2', ld2, (8, 8, 8, 1), sk2, 77, 21)]


_NETS = {n[0]: n for n in _hv_nets()}


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


# ------------------------------------------------------------------------------------------ oracle side (CPU)
def fragile_units(om64, x, eps=EPS):
    """Number of fragile ReLU / max-pool decisions of the fp64 evaluation of every sample (module docstring)."""
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


_CASES = {}


def case(name):
    """Weights, inputs, labels, a vector and both oracle products of one net: computed once, shared, never modified."""
    if name in _CASES:
        return _CASES[name]
    import torch
    _, ld, in_shape, sk, wseed, xseed = _NETS[name]
    pars = netspec.he_init(ld, in_shape, seed=wseed, skips=sk, bias_std=0.05)
    rs = np.random.RandomState(xseed)
    x = rs.randn(N, *in_shape).astype(np.float32)
    names = list(pars.keys())
    c = np.asarray(pars[names[-1]][0]).shape[0]
    labels = rs.randint(0, c, size=N).astype(np.int32)
    v = [rs.randn(*np.asarray(a).shape).astype(np.float32) for nme in names for a in pars[nme]]
    om64 = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
    om32 = OracleModel(ld, in_shape, pars, skips=sk)
    d = dict(ld=ld, in_shape=in_shape, sk=sk, pars=pars, x=x, labels=labels, v=v, names=names, om64=om64, om32=om32, c=c,
             hv64=oracle_hv(om64, x, labels, v, names, 1. / N), hv32=oracle_hv(om32, x, labels, v, names, 1. / N))
    _CASES[name] = d
    return d


def bars(hv64, hv32):
    """Per array: 2 e(fp32 oracle) + 6e-8 mean |Hv64 entry|."""
    return [2 * np.abs(a32 - a64).max() + 6e-8 * np.abs(a64).mean() for a64, a32 in zip(hv64, hv32)]


def mk(sess, d, max_batch=8, feature_layer=None):
    from nnal_amd import device
    m = device.DeviceModel(sess, d['ld'], d['in_shape'], d['sk'], feature_layer=feature_layer, max_batch=max_batch)
    m.set_weights(d['pars'])
    return m


def sub(v, names, chosen):
    return [v[2 * names.index(nme) + k] for nme in chosen for k in (0, 1)]


# ------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize('name', list(_NETS))
def test_hv_vs_fp64(sess, name):
    """The bar of the module docstring, per parameter array, no sample skipped.  The product is evaluated in fp64 on the
    forward pass's decisions (csrc/hvp.hip), so with no fragile decision e(device) is fp64 rounding.  Prints
    e(device) / e(fp32 oracle) per array: the figures of DESIGN.md's accuracy table."""
    from nnal_amd import ref64
    assert EPS == ref64.DEFAULT_EPS
    d = case(name)
    assert fragile_units(d['om64'], d['x']) == 0, (name, 'a fragile decision in fp64: pick other seeds')
    m = mk(sess, d)
    hv = m.hess_vecp(d['x'], d['labels'], d['v'])
    bar = bars(d['hv64'], d['hv32'])
    assert len(hv) == len(d['hv64']) == 2 * m.L
    bad = []
    for k, (a, a64, a32, b) in enumerate(zip(hv, d['hv64'], d['hv32'], bar)):
        assert a.dtype == np.float64 and a.shape == a64.shape
        e, e32 = np.abs(a - a64).max(), np.abs(a32 - a64).max()
        print('%s array %d (%s %s): e(device) %.3e  e(fp32 oracle) %.3e  ratio %.2e  floor %.3e  max|Hv64| %.3e'
              % (name, k, d['names'][k // 2], 'Wb'[k % 2], e, e32, e / max(e32, 1e-300), 6e-8 * np.abs(a64).mean(), np.abs(a64).max()))
        if not e <= b:
            bad.append((k, e, b))
    m.close()
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------ 2. layer subsets
@pytest.mark.parametrize('which', ['last_fc', 'middle_conv', 'two_apart'])
def test_layer_subsets(sess, which):
    """Other layers are held constant: the fp64 product over the chosen variables only.  Entries of the other layers are
    exact zeros in the flat device vector, and their entries of v - NaN here - are never read."""
    d = case('net3d_skip_c4')
    names = d['names']
    chosen = {'last_fc': [names[-1]], 'middle_conv': [names[1]], 'two_apart': [names[0], names[3]]}[which]
    vs = sub(d['v'], names, chosen)
    h64 = oracle_hv(d['om64'], d['x'], d['labels'], vs, chosen, 1. / N)
    h32 = oracle_hv(d['om32'], d['x'], d['labels'], vs, chosen, 1. / N)
    m = mk(sess, d)
    torch = sess.torch
    idx = m.hess_layer_idx(chosen)
    full = np.full(m.num_params, np.nan, dtype=np.float32)
    offs = m._param_offsets()
    for t, (vw, vb) in zip(idx, zip(vs[0::2], vs[1::2])):
        o, nw, nb = offs[t]
        full[o:o + nw] = vw.ravel()
        full[o + nw:o + nw + nb] = vb.ravel()
    tx, n = m._as_device_batch(d['x'])
    out, _ = m.hess_vecp_device(tx, n, sess.to_device(d['labels'], torch.int32), sess.to_device(full, torch.float32), idx, 1. / N)
    flat = out.cpu().numpy()
    assert np.all(np.isfinite(flat))
    got = m.unflatten(flat, idx)
    for t in range(m.L):
        if t not in idx:
            o, nw, nb = offs[t]
            assert np.all(flat[o:o + nw + nb] == 0.0), t
    for k, (a, a64, b) in enumerate(zip(got, h64, bars(h64, h32))):
        e = np.abs(a - a64).max()
        print('%s array %d: e(device) %.3e  bar %.3e' % (which, k, e, b))
        assert e <= b, (which, k, e, b)
    # the list interface gives the same bits
    lst = m.hess_vecp(d['x'], d['labels'], vs, layers=chosen)
    for a, b in zip(lst, got):
        np.testing.assert_array_equal(a, b)
    m.close()


# ------------------------------------------------------------------------------------------ 3. last-layer closed form
def test_last_layer_closed_form(sess):
    """Only the last fc layer on: Hv = loss_scale sum_n ((diag(p_n) - p_n p_n^T)(V a_n + c)) [a_n^T, 1], on the host in fp64
    from the device's own posteriors (divided by their sum) and feature activations as alq_forward returns them (no torch).
    The product evaluates the same network on the same ReLU / pool decisions in fp64, so the two sides differ by what the
    fp32 forward pass is off by: |da| <= 1e-5 (1 + |a|) per feature and |dp| <= 2e-5 per posterior, the bars the suite holds the
    forward pass to (test_gpu_parity's feature_layer bar; the smoke run's posterior bar).  Propagated: dRz_n <= max_j sum_f |V_jf|
    da_nf; with R = max_j |Rz_nj|, Rdelta_j = ls p_j (Rz_j - sum_k p_k Rz_k) moves by at most ls (2 dRz + (2 + 3 c) dp R) (p_j <= 1;
    dp enters through p_j, through the sum and through the normalisation); the outer product with [a, 1] carries that linearly
    and adds |Rdelta| da.  The fp64 roundings of either side are far below."""
    d = case('wide_fc_c5')
    names = d['names']
    m = mk(sess, d, feature_layer=len(d['ld']) - 2)
    res = m.forward(d['x'], want=('posteriors', 'feature_layer'))
    p = res['posteriors'].astype(np.float64)               # [c, n]
    a = res['feature_layer'].astype(np.float64)            # [F, n]
    V, cb = [np.asarray(t, np.float64) for t in sub(d['v'], names, [names[-1]])]
    ls = float(np.float32(1. / N))
    Rz = V @ a + cb.reshape(-1, 1)                          # [c, n]
    p = p / p.sum(0, keepdims=True)
    Rd = ls * p * (Rz - (p * Rz).sum(0, keepdims=True))
    HW = Rd @ a.T
    Hb = Rd.sum(1).reshape(cb.shape)
    da, dp, c = 1e-5 * (1 + np.abs(a)), 2e-5, d['c']
    dRz = (np.abs(V) @ da).max(0)                           # [n]
    errd = ls * (2 * dRz + (2 + 3 * c) * dp * np.abs(Rz).max(0))          # [n] per-entry error of Rdelta
    bW = (np.ones((c, 1)) * errd) @ np.abs(a).T + np.abs(Rd) @ da.T
    bb = errd.sum()
    got = m.hess_vecp(d['x'], d['labels'], [V, cb], layers=[names[-1]])
    print('closed form: max |dW| %.3e (bound %.3e), max |db| %.3e (bound %.3e)' % (np.abs(got[0] - HW).max(), bW.max(),
                                                                                 np.abs(got[1] - Hb).max(), bb))
    assert np.all(np.abs(got[0] - HW) <= bW)
    assert np.all(np.abs(got[1] - Hb) <= bb)
    m.close()


# ------------------------------------------------------------------------------------------ 4. exact properties
def _flat_call(m, sess, d, v, loss_scale=1. / N, out=None, n=None, first=0):
    torch = sess.torch
    tx, nn = m._as_device_batch(d['x'][first:first + (n or N)])
    hv, _ = m.hess_vecp_device(tx, nn, sess.to_device(d['labels'][first:first + nn], torch.int32),
                               sess.to_device(np.asarray(v, dtype=np.float32), torch.float32), None, loss_scale, out)
    return hv.cpu().numpy()


def test_exact_properties(sess):
    d = case('net3d_skip_c4')
    m = mk(sess, d)
    v = np.concatenate([a.ravel() for a in d['v']])
    base = _flat_call(m, sess, d, v)
    assert np.abs(base).max() > 0
    zero = _flat_call(m, sess, d, np.zeros_like(v))
    assert np.all(zero == 0.0)
    for k in (3, -3):
        np.testing.assert_array_equal(_flat_call(m, sess, d, v * np.float32(2.0 ** k)), base * 2.0 ** k)
    np.testing.assert_array_equal(_flat_call(m, sess, d, v, loss_scale=2. / N), base * 2.0)
    np.testing.assert_array_equal(_flat_call(m, sess, d, v), base)
    w = np.random.RandomState(5).randn(len(v))
    acc = _flat_call(m, sess, d, v, out=sess.to_device(w, sess.torch.float64))
    assert np.all(np.abs(acc - (w + base)) <= np.spacing(np.abs(w + base)))
    m.close()


# ------------------------------------------------------------------------------------------ 5. symmetry
def test_symmetry(sess):
    """u . Hv = v . Hu for the exact Hessian.  Each device product is within test 1's bar of the fp64 one, array by array,
    and the fp64 products are symmetric to fp64 rounding, so |u . Hv - v . Hu| <= sum over arrays of bar(Hv) |u|_1 + bar(Hu) |v|_1."""
    d = case('net3d_skip_c4')
    rs = np.random.RandomState(31)
    u = [rs.randn(*a.shape).astype(np.float32) for a in d['v']]
    v = d['v']
    hu64 = oracle_hv(d['om64'], d['x'], d['labels'], u, d['names'], 1. / N)
    hu32 = oracle_hv(d['om32'], d['x'], d['labels'], u, d['names'], 1. / N)
    bv, bu = bars(d['hv64'], d['hv32']), bars(hu64, hu32)
    m = mk(sess, d)
    hv = m.hess_vecp(d['x'], d['labels'], v)
    hu = m.hess_vecp(d['x'], d['labels'], u)
    lhs = sum((a.astype(np.float64) * b).sum() for a, b in zip(u, hv))
    rhs = sum((a.astype(np.float64) * b).sum() for a, b in zip(v, hu))
    bound = sum(b1 * np.abs(a).sum() + b2 * np.abs(c).sum() for b1, a, b2, c in zip(bv, u, bu, v))
    ref = sum((a.astype(np.float64) * b).sum() for a, b in zip(u, d['hv64']))
    print('symmetry: u.Hv %.9e  v.Hu %.9e  |diff| %.3e  bound %.3e  (fp64 u.Hv %.9e)' % (lhs, rhs, abs(lhs - rhs), bound, ref))
    assert abs(lhs - rhs) <= bound
    m.close()


# ------------------------------------------------------------------------------------------ 6. batch cuts
@pytest.mark.parametrize('name', ['net3d_skip_c4', 'wide_fc_c5'])
def test_batch_cuts(sess, name):
    """5 samples in one call = 2 + 3 samples with `accumulate` and the same loss_scale, and = the host interface on a second
    model of max_batch 2 (passes of 2 + 2 + 1): the per-sample tensors of the product do not depend on the batch and every sum
    over samples and voxels is fp64 in a fixed order, so the sides differ by fp64 rounding of the sums only: <= 1e-12 of the
    array's maximum."""
    d = case(name)
    bar = bars(d['hv64'], d['hv32'])
    m = mk(sess, d)
    v = np.concatenate([a.ravel() for a in d['v']])
    one = _flat_call(m, sess, d, v)
    acc = sess.torch.zeros((len(v),), dtype=sess.torch.float64, device=sess.device)
    _flat_call(m, sess, d, v, out=acc, n=2, first=0)
    cut = _flat_call(m, sess, d, v, out=acc, n=3, first=2)
    m2 = mk(sess, d, max_batch=2)
    host = m2.hess_vecp(d['x'], d['labels'], d['v'])
    for k, (a, b, c, br) in enumerate(zip(m.unflatten(one), m.unflatten(cut), host, bar)):
        print('%s array %d: |one - cut| %.3e  |one - model of max_batch 2| %.3e  bar %.3e  max %.3e'
              % (name, k, np.abs(a - b).max(), np.abs(a - c).max(), br, np.abs(a).max()))
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), (name, k)
        assert np.abs(a - c).max() <= 1e-12 * np.abs(a).max(), (name, k)
    m.close()
    m2.close()


# ------------------------------------------------------------------------------------------ 7. arguments
def test_arguments(sess):
    d = case('neta_c3')
    m = mk(sess, d, max_batch=8)
    torch = sess.torch
    tx, _ = m._as_device_batch(d['x'])
    lab = sess.to_device(d['labels'], torch.int32)
    v = sess.to_device(np.concatenate([a.ravel() for a in d['v']]), torch.float32)
    hv = sess.empty((m.num_params,), torch.float64)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    f = sess.lib.alq_hess_vecp
    EINVAL = -1
    sess.bind_stream()
    assert f(m._m, p(tx), 9, p(lab), 0.2, p(v), None, 0, p(hv), None) == EINVAL
    assert f(m._m, p(tx), 0, p(lab), 0.2, p(v), None, 0, p(hv), None) == EINVAL
    assert f(m._m, p(tx), -1, p(lab), 0.2, p(v), None, 0, p(hv), None) == EINVAL
    assert f(m._m, p(tx), N, p(lab), 0.2, None, None, 0, p(hv), None) == EINVAL
    assert f(m._m, p(tx), N, p(lab), 0.2, p(v), None, 0, None, None) == EINVAL
    assert f(m._m, p(tx), N, None, 0.2, p(v), None, 0, p(hv), None) == EINVAL
    assert f(m._m, None, N, p(lab), 0.2, p(v), None, 0, p(hv), None) == EINVAL
    # a label outside [0, c) contributes nothing: the batch without that sample, same loss_scale
    bad = d['labels'].copy()
    bad[2] = d['c']
    keep = [0, 1, 3, 4]
    with_bad, loss_bad = m.hess_vecp_device(tx, N, sess.to_device(bad, torch.int32), v, None, 0.2, want_loss=True)
    tk, _ = m._as_device_batch(d['x'][keep])
    without, loss_wo = m.hess_vecp_device(tk, 4, sess.to_device(d['labels'][keep], torch.int32), v, None, 0.2, want_loss=True)
    a, b = with_bad.cpu().numpy(), without.cpu().numpy()
    for x1, x2 in zip(m.unflatten(a), m.unflatten(b)):
        assert np.abs(x1 - x2).max() <= 1e-12 * np.abs(x2).max()
    assert abs(float(loss_bad.item()) - float(loss_wo.item())) <= 1e-12 * abs(float(loss_wo.item()))
    # the scaled loss of the call against the fp64 oracle (posteriors to 2e-5, the bar of the smoke run)
    y = np.zeros((d['c'], 4))
    y[d['labels'][keep], np.arange(4)] = 1
    l64, _ = d['om64'].loss_and_grads(d['x'][keep], y)
    p64 = d['om64'].forward(d['x'][keep])['posteriors'][d['labels'][keep], np.arange(4)]
    assert abs(float(loss_wo.item()) - 0.2 * 4 * l64) <= 0.2 * np.sum(2e-5 / p64)
    m.close()


# ------------------------------------------------------------------------------------------ 8. the Python interface
def _pw_setup(sess, seed=41, n_inds=7):
    """A two-modality volume, a binary mask, a small two-class patch-wise net (NN.CNN schema) on 5 x 5 x 1 patches."""
    import torch
    from nnal_amd import NN
    rs = np.random.RandomState(seed)
    shape, patch_shape = (9, 10, 3), (5, 5, 1)
    imgs = [rs.randn(*shape) * 2. + 1., rs.randn(*shape) + 3.]
    r = [2, 2, 0]
    padded = [np.pad(v, [(r[0], r[0]), (r[1], r[1]), (r[2], r[2])], 'constant') for v in imgs]
    mask = (rs.rand(*shape) > 0.5).astype(np.float64)
    stats = [[1., 2.], [3., 1.]]
    ld = OrderedDict([('conv1', [4, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [6, 'fc']), ('fc2', [2, 'fc'])])
    in_shape = (5, 5, 2)
    pars = netspec.he_init(ld, in_shape, seed=seed + 1, bias_std=0.05)
    model = NN.CNN(in_shape, ld, 'pw', sess=sess, max_batch=64)
    model.set_weights(pars)
    # interior voxels: a patch that reaches into the zero padding holds runs of one constant, i.e. exact pool ties
    interior = np.ravel_multi_index(np.meshgrid(np.arange(2, shape[0] - 2), np.arange(2, shape[1] - 2), np.arange(shape[2]),
                                                indexing='ij'), shape).ravel()
    inds = rs.choice(interior, size=n_inds, replace=False)
    om64 = OracleModel(ld, in_shape, pars, dtype=torch.float64)
    om32 = OracleModel(ld, in_shape, pars)
    return dict(model=model, padded=padded, mask=mask, stats=stats, patch_shape=patch_shape, inds=inds, om64=om64, om32=om32,
                names=list(pars.keys()), pars=pars, shape=shape)


def _pw_patches(sess, s, inds):
    from nnal_amd import patch_utils
    vols = patch_utils.DeviceVolumes(sess, s['padded'])
    x = vols.gather(inds, s['patch_shape'], np.asarray(s['stats'], dtype=np.float64), quirk=1).cpu().numpy()
    lab = s['mask'][np.unravel_index(inds, s['shape'])].astype(np.int32)
    return x, lab


def test_python_interface(sess):
    from nnal_amd import Influence, PW_NN
    s = _pw_setup(sess)
    model, names = s['model'], s['names']
    Influence.get_hess_vec_product(model, 'all')
    rs = np.random.RandomState(43)
    v = [rs.randn(*[dm.value for dm in h.shape]).astype(np.float32) for h in model.v_placeholder]
    x, lab = _pw_patches(sess, s, s['inds'])
    hot = np.zeros((2, len(lab)))
    hot[lab, np.arange(len(lab))] = 1
    # sess.run == DeviceModel.hess_vecp
    feed = {model.x: x, model.y_: hot, model.keep_prob: 1.}
    feed.update({h: a for h, a in zip(model.v_placeholder, v)})
    got = sess.run(model.hess_vecp, feed)
    ref = model.hess_vecp(x, lab, v)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    # batch_eval: the LAST batch's product (3 + 3 + 1 voxels)
    xfd = {h: a for h, a in zip(model.v_placeholder, v)}
    be = PW_NN.batch_eval(model, sess, s['padded'], s['inds'], s['patch_shape'], 3, s['stats'], 'hess_vecp', s['mask'], xfd)[0]
    last = model.hess_vecp(x[6:], lab[6:], v)
    for a, b in zip(be, last):
        np.testing.assert_array_equal(a, b)
    assert any(np.abs(a - b).max() > 0 for a, b in zip(be, ref))
    # 'loss': each batch's mean CE in that batch's entries, against the fp64 oracle (posteriors to 2e-5: |d log p| <= 2e-5 / p)
    loss = PW_NN.batch_eval(model, sess, s['padded'], s['inds'], s['patch_shape'], 3, s['stats'], 'loss', s['mask'])[0]
    assert loss.shape == (7,)
    for a, b in ((0, 3), (3, 6), (6, 7)):
        l64, _ = s['om64'].loss_and_grads(x[a:b], hot[:, a:b])
        py = s['om64'].forward(x[a:b])['posteriors'][lab[a:b], np.arange(b - a)]
        assert np.all(loss[a:b] == loss[a]) and abs(loss[a] - l64) <= np.mean(2e-5 / py), (a, loss[a:b], l64)
    assert abs(sess.run(model.loss, {model.x: x[:3], model.y_: hot[:, :3]}) - loss[0]) == 0
    # whole_set: the product of the mean loss over all indices, to test 1's bar
    ws = PW_NN.batch_eval(model, sess, s['padded'], s['inds'], s['patch_shape'], 3, s['stats'], 'hess_vecp', s['mask'], xfd,
                          _whole_set=True)[0]
    assert fragile_units(s['om64'], x) == 0
    h64 = oracle_hv(s['om64'], x, lab, v, names, 1. / 7)
    h32 = oracle_hv(s['om32'], x, lab, v, names, 1. / 7)
    for k, (a, a64, b) in enumerate(zip(ws, h64, bars(h64, h32))):
        e = np.abs(a - a64).max()
        print('whole_set array %d: e(device) %.3e  bar %.3e' % (k, e, b))
        assert e <= b, (k, e, b)
    model.close()


# ------------------------------------------------------------------------------------------ 9. influence, end to end
def test_influence_end_to_end(sess):
    """40 training voxels, one query voxel, the last fc layer's parameters: PW_sample_influence(whole_set=True) returns t with
    |H t - g| below its value at the start point t0 = g, H applied by the fp64 oracle; the solve went through the device."""
    from nnal_amd import Influence
    s = _pw_setup(sess, seed=51, n_inds=41)
    model, names = s['model'], s['names']
    tr_inds, q_ind = s['inds'][:40], s['inds'][40]
    layers = [names[-1]]
    calls = [0]
    real = model.hess_vecp_device

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    model.hess_vecp_device = counted
    t = Influence.PW_sample_influence(model, sess, s['padded'], s['mask'], tr_inds, s['stats'], s['padded'], s['mask'], q_ind,
                                      s['stats'], s['patch_shape'], 16, layers=layers, whole_set=True)
    assert calls[0] >= 3      # at least one product = 3 batches of 16 / 16 / 8 voxels
    x, lab = _pw_patches(sess, s, tr_inds)
    xq, labq = _pw_patches(sess, s, np.asarray([q_ind]))
    hotq = np.zeros((2, 1))
    hotq[labq[0], 0] = 1
    _, g_all = s['om64'].loss_and_grads(xq, hotq)
    g = np.concatenate([a.ravel() for a in g_all[-2:]])

    def H(vec):
        vl = Influence.unravel_vec(model, vec)
        return np.concatenate([a.ravel() for a in oracle_hv(s['om64'], x, lab, vl, layers, 1. / 40)])
    r0, r1 = np.linalg.norm(H(g) - g), np.linalg.norm(H(t) - g)
    print('influence: |H t0 - g| %.6e -> |H t - g| %.6e after %d device calls' % (r0, r1, calls[0]))
    assert np.all(np.isfinite(t)) and r1 < r0
    model.close()
