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

The product is evaluated in fp64, so beside that fp32 bar every product is held to the fp64 bar of tests/hvp_cases.py,
b64 = 2^-38 x (max over entries of sum_n |H_n v|) per array, on inputs for which tests/test_hvp_cases_host.py proves on the CPU
that the bar lies 64 x above the truth's own fp64 noise, 1024 x below the fp32 oracle's error, and that no decision is fragile
at hvp_cases.EPS_TIGHT = 2e-5.  The oracle, the bar and the table of cases live in tests/hvp_cases.py; tests 10 on run the
cases that exist for one branch of csrc/hvp.hip or of run_hess_vecp (csrc/grads.hip) each.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests import hvp_cases  # noqa: E402
from tests.hvp_cases import EPS, N, bars64, case, fragile_units, hold64, oracle_hv, symmetry_u, yard  # noqa: E402,F401  (other files import them here)


def _hv_nets():
    """(name, layer dict, input shape, skips, weight seed, input seed): the first four cases of tests/hvp_cases.TABLE - the nets
    of test_gpu_lsum._nets() that the first issue named plus a two-class 3-D net (fused two-class head); seeds with no fragile
    unit in fp64 at hvp_cases.EPS_TIGHT."""
    return [(n,) + tuple(hvp_cases.TABLE[n][k] for k in ('ld', 'in_shape', 'sk', 'wseed', 'xseed')) for n in hvp_cases.FOUR_NETS]


_NETS = {n[0]: n for n in _hv_nets()}


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


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
    hold64(name, hv, yard(name), d['arrays'])


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
    y = yard('net3d_skip_c4', chosen)
    hold64(which, got, y, y['arrays'])
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
    """u . Hv = v . Hu for the exact Hessian.  Each device product is within the fp64 bar of the fp64 one, array by array
    (hvp_cases.bars64; the conditions for u as for v are proven in tests/test_hvp_cases_host.py), and the fp64 products are
    symmetric to fp64 rounding, so |u . Hv - v . Hu| <= sum over arrays of b64(Hv) |u|_1 + b64(Hu) |v|_1."""
    d = case('net3d_skip_c4')
    u = symmetry_u(d)
    v = d['v']
    bv, bu = bars64(yard('net3d_skip_c4')), bars64(yard('net3d_skip_c4', v=u, key='u'))
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
    hold64('symmetry Hu', hu, yard('net3d_skip_c4', v=u, key='u'), d['arrays'])


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
    # ... and to the fp64 bar.  The patches come out of the device gather, so its three conditions are asserted here, on the CPU
    y = hvp_cases.yardsticks(s['om64'], s['om32'], x, lab, v, names, 1. / 7, h64, h32)
    hvp_cases.figures('whole_set', y)
    assert hvp_cases.conditions(y, s['om64'], x) == []
    hold64('whole_set', [np.asarray(a) for a in ws], y)
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


# ------------------------------------------------------------------------------------------ 10. one case per branch (tests/hvp_cases.TABLE)
# Every case: N = 5 under max_batch = 8 unless its row says otherwise, weights he_init(bias_std=0.05), the product under the fp64
# bar; what a case claims about the net or the launch is asserted on the host from the layer table or the rule restated in
# hvp_cases (tests/test_hvp_cases_host.py repeats those claims where no device is needed).
def _held(sess, name, m=None):
    """The whole product of a case on a fresh model (or on m), held to the fp64 bar; (the product, the flat device result)."""
    d = case(name)
    own = m is None
    if own:
        m = mk(sess, d, max_batch=hvp_cases.MAX_BATCH)
    hv = m.hess_vecp(d['x'], d['labels'], d['v'])
    if own:
        m.close()
    assert len(hv) == 2 * len(d['names'])
    hold64(name, hv, yard(name), d['arrays'])
    return hv


def _layers_of(name):
    from nnal_amd.device_host import translate_layers
    d = case(name)
    return translate_layers(d['ld'], d['in_shape'], d['sk'])


@pytest.mark.parametrize('name', ['pool_route', 'pool_w3'])
def test_pool_routing(sess, name):
    """hvp_pool_fwd_kernel / hvp_pool_bwd_kernel: non-cubic windows (1, 2, 2) then (2, 2, 1) whose last window overhangs the
    volume (pool_route), and a window 3 whose padding starts in front of it, lo = 1 on every axis (pool_w3)."""
    from oracle import tfops
    from nnal_amd._lib import ALQ_POOL
    pools = [ly for ly in _layers_of(name) if ly['type'] == ALQ_POOL]
    size = list(case(name)['in_shape'][:-1])
    pads = []
    for ly in pools:
        pads.append([tfops.same_pads(n, k, k)[1:] for n, k in zip(size, ly['k'])])
        size = [-(-n // k) for n, k in zip(size, ly['k'])]
    if name == 'pool_route':
        assert [ly['k'] for ly in pools] == [[1, 2, 2], [2, 2, 1]]
        assert pads == [[(0, 0), (0, 1), (0, 0)], [(0, 1), (0, 0), (0, 0)]]      # H = 7 and then D = 5 end in half a window
    else:
        assert [ly['k'] for ly in pools] == [[3, 3, 3]] and pads == [[(1, 1), (1, 1), (1, 1)]]
    _held(sess, name)


@pytest.mark.parametrize('what', ['first', 'behind a concat'])
def test_pool_refusal(sess, what):
    """hvp_prepare's refusal of a pool layer that reads the network input or a concat, with its message."""
    from nnal_amd import device
    from nnal_amd._lib import AlqError
    if what == 'first':
        ld, sk = OrderedDict([('pool1', ['pool', [2, 2]]), ('conv1', ['conv', [4, [3, 3]], 'MA']), ('fc', ['fc', [2]])]), ()
    else:
        ld = OrderedDict([('conv1', ['conv', [4, [3, 3]], 'MA']), ('conv2', ['conv', [4, [3, 3]], 'MA']), ('pool1', ['pool', [2, 2]]),
                          ('fc', ['fc', [2]])])
        sk = [[0, [2], 'con']]
    in_shape = (6, 6, 1)
    pars = netspec.he_init(ld, in_shape, seed=91, skips=sk, bias_std=0.05)
    m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=4)
    m.set_weights(pars)
    rs = np.random.RandomState(92)
    v = [rs.randn(*np.asarray(a).shape).astype(np.float32) for nme in pars for a in pars[nme]]
    with pytest.raises(AlqError) as ei:
        m.hess_vecp(rs.randn(3, *in_shape).astype(np.float32), np.zeros(3, np.int32), v)
    print('refused: %s' % ei.value)
    assert str(ei.value).endswith('alq_hess_vecp: pool layer first or behind a concat')
    m.close()


def test_layers_without_relu(sess):
    """The `mask` off branches: HSrc() as mask in hvp_contract_kernel and hvp_fc_fwd_kernel and no k_hvp_mask on the way back, for a
    conv and an fc layer without ReLU between ReLU layers."""
    from nnal_amd._lib import ALQ_CONV, ALQ_FC
    assert [(ly['type'], ly['relu']) for ly in _layers_of('no_relu')] == [(ALQ_CONV, 1), (ALQ_CONV, 0), (ALQ_CONV, 1), (ALQ_FC, 1), (ALQ_FC, 0),
                                                                        (ALQ_FC, 1), (ALQ_FC, 0)]
    _held(sess, 'no_relu')


def test_fc_flatten_order(sess):
    """hvp_ftf in hvp_fc_fwd / hvp_fc_bwd / hvp_fc_wgrad: the first fc reads an activation with D, H, W, C = 3, 4, 5, 2 all different,
    the second reads (1, 1, 1, F)."""
    d = case('fc_geom')
    assert d['in_shape'][:-1] == (3, 4, 5) and d['pars']['conv1'][0].shape[-1] == 2
    assert [d['pars'][n][0].shape for n in ('fc1', 'fc2', 'fc3')] == [(7, 3 * 4 * 5 * 2), (6, 7), (4, 6)]
    _held(sess, 'fc_geom')


def test_wide_fc_weight_sources(sess, monkeypatch):
    """The TF-layout copy of a wide fc layer's weights: unpermuted on the device from the resident copy of a layer packed there
    (hvp_unpermute_kernel, D, H, W, C = 2, 4, 8, 12), or uploaded from the host arrays of a layer set through the host.  Same bits."""
    d = case('fc_wide')
    assert d['pars']['fc1'][0].shape == (256, 2 * 4 * 8 * 12)
    t = d['names'].index('fc1')
    m = mk(sess, d, max_batch=hvp_cases.MAX_BATCH)
    assert sess.lib.alq_model_layer_packs_on_device(m._m, t) == 1 and not m._host_repack and m._dev_w[t] is not None
    dev = _held(sess, 'fc_wide', m)
    m.close()
    monkeypatch.setenv('ALQ_HOST_REPACK', '1')
    mh = mk(sess, d, max_batch=hvp_cases.MAX_BATCH)
    monkeypatch.delenv('ALQ_HOST_REPACK')
    assert mh._host_repack and mh._dev_w[t] is None
    host = _held(sess, 'fc_wide', mh)
    mh.close()
    for a, b in zip(dev, host):
        np.testing.assert_array_equal(a, b)


def _subset_call(sess, m, d, chosen, loss_scale):
    """H v over the layers `chosen` through the flat interface, every other layer's entries of v NaN; the chosen layers' arrays."""
    torch = sess.torch
    names = d['names']
    vs = sub(d['v'], names, chosen)
    idx = m.hess_layer_idx(chosen)
    full = np.full(m.num_params, np.nan, dtype=np.float32)
    offs = m._param_offsets()
    for t, (vw, vb) in zip(idx, zip(vs[0::2], vs[1::2])):
        o, nw, nb = offs[t]
        full[o:o + nw] = vw.ravel()
        full[o + nw:o + nw + nb] = vb.ravel()
    tx, n = m._as_device_batch(d['x'])
    out, _ = m.hess_vecp_device(tx, n, sess.to_device(d['labels'], torch.int32), sess.to_device(full, torch.float32), idx, loss_scale)
    flat = out.cpu().numpy()
    assert np.all(np.isfinite(flat))
    for t in range(m.L):
        if t not in idx:
            o, nw, nb = offs[t]
            assert np.all(flat[o:o + nw + nb] == 0.0), t
    return m.unflatten(flat, idx)


_SUBSETS = [('only %d' % t, 'only', t) for t in range(5)] + [('all but %d' % t, 'but', t) for t in range(5)]


@pytest.mark.parametrize('kind,t', [s[1:] for s in _SUBSETS], ids=[s[0] for s in _SUBSETS])
def test_switched_off_terms(sess, kind, t):
    """The null-source and null-V branches: every layer of net3d_skip_c4 alone and all but layer t, the off layers' entries of v
    NaN.  Each weight and bias product kernel alone per layer type; the skipped s1 term of hvp_contract_kernel; V == nullptr in
    hvp_fc_bwd_kernel; hs_on(Ra) false in hvp_wgrad_kernel for the first layer alone (no tangent reaches it)."""
    d = case('net3d_skip_c4')
    names = d['names']
    assert len(names) == 5
    chosen = [names[t]] if kind == 'only' else [nme for nme in names if nme != names[t]]
    assert chosen in hvp_cases.subsets('net3d_skip_c4')
    m = mk(sess, d)
    got = _subset_call(sess, m, d, chosen, 1. / N)
    m.close()
    y = yard('net3d_skip_c4', chosen)
    hold64('%s %d' % (kind, t), got, y, y['arrays'])


@pytest.mark.parametrize('name', ['labels_c2', 'labels_c21'])
def test_unlabelled_rows(sess, name):
    """The zero rows of hvp_softmax64_kernel and hvp_softmax2_kernel: labels -1 and c mixed among valid ones, against the same
    samples with the unlabelled ones removed (same loss_scale): the products within b64 of each other, each within b64 of the
    truth, the losses equal to 1e-12 relative.  c = 2 (fused two-class head) and c = 21."""
    d = case(name)
    c, n = d['c'], d['n']
    assert sorted(set(d['labels'].tolist()) - set(range(c))) == [-1, c] and n == 7
    keep, ykeep = hvp_cases.labelled_only(name)
    assert len(keep) == 4
    torch = sess.torch
    m = mk(sess, d, max_batch=hvp_cases.MAX_BATCH)
    v = sess.to_device(np.concatenate([a.ravel() for a in d['v']]), torch.float32)
    tx, _ = m._as_device_batch(d['x'])
    mixed, loss_mixed = m.hess_vecp_device(tx, n, sess.to_device(d['labels'], torch.int32), v, None, 1. / n, want_loss=True)
    tk, _ = m._as_device_batch(d['x'][keep])
    alone, loss_alone = m.hess_vecp_device(tk, len(keep), sess.to_device(d['labels'][keep], torch.int32), v, None, 1. / n, want_loss=True)
    a, b = m.unflatten(mixed.cpu().numpy()), m.unflatten(alone.cpu().numpy())
    lm, la = float(loss_mixed.item()), float(loss_alone.item())
    m.close()
    hold64(name + ' mixed', a, yard(name), d['arrays'])
    hold64(name + ' labelled only', b, ykeep, d['arrays'])
    for arr, x1, x2, bar in zip(d['arrays'], a, b, bars64(ykeep)):
        e = np.abs(x1 - x2).max()
        print('%s %s: |mixed - labelled only| %.3e  b64 %.3e' % (name, arr, e, bar))
        assert e <= bar, (name, arr, e, bar)
    print('%s: loss %.17g against %.17g' % (name, lm, la))
    assert la > 0 and abs(lm - la) <= 1e-12 * abs(la)


def test_wgrad_slab_cap(sess):
    """hvp_wgrad_kernel where the partial buffer's cap 2^22 / M sets the slab count: the 5x5 conv 64 -> 64 on 46 x 46, N = 5:
    M = 102,400, cap 40 below rows / 256 = 41; 265 rows per slab against 2,116 per sample, the last slab 245 rows."""
    prod = {p[0]: p[1:] for p in hvp_cases.conv_products('slab_cap')}
    assert prod['conv2'] == (10580, 2116, 102400, 40, 265, 'cap') and 10580 // 256 == 41 and 10580 - 39 * 265 == 245
    assert prod['conv1'][3:] == (41, 259, 'rows')
    _held(sess, 'slab_cap')


def test_one_sample(sess):
    """N = 1, and rows < 256 in hvp_wgrad_kernel: one slab."""
    assert hvp_cases.conv_products('one_sample') == [('conv1', 210, 210, 216, 1, 210, 'rows')] and case('one_sample')['n'] == 1
    _held(sess, 'one_sample')


def test_full_batch(sess):
    """N = max_batch."""
    assert case('full_batch')['n'] == hvp_cases.MAX_BATCH == 8
    _held(sess, 'full_batch')


@pytest.mark.parametrize('name', ['net3d_skip_c4', 'net3d_skip_c2', 'labels_c21'])
def test_constant_logit_shift_is_null(sess, name):
    """The cancellation order of hvp_softmax2_kernel.  A vector that is K on every entry of the head's bias and zero elsewhere moves
    every logit by K, which the softmax does not see: H v = 0.  On the device Rz_nj = K exactly (every product with a zero of v is
    a zero, 0 + K is exact), the kernel sums p_k (Rz_j - Rz_k) = p_k 0, and every array of the product is EXACTLY zero, whatever
    K.  The other order, p_j (Rz_j - sum_k p_k Rz_k), leaves K (1 - sum_k p_k) wherever the fp64 posteriors of a sample do not add
    up to exactly 1.  (The fp64 bar cannot see this: the truth's own evaluation carries the same K x 2^-53.)"""
    d = case(name)
    m = mk(sess, d, max_batch=hvp_cases.MAX_BATCH)
    for K in (1.0, 3.0, 2.0 ** 20):
        v = [np.zeros_like(a) for a in d['v']]
        v[-1] = np.full_like(d['v'][-1], K)
        hv = m.hess_vecp(d['x'], d['labels'], v)
        for arr, a in zip(d['arrays'], hv):
            assert np.all(a == 0.0), (name, K, arr, np.abs(a).max())
    m.close()


def test_accumulate_three_calls(sess):
    """1 + 3 + 1 samples in three calls with `accumulate` against one call of 5: within 1e-12 of the array's maximum (fp64
    rounding of the sums, as in test_batch_cuts), and the accumulated product under the fp64 bar."""
    d = case('net3d_skip_c4')
    m = mk(sess, d)
    v = np.concatenate([a.ravel() for a in d['v']])
    one = _flat_call(m, sess, d, v)
    acc = sess.torch.zeros((len(v),), dtype=sess.torch.float64, device=sess.device)
    for first, n in ((0, 1), (1, 3), (4, 1)):
        cut = _flat_call(m, sess, d, v, out=acc, n=n, first=first)
    got = m.unflatten(cut)
    for k, (a, b) in enumerate(zip(m.unflatten(one), got)):
        print('array %d: |one - 1 + 3 + 1| %.3e  max %.3e' % (k, np.abs(a - b).max(), np.abs(a).max()))
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), k
    m.close()
    hold64('1 + 3 + 1', got, yard('net3d_skip_c4'), d['arrays'])
