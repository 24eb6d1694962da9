"""The last-layer closed forms and the stochastic influence recursion on the device (csrc/llfc.hip): the kernels through the C ABI
against the float64 restatement (tests/llfc_ref.py) on the same fp32 inputs, and NN.LLFC_grads / NN.LLFC_hess /
PW_NNAL.stoch_approx_IF end to end against tests/golden/llfc.npz, the reference's own outputs (GPU box).

Bounds.  V is fp32 on chip: the asserted bound on max|V_dev - V_ref| / max|V_ref| is four times the largest value measured on
the MI355X over the cases below (MEASURED_*, the margin for other summation orders) and never above (T + 2) * 2^-22: one
rounding of 2^-24 per element and iteration plus those of V_0, times the same four.  End to end the cap is 1e-4 of max|V|, the
project's score tolerance carried through 25 contracting iterations."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import llfc_ref  # noqa: E402

SCALE = 50.
# largest max|V_dev - V_ref| / max|V_ref| measured over the kernel-level cases, per iteration count T (MI355X)
MEASURED_KERNEL = {0: 5.7e-8, 1: 6.1e-8, 40: 2.42e-7}
# largest error against the golden over both nets, relative to the largest entry of the reference's output (MI355X)
MEASURED_E2E = {'grads': 4.95e-7, 'hess': 1.32e-7, 'V': 5.58e-7}
E2E_CAP = 1e-4


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(c, d, n_pool, n_tr, seed):
    """fp32 features with |u~|^2 <= scale / 2 and soft-max posteriors, [n, d] / [c, n] like alq_forward's outputs."""
    rs = np.random.RandomState(seed)

    def one(n):
        U = rs.randn(n, d)
        U *= np.sqrt(0.45 * SCALE) / np.sqrt((U ** 2).sum(1, keepdims=True))
        Z = rs.randn(c, n)
        Pm = np.exp(Z) / np.exp(Z).sum(0)
        return U.astype(np.float32), Pm.astype(np.float32)
    Up, Pp = one(n_pool)
    Ut, Pt = one(n_tr)
    lab = rs.randint(0, c, size=n_pool).astype(np.int32)
    return Up, Pp, lab, Ut, Pt


def _stoch_if(sess, Up, Pp, lab, Ut, Pt, draws, path):
    from nnal_amd._lib import check
    torch = sess.torch
    sess.bind_stream()
    n_pool, d = Up.shape
    c, n_tr, T = Pp.shape[0], Ut.shape[0], len(draws)
    t = [sess.to_device(a, dt) for a, dt in ((Up, torch.float32), (Pp, torch.float32), (lab, torch.int32), (Ut, torch.float32),
                                             (Pt, torch.float32), (np.asarray(draws, dtype=np.int32).reshape(-1), torch.int32))]
    V = torch.full((n_pool, (d + 1) * c), float('nan'), dtype=torch.float32, device=sess.device)
    work = sess.empty((max(int(sess.lib.alq_llfc_if_work_bytes(n_pool, c)), 8),), torch.uint8)
    check(sess.lib.alq_llfc_stoch_if(sess.ctx, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), n_pool, _ptr(t[3]), _ptr(t[4]), n_tr,
                                     _ptr(t[5]) if T else None, T, SCALE, d, c, path, _ptr(V), _ptr(work)))
    return V.cpu().numpy()


def _draws(T, n_tr):
    return [(7 * t * t + 2) % n_tr for t in range(T)] if T != 1 else [n_tr - 1]      # T = 40: every index repeats


def _check_case(sess, c, d, n_pool, T, n_tr, paths, worst):
    Up, Pp, lab, Ut, Pt = _inputs(c, d, n_pool, n_tr, seed=1000 * c + d + n_pool + T)
    draws = _draws(T, n_tr)
    ref = llfc_ref.stoch_if(Up.T, Pp, lab, Ut.T, Pt, draws, SCALE).T
    bound = min(4 * MEASURED_KERNEL[T], (T + 2) * 2. ** -22)
    outs = []
    for path in paths:
        V = _stoch_if(sess, Up, Pp, lab, Ut, Pt, draws, path)
        err = np.abs(V - ref).max() / np.abs(ref).max()
        print('c=%d d=%d n_pool=%d T=%d n_tr=%d path=%d: err %.3e (bound %.3e)' % (c, d, n_pool, T, n_tr, path, err, bound))
        worst[T] = max(worst.get(T, 0.), err)
        outs.append(V)
    for V in outs:
        assert np.isfinite(V).all()
        assert np.abs(V - ref).max() / np.abs(ref).max() <= bound
    if len(outs) == 2:
        np.testing.assert_array_equal(outs[0], outs[1])      # one element-to-thread map, one summation tree


@pytest.mark.parametrize('c,d', [(2, 1), (2, 37), (3, 130), (2, 4096)])
def test_stoch_if_kernels_vs_float64(sess, c, d):
    """Both paths on every case: n_pool 1, 5 and 67 (5 and 67 are no multiples of the 4 columns of a resident workgroup; 67 < the CU
    count gives one column per workgroup), T 0, 1 and 40 with repeated draws; n_tr = 1 rides on n_pool = 5."""
    assert sess.lib.alq_llfc_if_path(d, c) == 1
    worst = {}
    for n_pool in (1, 5, 67):
        for T in (0, 1, 40):
            _check_case(sess, c, d, n_pool, T, 1 if n_pool == 5 else 3, (1, 2), worst)
    print('largest error per T:', worst)


def test_stoch_if_more_columns_than_cus(sess):
    """1030 columns: four per resident workgroup, the last workgroup with two."""
    worst = {}
    _check_case(sess, 2, 37, 1030, 40, 3, (1, 2), worst)


def test_stoch_if_streaming_only(sess):
    """Five classes: the resident kernel refuses, automatic choice and path 2 stream (4-byte accesses: d odd)."""
    from nnal_amd._lib import AlqError
    c, d = 5, 33
    assert sess.lib.alq_llfc_if_path(d, c) == 2
    worst = {}
    for T in (0, 1, 40):
        _check_case(sess, c, d, 5, T, 3, (0, 2), worst)
    Up, Pp, lab, Ut, Pt = _inputs(c, d, 5, 3, seed=3)
    with pytest.raises(AlqError):
        _stoch_if(sess, Up, Pp, lab, Ut, Pt, [0], 1)


def test_stoch_if_bit_identical_runs(sess):
    Up, Pp, lab, Ut, Pt = _inputs(2, 4096, 67, 3, seed=11)
    for path in (1, 2):
        a = _stoch_if(sess, Up, Pp, lab, Ut, Pt, _draws(40, 3), path)
        b = _stoch_if(sess, Up, Pp, lab, Ut, Pt, _draws(40, 3), path)
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('c,d,n', [(2, 1, 1), (2, 37, 5), (3, 130, 67), (2, 4096, 5)])
def test_grads_kernel_vs_fp32_restatement(sess, c, d, n):
    from nnal_amd._lib import check
    torch = sess.torch
    sess.bind_stream()
    U, Pm, lab, _, _ = _inputs(c, d, n, 1, seed=d)
    E = -Pm.copy()
    for j in range(c):
        E[j] = (lab == j).astype(np.float32) - Pm[j]
    ref = np.concatenate([(E[:, None, :] * U.T[None, :, :]).reshape(c * d, n), E], 0).T
    assert ref.dtype == np.float32
    tU, tP, tl = sess.to_device(U, torch.float32), sess.to_device(Pm, torch.float32), sess.to_device(lab, torch.int32)
    out = torch.full((n, (d + 1) * c), float('nan'), dtype=torch.float32, device=sess.device)
    check(sess.lib.alq_llfc_grads(sess.ctx, _ptr(tU), _ptr(tP), _ptr(tl), n, d, c, _ptr(out)))
    out = out.cpu().numpy()
    ulp = np.spacing(np.abs(ref).max(1, keepdims=True))
    print('c=%d d=%d n=%d: max |dev - fp32 restatement| / ulp(row max) = %.2f' % (c, d, n, (np.abs(out - ref) / ulp).max()))
    assert (np.abs(out - ref) <= ulp).all()
    assert np.abs(out.astype(np.float64) - llfc_ref.llfc_grads(U.T, Pm, lab).T).max() <= 2. ** -22 * np.abs(ref).max()


@pytest.mark.parametrize('c,d', [(2, 37), (3, 5)])
def test_hess_kernel(sess, c, d):
    from nnal_amd._lib import check
    torch = sess.torch
    sess.bind_stream()
    U, Pm, _, _, _ = _inputs(c, d, 1, 1, seed=17 + d)
    P = (d + 1) * c
    H = torch.full((P, P), float('nan'), dtype=torch.float64, device=sess.device)
    tu, tp = sess.to_device(U[0], torch.float32), sess.to_device(Pm[:, 0], torch.float32)
    check(sess.lib.alq_llfc_hess(sess.ctx, _ptr(tu), _ptr(tp), d, c, _ptr(H)))
    H = H.cpu().numpy()
    ref = llfc_ref.llfc_hess(U[0], Pm[:, 0])
    np.testing.assert_array_equal(H, H.T)
    ut = np.append(U[0].astype(np.float64), 1.)
    A = llfc_ref.llfc_A(Pm[:, 0])
    rows = np.concatenate([(A.sum(1)[:, None] * U[0].astype(np.float64)[None, :]).reshape(-1), A.sum(1)]) * ut.sum()
    print('c=%d d=%d: max |H - ref| / max|ref| = %.2e' % (c, d, np.abs(H - ref).max() / np.abs(ref).max()))
    assert np.abs(H.sum(1) - rows).max() <= 1e-12 * np.abs(ref).max() * P
    assert np.abs(H - ref).max() <= 1e-12 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------ end to end on the golden nets
_NETS = {
    'pool': OrderedDict([('conv1', [2, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [2, 'fc'])]),
    'fc': OrderedDict([('conv1', [3, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [10, 'fc']), ('fc2', [3, 'fc'])]),
}
_e2e = {}


def _gold(golden_dir, net):
    z = np.load(os.path.join(golden_dir, 'llfc.npz'))
    g = {k[len(net) + 1:]: z[k] for k in z.files if k.startswith(net + '_')}
    g['scale'], g['max_iter'], g['in_shape'] = float(z['scale']), int(z['max_iter']), tuple(int(v) for v in z['in_shape'])
    return g


def _model(sess, g, net, feature_layer=None, ld=None):
    from nnal_amd import NN
    ld = ld or _NETS[net]
    m = NN.CNN(g['in_shape'], ld, net, int(g['feature_layer']) if feature_layer is None else feature_layer, None, [], sess, max_batch=8)
    m.set_weights({n: [g['W_' + n], g['b_' + n]] for n in ld if 'W_' + n in g})
    return m


def _case(sess, golden_dir, net):
    """Per net, computed once and left unchanged: the device's outputs for the golden's inputs."""
    if net not in _e2e:
        from nnal_amd import NN, PW_NNAL
        g = _gold(golden_dir, net)
        m = _model(sess, g, net)
        fd = {m.x: g['pool_x'], m.keep_prob: 1.}
        o = dict(g=g)
        o['G_given'] = NN.LLFC_grads(m, sess, fd, g['labels'])
        o['G_pred'], o['pred'] = NN.LLFC_grads(m, sess, fd)
        o['H3'] = NN.LLFC_hess(m, sess, {m.x: g['tr_x'][[3]], m.keep_prob: 1.})
        np.random.seed(int(g['seed']))
        o['V'], o['weak'] = PW_NNAL.stoch_approx_IF(m, sess, g['tr_x'], g['pool_x'], g['max_iter'], g['scale'])
        o['feat'] = sess.run(m.feature_layer, feed_dict=fd)
        o['post'] = sess.run(m.posteriors, feed_dict=fd)
        V1, _ = m.llfc_stoch_if_device(*m._as_device_batch(g['pool_x']), m._as_device_batch(g['tr_x'][[3]])[0], [0], g['scale'])
        o['V1'] = V1.cpu().numpy().astype(np.float64)[:, m.llfc_reference_order()].T
        m.close()
        _e2e[net] = o
    return _e2e[net]


def _e2e_assert(what, dev, ref):
    err = np.abs(dev - ref).max() / np.abs(ref).max()
    bound = min(4 * MEASURED_E2E[what], E2E_CAP)
    print('%s: max |dev - golden| / max|golden| = %.3e (bound %.3e)' % (what, err, bound))
    assert dev.shape == ref.shape and dev.dtype == np.float64
    assert err <= bound


@pytest.mark.parametrize('net', ['pool', 'fc'])
def test_llfc_grads_vs_golden(sess, golden_dir, net):
    o = _case(sess, golden_dir, net)
    np.testing.assert_array_equal(o['pred'], o['g']['pred'])
    _e2e_assert('grads', o['G_given'], o['g']['G_given'])
    _e2e_assert('grads', o['G_pred'], o['g']['G_pred'])


@pytest.mark.parametrize('net', ['pool', 'fc'])
def test_llfc_hess_vs_golden(sess, golden_dir, net):
    o = _case(sess, golden_dir, net)
    np.testing.assert_array_equal(o['H3'], o['H3'].T)
    _e2e_assert('hess', o['H3'], o['g']['H3'])


@pytest.mark.parametrize('net', ['pool', 'fc'])
def test_stoch_approx_IF_vs_golden(sess, golden_dir, net):
    o = _case(sess, golden_dir, net)
    np.testing.assert_array_equal(o['weak'], o['g']['weak'])
    _e2e_assert('V', o['V'], o['g']['V'])


@pytest.mark.parametrize('net', ['pool', 'fc'])
def test_hessian_times_gradient_is_one_update_term(sess, golden_dir, net):
    """T = 1 from V_0 = G: V_1 - 2 G = LLFC_hess(training sample) @ G / scale.  V_1 carries one fp32 rounding of about 2 max|G|
    (2^-23 max|G|) and 2 G two roundings of LLFC_grads' fp32 arithmetic (2^-22 max|G|): 2^-21 max|G| bounds their sum."""
    o = _case(sess, golden_dir, net)
    G = o['G_pred']
    lhs = o['V1'] - 2 * G
    rhs = o['H3'] @ G / o['g']['scale']
    print('%s: max |(V_1 - 2G) - H G / scale| / max|G| = %.3e' % (net, np.abs(lhs - rhs).max() / np.abs(G).max()))
    assert np.abs(lhs - rhs).max() <= 2. ** -21 * np.abs(G).max()


@pytest.mark.parametrize('net', ['pool', 'fc'])
def test_class_sums_of_a_gradient_column(sess, golden_dir, net):
    """sum_i g[j d + i] + g[c d + j] = (sum u + 1) (y_j - p_j); each fp32 entry is within 2^-23 of its own size."""
    o = _case(sess, golden_dir, net)
    G, U, Pm = o['G_given'], o['feat'].astype(np.float64), o['post'].astype(np.float64)
    d, n = U.shape
    c = Pm.shape[0]
    for j in range(c):
        lhs = G[j * d:(j + 1) * d].sum(0) + G[c * d + j]
        rhs = (U.sum(0) + 1.) * ((o['g']['labels'] == j) - Pm[j])
        assert (np.abs(lhs - rhs) <= 2. ** -22 * (np.abs(U).sum(0) + 1.)).all()


def test_pw_llfc_grads_takes_every_samples_own_features(sess, golden_dir, monkeypatch):
    """Two subjects (3 + 4 patches, handed over in place of the gather): the columns are LLFC_grads' of all 7, in subject order -
    not the reference's label term from the last subject's features (NN.py:1015)."""
    from nnal_amd import NN, patch_utils
    g = _gold(golden_dir, 'pool')
    m = _model(sess, g, 'pool')
    monkeypatch.setattr(patch_utils, 'get_patches_multimg', lambda *a, **k: ([g['pool_x'][:3], g['pool_x'][3:]], None))

    class Expr(object):
        pars = {'patch_shape': g['in_shape'][:2]}
        train_stats = None
        nclass = 2
    try:
        out = NN.PW_LLFC_grads(m, sess, Expr(), None, [[0, 1, 2], [0, 1, 2, 3]], g['labels'])
    finally:
        m.close()
    _e2e_assert('grads', out, g['G_given'])


def test_feature_layer_must_feed_the_last_fc(sess, golden_dir):
    from nnal_amd import NN, PW_NNAL
    g = _gold(golden_dir, 'pool')
    m = _model(sess, g, 'pool', feature_layer=0)          # the conv's output: 288 values against fc1's 72 inputs
    fd = {m.x: g['pool_x'], m.keep_prob: 1.}
    try:
        with pytest.raises(ValueError):
            NN.LLFC_grads(m, sess, fd)
        with pytest.raises(ValueError):
            NN.LLFC_hess(m, sess, {m.x: g['pool_x'][[0]], m.keep_prob: 1.})
        with pytest.raises(ValueError):
            PW_NNAL.stoch_approx_IF(m, sess, g['tr_x'], g['pool_x'], 2)
        with pytest.raises(ValueError):
            m.llfc_stoch_if_device(*m._as_device_batch(g['pool_x']), None, [], 50.)
    finally:
        m.close()


def test_llfc_hess_refuses_above_the_byte_cap(sess, golden_dir):
    """(d+1) c = 2897 * 2 = 5794 parameters: 268,563,488 bytes against the cap's 268,435,456 (5792 parameters)."""
    from nnal_amd import NN
    g = _gold(golden_dir, 'pool')
    ld = OrderedDict([('conv1', [2, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [2896, 'fc']), ('fc2', [2, 'fc'])])
    m = NN.CNN(g['in_shape'], ld, 'wide', 2, None, [], sess, max_batch=2)
    try:
        assert ((m.feature_dim + 1) * 2) ** 2 * 8 > sess.lib.alq_llfc_hess_max_bytes() >= (m.feature_dim * 2) ** 2 * 8
        with pytest.raises(ValueError, match='stoch_approx_IF'):
            NN.LLFC_hess(m, sess, {m.x: g['pool_x'][[0]], m.keep_prob: 1.})
    finally:
        m.close()
