"""Per-class layer sums without parameter-sized rows (alq_class_layer_sums, csrc/lsum.hip) and the multi-class Fisher query
on top of them, against the fp64 oracle and against the rows arm (alq_param_grads + alq_shrink_sum) (GPU box)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import alpath, netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests.test_gpu_parity import (G_RTOL, SCORE_ATOL, _load, assert_scores_close,  # noqa: E402
                                   build_fisher_model)
from tests.test_r3_goldens import _imgfi_case  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def net_3d_skip(nclass):
    """A small 3-D net with a 'con' skip and a conv_transpose (NN_extended schema)."""
    k3, s2 = [3, 3, 3], [2, 2, 2]
    layers = OrderedDict([
        ('enc1', ['conv', [8, k3], 'MA']),
        ('pool1', ['pool', s2]),
        ('enc2', ['conv', [16, k3], 'MA']),
        ('up1', ['conv_transpose', [8, k3, s2], 'M']),
        ('dec1', ['conv', [8, k3], 'MA']),
        ('fc', ['fc', [nclass]]),
    ])
    return layers, [[0, [4], 'con']]


def net_wide_fc(nclass):
    """One wide fc layer (256 x 256) behind a conv + pool on 8 x 8 inputs."""
    return OrderedDict([('conv1', [16, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [256, 'fc']), ('fc2', [nclass, 'fc'])])


def _nets():
    ld3, sk3 = net_3d_skip(4)
    # (name, layer dict, input shape, skips, weight seed, input seed): seeds for which neither the fp32 oracle (checked in
    # the test, on the CPU) nor the rows arm leaves a sample out of the metric
    return [('neta_c3', netspec.net_a(nclass=3), (20, 20, 1), (), 71, 17),
            ('neta_c12', netspec.net_a(nclass=12), (20, 20, 1), (), 72, 18),
            ('net3d_skip_c4', ld3, (8, 8, 8, 1), sk3, 73, 19),
            ('wide_fc_c5', net_wide_fc(5), (8, 8, 1), (), 74, 20)]


def _mk(sess, ld, in_shape, sk, seed, max_batch=16):
    from nnal_amd import device
    pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
    m.set_weights(pars)
    return m, pars


def _dev(sess, x):
    return sess.to_device(np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1), sess.torch.float32)


def _sums(m, sess, x, classes):
    return m.class_layer_sums_device(_dev(sess, x), len(x), classes).cpu().numpy()


def _misses_gradient_bar(dev, ref, rtol=2e-4):
    """The bar of test_gpu_train.test_full_log_posterior_gradients_vs_oracle (_close) as a predicate."""
    for a, b in zip(dev, ref):
        scale = np.abs(b).max() + 1e-30
        if np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() > rtol * scale + 1e-9:
            return True
    return False


def _call(m, sess, t, n, J, dc, g, post=None):
    return sess.lib.alq_class_layer_sums(m._m, C.c_void_p(t.data_ptr()), n, J, C.c_void_p(dc.data_ptr()),
                                         C.c_void_p(post.data_ptr()) if post is not None else None, C.c_void_p(g.data_ptr()))


@pytest.mark.parametrize('name,ld,in_shape,sk,wseed,xseed', _nets())
def test_class_layer_sums_vs_fp64_oracle(sess, name, ld, in_shape, sk, wseed, xseed):
    """Every class of every sample against torch autograd in fp64, shrunk by alpath.shrink_gradient.  Per layer t,
    e(path)[t] = max over samples and classes |g_path - g64|; the bar is e(fused)[t] <= 2 e(rows)[t] + 6e-8 mean |entry of
    layer t| (fp64 gradient): the two arms see the same fp32 cotangents and differ in summation order only (factor 2); the
    floor is one fp32 rounding of the layer's typical entry (the 'sum' shrink cancels, a bar relative to |g| would be
    meaningless).  A sample whose rows-arm gradient misses the bar of test_full_log_posterior_gradients_vs_oracle against
    fp64 (a ReLU or pool decision flipped) is left out: at most 1 in 16, and none for the fp32 oracle on the CPU."""
    import torch
    n = 16
    m, pars = _mk(sess, ld, in_shape, sk, wseed)
    c, L = m.nclass, m.L
    om64 = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
    om32 = OracleModel(ld, in_shape, pars, skips=sk)
    x = np.random.RandomState(xseed).randn(n, *in_shape).astype(np.float32)
    g64 = np.zeros((n, c, L))
    absent = np.zeros((n, c, L))
    full64 = {}
    for i in range(n):
        for j in range(c):
            gr = om64.grad_log_post(j, x[[i]])
            full64[i, j] = gr
            g64[i, j] = alpath.shrink_gradient(gr)
            absent[i, j] = [(np.abs(gr[2 * t]).sum() + np.abs(gr[2 * t + 1]).sum()) / (gr[2 * t].size + gr[2 * t + 1].size)
                            for t in range(L)]
            assert not _misses_gradient_bar(om32.grad_log_post(j, x[[i]]), gr), (name, 'fp32 oracle flips', i, j)
    mean_abs = absent.mean(axis=(0, 1))
    # flip screen on the rows arm's full gradients
    t = _dev(sess, x)
    out = np.zeros(n, bool)
    for j in range(c):
        rows = m.param_grads_device(t, n, 0, cls=j)[0].cpu().numpy()
        for i in range(n):
            out[i] |= _misses_gradient_bar(m.unflatten(rows[i]), full64[i, j])
    print('%s: samples left out by the flip screen: %d of %d' % (name, out.sum(), n))
    assert out.sum() <= n // 16
    g_rows = m.shrunk_class_gradients(x)[0].cpu().numpy()
    assert sess.lib.alq_model_engine_info(m._m, 15) == 0
    g_fused = _sums(m, sess, x, np.tile(np.arange(c), (n, 1)))
    assert sess.lib.alq_model_engine_info(m._m, 15) == 1
    assert g_fused.shape == g_rows.shape == (n, c, L)
    keep = ~out
    e_fused = np.abs(g_fused - g64)[keep].max(axis=(0, 1))
    e_rows = np.abs(g_rows - g64)[keep].max(axis=(0, 1))
    bar = 2 * e_rows + 6e-8 * mean_abs
    for tt in range(L):
        print('%s layer %d: e(fused) %.3e  e(rows) %.3e  ratio %.3f  floor %.3e  max|g64| %.3e'
              % (name, tt, e_fused[tt], e_rows[tt], e_fused[tt] / max(e_rows[tt], 1e-300), 6e-8 * mean_abs[tt], np.abs(g64[:, :, tt]).max()))
    assert np.all(e_fused <= bar), (name, e_fused, e_rows, bar)
    m.close()


def test_batch_cuts_and_repeats_are_bit_identical(sess):
    """37 samples in one pass, in passes of 16 / 16 / 5 and a second time: the same bits."""
    ld, sk = net_3d_skip(4)
    in_shape = (8, 8, 8, 1)
    x = np.random.RandomState(21).randn(37, *in_shape).astype(np.float32)
    classes = np.random.RandomState(22).randint(0, 4, size=(37, 3))
    m64, pars = _mk(sess, ld, in_shape, sk, 75, max_batch=64)
    one = _sums(m64, sess, x, classes)
    again = _sums(m64, sess, x, classes)
    m64.close()
    m16, _ = _mk(sess, ld, in_shape, sk, 75, max_batch=16)
    cut = _sums(m16, sess, x, classes)
    m16.close()
    assert one.shape == (37, 3, m16.L) and np.all(np.isfinite(one)) and np.abs(one).max() > 0
    np.testing.assert_array_equal(one, again)
    np.testing.assert_array_equal(one, cut)


def test_per_sample_slots(sess):
    """A slot that holds one class for every sample returns the bits of that class in another slot position, and a sample's
    row does not change when its neighbours' classes do."""
    ld = netspec.net_a(nclass=12)
    in_shape = (20, 20, 1)
    m, _ = _mk(sess, ld, in_shape, (), 76)
    n = 9
    x = np.random.RandomState(23).randn(n, *in_shape).astype(np.float32)
    a = _sums(m, sess, x, np.tile([5, 0, 11], (n, 1)))
    b = _sums(m, sess, x, np.tile([11, 5], (n, 1)))
    np.testing.assert_array_equal(a[:, 0], b[:, 1])
    np.testing.assert_array_equal(a[:, 2], b[:, 0])
    assert np.abs(a[:, 0] - a[:, 1]).max() > 0
    cls = np.random.RandomState(24).randint(0, 12, size=(n, 2))
    ref = _sums(m, sess, x, cls)
    other = (cls + 1 + np.arange(n)[:, None]) % 12
    for i in (0, 4, 8):
        mixed = other.copy()
        mixed[i] = cls[i]
        np.testing.assert_array_equal(_sums(m, sess, x, mixed)[i], ref[i])
    # the slots against the one-class passes, class by class
    for j in np.unique(cls[:, 0]):
        one = _sums(m, sess, x, np.full((n, 1), j))
        np.testing.assert_array_equal(ref[cls[:, 0] == j, 0], one[cls[:, 0] == j, 0])
    m.close()


def test_arguments(sess):
    """A class of c or -1: ALQ_EINVAL, output (and posteriors) untouched.  J and N outside their ranges: ALQ_EINVAL."""
    torch = sess.torch
    ld = netspec.net_a(nclass=3)
    in_shape = (20, 20, 1)
    m, _ = _mk(sess, ld, in_shape, (), 77, max_batch=8)
    n, J = 4, 2
    t = _dev(sess, np.random.RandomState(25).randn(n, *in_shape))
    sess.bind_stream()
    for bad in (3, -1):
        cls = np.array([[0, 1, 2, 0], [1, bad, 0, 2]], dtype=np.int32)
        g = torch.full((n, J, m.L), 7.25, dtype=torch.float64, device=t.device)
        post = torch.full((3, n), -3., dtype=torch.float32, device=t.device)
        rc = _call(m, sess, t, n, J, sess.to_device(cls, torch.int32), g, post)
        assert rc == -1, rc
        assert bool((g == 7.25).all()) and bool((post == -3.).all())
    ok = sess.to_device(np.zeros((J, n), dtype=np.int32), torch.int32)
    g = sess.empty((n, J, m.L), torch.float64)
    assert _call(m, sess, t, n, 0, ok, g) == -1
    assert _call(m, sess, t, n, 65, ok, g) == -1
    assert _call(m, sess, t, 9, J, ok, g) == -1          # N > max_batch
    assert _call(m, sess, t, n, J, ok, g) == 0
    post = sess.empty((3, n), torch.float32)
    assert _call(m, sess, t, n, J, ok, g, post) == 0
    np.testing.assert_allclose(post.cpu().numpy().sum(0), 1., rtol=0, atol=1e-6)
    m.close()


@pytest.mark.parametrize('fname,kind', [('fisher_neta.npz', 'a'), ('fisher_netc2d.npz', 'c2'), ('fisher_netc_8cube.npz', 'c')])
def test_one_slot_on_a_two_class_net_vs_alq_fisher(sess, golden_dir, fname, kind):
    """J = 1 on a two-class net: the class-1 and class-0 sums agree with alq_fisher's g1 and g0 on non-saturated samples to
    the bars of test_gen_A_matrices_vs_golden (g: atol 1e-4, p90-relative 1e-3 above 1e-5, median 1e-4)."""
    g = _load(golden_dir, fname)
    ld, skips, in_shape, pars = build_fisher_model(g, kind)
    from nnal_amd import device
    m = device.DeviceModel(sess, ld, in_shape, skips, max_batch=16)
    m.set_weights(pars)
    x = g['x']
    res = m.fisher(x, None, float(g['diag_load']))
    p1 = res['p1']
    mid = (p1 > 1e-6) & (p1 < 1 - 1e-6)
    assert mid.sum() >= 2
    n = len(x)
    s1 = _sums(m, sess, x, np.ones((n, 1), dtype=np.int64))[:, 0]
    s0 = _sums(m, sess, x, np.zeros((n, 1), dtype=np.int64))[:, 0]
    assert_scores_close(s1[mid], res['g1'][mid], SCORE_ATOL, G_RTOL, 1e-5)
    assert_scores_close(s0[mid], res['g0'][mid], SCORE_ATOL, G_RTOL, 1e-5)
    # d log p1 = -p0 u and d log p0 = p1 u: p1 s1 = -p0 s0
    assert_scores_close((p1[:, None] * s1)[mid], (-(1. - p1)[:, None] * s0)[mid], SCORE_ATOL, G_RTOL, 1e-5)
    m.close()


@pytest.mark.parametrize('tag', ['c3', 'c12'])
def test_image_level_fi_query_on_both_arms(sess, golden_dir, tmp_path, tag, monkeypatch):
    """NNAL.CNN_query(..., 'fi') on the golden of test_image_level_fi_device: the fused default (engine info 15 = 1) and the
    rows arm under ALQ_FI_ROWS=1 (engine info 15 = 0), each to that test's bars (Q equal, A rtol 2e-3, atol 2e-5 max|A|)."""
    from nnal_amd import NN
    g = _load(golden_dir, 'r3_imgfi.npz')

    def make(ld, in_shape, pars):
        m = NN.CNN(in_shape, ld, 'imgfi', len(ld) - 2, None, sess=sess, max_batch=5)
        m.set_weights(pars)
        return m, sess
    for rows, info in ((False, 1), (True, 0)):
        if rows:
            monkeypatch.setenv('ALQ_FI_ROWS', '1')
        else:
            monkeypatch.delenv('ALQ_FI_ROWS', raising=False)
        (tmp_path / str(info)).mkdir()
        model = _imgfi_case(g, tag, tmp_path / str(info), make, 2e-3, 2e-5 * np.abs(g[tag + '_A']).max())
        assert sess.lib.alq_model_engine_info(model._m, 15) == info
        model.close()
