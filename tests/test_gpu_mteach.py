"""Mean-teacher consistency training on the device (csrc/mteach.hip; GPU box): the cotangent kernel on fed posteriors against
the fp64 statement (nnal_amd.mteach), whole nets against the fp64 torch graph of tests/dense_ref.py, the moving average, the
input perturbation, three optimiser steps against a NumPy / torch stepper, the training loop and the refusals.

Bars: rows 4 * 2^-24 * (|labelled term| + |consistency term|) - the row is three fp32 roundings of fp64 arithmetic on the same
fp32 inputs; statistics 1e-12 relative; whole nets as tests/test_gpu_dense.py (posteriors 2e-6, loss 1e-6 relative, gradients
2e-4 of max|g64|); steps as tests/test_gpu_losses.py (2e-5 / 5e-4)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dense_ref, test_gpu_losses  # noqa: E402
from tests.test_gpu_losses import _TorchStep, _objective, _weights_close  # noqa: E402
from tests.test_gpu_train import _close  # noqa: E402
from tests.test_mteach_host import ANGLES, SIZES  # noqa: E402

CW = [0.3, 1.7]
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def P(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def _posteriors(rs, c, R):
    z = rs.randn(c, R) * 2.
    e = np.exp(z - z.max(0))
    return (e / e.sum(0)).astype(np.float32)


def _mt_call(sess, p, q, lab, measure, s, k, cw=None, sw=None, gamma=None, off=0, rows=True):
    """alq_mt_cotangent (or alq_mt_stats) on host arrays; `off`: the planes start that many floats into their buffers."""
    from nnal_amd._lib import LossT, check
    torch = sess.torch
    c, R = p.shape

    def up(a, dt=torch.float32):
        buf = sess.empty((a.size + off,), dt)
        buf[off:] = sess.to_device(a.reshape(-1), dt)
        return buf
    pd, qd, ld = up(p), up(q), sess.to_device(lab.astype(np.int32), torch.int32)
    cwd = sess.to_device(np.asarray(cw, np.float32), torch.float32) if cw is not None else None
    swd = sess.to_device(sw.astype(np.float32), torch.float32) if sw is not None else None
    L = LossT(0, -1. if gamma is None else gamma, 0.7, 1., cwd.data_ptr() if cwd is not None else None,
              swd.data_ptr() if swd is not None else None, None, None)
    out = torch.full((R, c), float('nan'), dtype=torch.float32, device=sess.device)
    st = torch.full((3,), float('nan'), dtype=torch.float64, device=sess.device)
    sess.bind_stream()
    if rows:
        check(sess.lib.alq_mt_cotangent(sess.ctx, P(pd, 4 * off), P(qd, 4 * off), c, R, P(ld), C.byref(L), float(s), float(k), measure, P(out), P(st)))
    else:
        check(sess.lib.alq_mt_stats(sess.ctx, P(pd, 4 * off), P(qd, 4 * off), c, R, P(ld), C.byref(L), measure, P(st)))
    return out.cpu().numpy(), st.cpu().numpy()


def _kernel_case(sess, R, c, measure, weighted, off=0, seed=0):
    from nnal_amd import mteach
    rs = np.random.RandomState(seed + 7 * c + R % 1000)
    p, q = _posteriors(rs, c, R), _posteriors(rs, c, R)
    lab = rs.randint(0, c, size=R)
    cw = sw = gamma = None
    if weighted:
        lab[rs.rand(R) < 0.3] = -1
        sw = (0.25 + rs.rand(R)).astype(np.float32)
        sw[rs.rand(R) < 0.05] = 0
        if c == 2:
            cw, gamma = np.asarray(CW, np.float32), 2.          # (the statement reads the weights the device reads)
    s, k = np.float32(3. / max(R, 1)), np.float32(0.8 * 2. / (c * 35))
    rows, st = _mt_call(sess, p, q, lab, measure, s, k, cw, sw, gamma, off)
    rows2, st2 = _mt_call(sess, p, q, lab, measure, s, k, cw, sw, gamma, off)
    assert rows.tobytes() == rows2.tobytes() and st.tobytes() == st2.tobytes()          # no atomics: the same bits
    ref = mteach.evaluate(p, q, lab, measure, float(s), float(k), cw, sw, gamma)
    tol = 4 * 2. ** -24 * (np.abs(ref['labelled_rows']) + np.abs(ref['cons_rows']))
    err = np.abs(rows.astype(np.float64) - ref['rows'])
    print('R=%d c=%d measure=%d weighted=%d off=%d: worst row error / bound %.3f, stats %s' % (R, c, measure, weighted, off,
          (err / np.maximum(tol, 1e-300)).max(), st))
    assert not np.isnan(rows).any() and (err <= tol).all()
    for a, b in zip(st, ref['stats']):
        assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300) or a == b
    _, st3 = _mt_call(sess, p, q, lab, measure, s, k, cw, sw, gamma, off, rows=False)
    assert st3.tobytes() == st.tobytes()
    if measure == mteach.CE:
        assert np.array_equal(rows, _mt_call(sess, p, q, lab, measure, s, np.float32(0.), cw, sw, gamma, off)[0])


@pytest.mark.parametrize('measure', [0, 1])
@pytest.mark.parametrize('c', [2, 3, 8])
@pytest.mark.parametrize('shape', ['R140', 'R105', 'R1', 'R140_unaligned'])
def test_cotangent_kernel_vs_fp64_statement(sess, shape, c, measure):
    """140 = 4 x 5 x 7 voxels: the 16-byte path; 105: R % 4 != 0, the guarded path; 1; 140 with the planes one float into their
    buffers: unaligned bases, the guarded path again."""
    R = {'R140': 140, 'R105': 105, 'R1': 1, 'R140_unaligned': 140}[shape]
    for weighted in (False, True):
        _kernel_case(sess, R, c, measure, weighted, off=1 if shape.endswith('unaligned') else 0)


@pytest.mark.parametrize('measure', [0, 1])
def test_cotangent_kernel_beyond_one_trip_of_the_grid(sess, measure):
    """Four voxels more than one sweep of the capped grid covers (the kernel's exported figure): one lane grid-strides."""
    R = int(sess.lib.alq_mt_trip_voxels()) + 4
    assert R % 4 == 0 and R < 2 ** 22
    _kernel_case(sess, R, 2, measure, True)


def _dense_model(sess, tag, c=2, in_shape=(16, 16, 1), fn='net_c_2d_dense', max_batch=8, dropout=None, seed=61, **hy):
    from nnal_amd import NN_extended, netspec
    ld, sk = getattr(netspec, fn)(c)
    pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    m = NN_extended.CNN(in_shape, ld, tag, list(sk), dropout=dropout, sess=sess, max_batch=max_batch, **hy)
    m.set_weights(pars)
    return m, ld, sk, pars


@pytest.mark.parametrize('drop', [False, True])
def test_zero_consistency_scale_writes_the_bits_of_param_grads_loss(sess, drop):
    from nnal_amd._lib import LossT, check
    torch = sess.torch
    m, _, _, _ = _dense_model(sess, 'k0', dropout=[[0], 0.5] if drop else None)
    n, V, c = 4, m.out_voxels, 2
    rs = np.random.RandomState(5)
    t = sess.to_device(rs.randn(n, 256).astype(np.float32), torch.float32)
    lab = rs.randint(0, 2, size=n * V)
    lab[rs.rand(n * V) < 0.3] = -1
    labd = sess.to_device(lab.astype(np.int32), torch.int32)
    tq = sess.to_device(_posteriors(rs, c, n * V), torch.float32)
    L = LossT(0, -1., 0.7, 1., None, None, None, None)
    kp, arr, nl, seed = m._drop_args(0.5 if drop else 1., 77)
    s = 4. / np.count_nonzero(lab >= 0)
    outs = []
    sess.bind_stream()
    for mt in (False, True):
        g = torch.full((m.num_params,), float('nan'), dtype=torch.float32, device=sess.device)
        st = sess.empty((3,), torch.float64)
        if mt:
            check(m.lib.alq_param_grads_loss_mt(m._m, P(t), n, P(labd), C.byref(L), s, P(tq), 0, 0., kp, seed, 0, arr, nl, P(g), None, P(st)))
        else:
            check(m.lib.alq_param_grads_loss(m._m, P(t), n, P(labd), C.byref(L), s, 0., kp, seed, 0, arr, nl, P(g), None, P(st)))
        outs.append((g.cpu().numpy(), st.cpu().numpy()[:2]))
    assert not np.isnan(outs[0][0]).any() and np.abs(outs[0][0]).max() > 0
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    # the statistics are the same sums folded in another order (4 voxels a lane, up to 2048 workgroups): equal to fp64 rounding
    assert abs(outs[0][1][0] - outs[1][1][0]) <= 1e-12 * abs(outs[0][1][0]) and outs[0][1][1] == outs[1][1][1]
    m.close()


def _mt_reference(g, gt, hy, x, px, ycols, vw, measure, coeff, N):
    """(value, what the optimiser differentiates) of loss = L + coeff * cons read as the vector [N], in torch on graph g with
    the teacher's posteriors (graph gt on px) as constants."""
    import torch
    z = g._graph(g._as_input(x))['output']
    L, _ = _objective(hy, z, ycols, vw)
    with torch.no_grad():
        zt = gt._graph(gt._as_input(px))['output']
    p = torch.softmax(z, 0)
    if measure == 'L2':
        div = ((p - torch.softmax(zt, 0)) ** 2).mean(0)
    else:
        div = -(p.detach() * torch.log_softmax(zt, 0)).sum(0)          # TF: no gradient into the labels
    cons = div.reshape(N, -1).mean(1)
    return L + coeff * cons.mean(), N * L + coeff * cons.sum()


NETS = {'2d_c2': ('net_c_2d_dense', 2, (16, 16, 1), 4, 44), '2d_c3': ('net_c_2d_dense', 3, (16, 16, 1), 4, 44),
        '3d_8': ('net_c_dense', 2, (8, 8, 8, 1), 2, 53)}


@pytest.mark.parametrize('measure', ['L2', 'CE'])
@pytest.mark.parametrize('net', sorted(NETS))
def test_whole_nets_vs_fp64(sess, net, measure):
    """Student and a teacher of different weights through tests/dense_ref.DenseGraph; 2-D nets at max_batch 3: two cuts."""
    import torch
    from nnal_amd import NN_extended, mteach, netspec, ref64
    fn, c, in_shape, N, seed = NETS[net]
    max_coeff, ramp = 150., 1.          # cons_coeff = 150 exp(-5) = 1.01 at step 0
    m, ld, sk, pars = _dense_model(sess, 'mt ' + net, c, in_shape, fn, 3 if len(in_shape) == 3 else 8, [[0], 0.5], seed, MT_SSL=True,
                                   output_perturbation_measure=measure, max_cons_coeff=max_coeff, rampup_length=ramp, learning_rate=0.01)
    m.get_optimizer()
    tpars = netspec.he_init(ld, in_shape, seed=seed + 1, skips=sk, bias_std=0.05)
    m.teacher.set_weights(tpars)
    coeff = mteach.cons_coeff(0, ramp, max_coeff)
    assert m.cons_coeff == coeff and abs(coeff - 1.01) < 0.01
    g64, g32 = (dense_ref.DenseGraph(ld, in_shape, pars, sk, dt) for dt in (torch.float64, torch.float32))
    t64, t32 = (dense_ref.DenseGraph(ld, in_shape, tpars, sk, dt) for dt in (torch.float64, torch.float32))
    x, _ = dense_ref.select_inputs(g64, in_shape, N, seed + 1000, ref64.DEFAULT_EPS)
    px, _ = dense_ref.select_inputs(t64, in_shape, N, seed + 2000, ref64.DEFAULT_EPS)
    tpost = sess.run(m.teacher.posteriors, feed_dict={m.teacher.x: px})
    assert np.abs(tpost - t64.posteriors(px)).max() <= 2e-6
    rs = np.random.RandomState(seed + 7)
    shape = (N,) + tuple(in_shape[:-1])
    variants = [('plain', {}, 0., False, 1.), ('weighted', dict(bin_class_weights=CW, focal_gamma=2.) if c == 2 else {}, 0.3, True, 1.),
                ('dropout', {}, 0., False, 0.5)]
    for name, hy, unl, weights, kp in variants:
        lab = rs.randint(0, c, size=shape)
        y = (lab[..., None] == np.arange(c)).astype(np.float32)
        y[rs.rand(*shape) < unl] = 0
        vw = (0.25 + rs.rand(*shape)).astype(np.float32) if weights else None
        if weights:
            vw[rs.rand(*shape) < 0.05] = 0
        ycols = np.ascontiguousarray(y.reshape(-1, c).T)
        hyf = dict(loss_name='CE', **hy)
        m.set_hypers(dict(NN_extended.CNN.DEFAULT_HYPERS, **hyf))
        refs = []
        for g, gt in ((g64, t64), (g32, t32)):
            g.drop = dict(layers=[0], keep_prob=kp, seed=20251, first_sample=0) if kp < 1. else None
            val, diff = _mt_reference(g, gt, hyf, x, px, ycols, None if vw is None else vw.reshape(-1), measure, coeff, N)
            refs.append((float(val.detach()), dense_ref.flat_grads(g, diff)))
            g.drop = None
        (l64, gr64), (_, gr32) = refs
        t, n = m._as_device_batch(x)
        gsum, l_dev = m._objective_pass(t, n, ycols, kp, 20251, None if vw is None else vw.reshape(-1), None, mt_feed=dict(kp=1., px=px))
        gdev = m.unflatten(gsum.cpu().numpy())
        rel = lambda a, b: max(np.abs(np.asarray(u, np.float64) - v).max() / (np.abs(v).max() + 1e-30) for u, v in zip(a, b))
        e_dev, e_32 = rel(gdev, gr64), rel(gr32, gr64)
        print('%s %s %s: loss %.9g vs %.9g, labelled %.6g cons %.6g, gradients e_dev %.3e e_32 %.3e e_dev / e_32 = %.2f'
              % (net, measure, name, l_dev, l64, m._mt['last'][0], m._mt['last'][1], e_dev, e_32, e_dev / max(e_32, 1e-30)))
        assert abs(l_dev - l64) <= 1e-6 * abs(l64), (name, l_dev, l64)
        _close(gdev, gr64, name='%s %s %s' % (net, measure, name))
        if kp == 1.:          # the same figures through the reference's call shapes
            fd = {m.x: x, m.y_: y, m.keep_prob: 1., m.perturbed_x: px}
            if vw is not None:
                fd[m.input_vox_weights] = vw
            assert sess.run(m.loss, feed_dict=fd) == l_dev
            lab_l, cons_l = sess.run(m.labeled_loss, feed_dict=fd), sess.run(m.cons_loss, feed_dict=fd)
            assert lab_l + coeff * cons_l == l_dev
    with pytest.raises(NotImplementedError):
        m._objective_pass(t, n, ycols, 1., None, None, (np.zeros((c, n * m.out_voxels)), 1., 2.))          # LwF
    m.teacher.close()
    m.close()


@pytest.mark.parametrize('n,off', [(1, 0), (3, 0), (4, 0), (1027, 0), (1027, 1)])
def test_ema_step_bit_exact(sess, n, off):
    from nnal_amd import mteach
    from nnal_amd._lib import check
    torch = sess.torch
    rs = np.random.RandomState(n + off)
    sh, th = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    bufs = []
    for a in (sh, th):
        b = torch.zeros((n + off + 3,), dtype=torch.float32, device=sess.device)
        b[off:off + n] = sess.to_device(a, torch.float32)
        bufs.append(b)
    sess.bind_stream()
    check(sess.lib.alq_ema_step(sess.ctx, P(bufs[0], 4 * off), P(bufs[1], 4 * off), n, 0.9))
    got = bufs[0].cpu().numpy()
    assert got[off:off + n].tobytes() == mteach.ema_step(sh, th, 0.9).tobytes()
    assert not got[:off].any() and not got[off + n:].any()          # nothing outside the vector


def test_ema_apply_repacks_the_teacher(sess):
    """After sess.run(model.ema_apply) the teacher computes what a fresh model given the shadow weights computes, bit for bit;
    the shadow started as a copy of the student's weights, and a teacher.set_weights overrides it."""
    from nnal_amd import device, mteach, netspec
    m, ld, sk, pars = _dense_model(sess, 'ema', MT_SSL=True, MT_ema_decay_schedule=lambda t: 0.5 + 0.1 * t, learning_rate=0.05)
    m.get_optimizer()
    rs = np.random.RandomState(8)
    x = rs.randn(3, 16, 16, 1).astype(np.float32)
    y = (rs.randint(0, 2, size=(3, 16, 16))[..., None] == np.arange(2)).astype(np.float32)
    theta0 = m.flat_params().copy()
    sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1.})
    assert np.array_equal(m.teacher.flat_params(), theta0)                     # the first use of the teacher: the student's weights
    sess.run(m.ema_apply)
    theta1 = m.flat_params()
    want = mteach.ema_step(theta0, theta1, 0.6)                                # decay schedule at global_step = 1
    assert np.array_equal(m._mt['shadow'].cpu().numpy(), want) and not np.array_equal(want, theta0)
    fresh = device.DeviceModel(sess, ld, (16, 16, 1), sk, max_batch=8)
    fresh.set_flat_params(want)
    a = sess.run(m.teacher.posteriors, feed_dict={m.teacher.x: x})
    b = sess.run(fresh.posteriors, feed_dict={fresh.x: x})
    assert a.tobytes() == b.tobytes()
    other = netspec.he_init(ld, (16, 16, 1), seed=99, skips=sk, bias_std=0.05)
    m.teacher.set_weights(other)
    sess.run(m.ema_apply)
    fresh.set_weights(other)
    assert np.array_equal(m._mt['shadow'].cpu().numpy(), mteach.ema_step(fresh.flat_params(), theta1, 0.6))
    for mod in (fresh, m.teacher, m):
        mod.close()


def _perturb(sess, x, std, seed, first, angle):
    from nnal_amd._lib import check
    torch = sess.torch
    N, H, W, Cc = x.shape
    xd = sess.to_device(x, torch.float32)
    out = torch.full((x.size,), float('nan'), dtype=torch.float32, device=sess.device)
    sess.bind_stream()
    check(sess.lib.alq_perturb_input(sess.ctx, P(xd), P(out), N, H, W, Cc, std, seed, first, int(angle is not None), float(angle or 0.)))
    return out.cpu().numpy().reshape(x.shape)


@pytest.mark.parametrize('Cc', [1, 3])
def test_rotation_equals_the_statement(sess, Cc):
    from nnal_amd import mteach
    for H, W in SIZES:
        x = np.random.RandomState(H + W + Cc).randn(2, H, W, Cc).astype(np.float32)
        for angle in ANGLES:
            got = _perturb(sess, x, 0., 0, 0, angle)
            assert np.array_equal(got, mteach.perturb(x, angle=angle)[0]), (H, W, angle)
    assert np.array_equal(_perturb(sess, x, 0., 0, 0, None), x)


def test_noise_against_the_statement_and_batch_split(sess):
    from nnal_amd import mteach
    std = 0.7
    zero = np.zeros((5, 12, 20, 3), np.float32)
    got = _perturb(sess, zero, std, 9, 10, None)
    want = mteach.perturb(zero, std, seed=9, first_sample=10)[0]
    err = np.abs(got - want).max()
    print('noise: max |device - statement| = %.3e std (bar 1e-5), sample mean %.4f var %.4f' % (err / std, got.mean() / std, got.var() / std ** 2))
    assert err <= 1e-5 * std
    x = np.random.RandomState(2).randn(5, 12, 20, 3).astype(np.float32)
    for angle in (None, 0.3):
        whole = _perturb(sess, x, std, 9, 10, angle)
        parts = np.concatenate([_perturb(sess, x[:2], std, 9, 10, angle), _perturb(sess, x[2:], std, 9, 12, angle)])
        assert whole.tobytes() == parts.tobytes()
        ref, eps = mteach.perturb(x, std, seed=9, first_sample=10, angle=angle)
        assert np.abs(whole - ref).max() <= 1e-5 * std + 2. ** -23 * np.abs(ref).max()          # ... plus the rounding of x + noise
    vol = np.random.RandomState(3).randn(2, 4, 6, 5, 1).astype(np.float32)          # a 3-D batch: D * H rows, no rotation
    got = _perturb(sess, vol.reshape(2, 24, 5, 1), std, 4, 0, None).reshape(vol.shape)
    assert np.abs(got - mteach.perturb(vol, std, seed=4)[0]).max() <= 1e-5 * std + 2. ** -23 * np.abs(vol).max()


@pytest.mark.parametrize('opt', ['SGD', 'Adam'])
def test_three_steps_vs_numpy_stepper(sess, opt, monkeypatch):
    """train_step + ema_apply with noise and rotation; rampup_length 2 and decay 0.9, so the consistency coefficient and the
    moving average both move.  The stepper is tests.test_gpu_losses._TorchStep with the mean-teacher objective as its oracle."""
    import torch
    from nnal_amd import mteach, netspec
    in_shape, N, lr = (16, 16, 1), 6, (0.003 if opt == 'SGD' else 0.002)
    bound = 2e-5 if opt == 'SGD' else 5e-4
    hy = dict(bin_class_weights=CW, optimizer_name=opt, learning_rate=lr, beta1=0.8, beta2=0.99)
    mt = dict(MT_SSL=True, output_perturbation_measure='L2', max_cons_coeff=20., rampup_length=2, Gaussian_noise_std=0.1, rotation_angle=0.2,
              MT_ema_decay_schedule=lambda t: 0.9)
    m, ld, sk, pars = _dense_model(sess, 'steps', seed=74, **dict(hy, **mt))
    m.get_optimizer()
    g32, t32 = (dense_ref.DenseGraph(ld, in_shape, pars, sk, torch.float32) for _ in range(2))
    state = {}

    def oracle(om, hy_, x, y, sw=None, lwf=None):
        val, diff = _mt_reference(om, t32, hy_, x, state['px'], y, sw, 'L2', state['coeff'], N)
        return float(val.detach()), dense_ref.flat_grads(om, diff)
    monkeypatch.setattr(test_gpu_losses, '_oracle', oracle)
    ref = _TorchStep(g32, hy, lr)
    for step in range(3):
        rs = np.random.RandomState(30 + step)
        x = rs.randn(N, *in_shape).astype(np.float32)
        lab = rs.randint(0, 2, size=(N, 16, 16))
        y = (lab[..., None] == np.arange(2)).astype(np.float32)
        y[rs.rand(N, 16, 16) < 0.3] = 0
        vw = (0.25 + rs.rand(N, 16, 16)).astype(np.float32)
        np.random.seed(100 + step)
        nseed = int(np.random.randint(0, 2 ** 31 - 1))          # the one draw of the step: no dropout on either model
        state['px'] = mteach.perturb(x, 0.1, seed=nseed, angle=0.2)[0].astype(np.float32)
        state['coeff'] = mteach.cons_coeff(step, 2, 20.)
        assert m.cons_coeff == state['coeff']
        np.random.seed(100 + step)
        l_dev = sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1., m.input_vox_weights: vw})
        sess.run(m.ema_apply)
        l_ref = ref.step(x, np.ascontiguousarray(y.reshape(-1, 2).T), vw.reshape(-1))
        with torch.no_grad():
            for nme in t32.params:
                for ps, pt in zip(g32.params[nme], t32.params[nme]):
                    pt.copy_(torch.as_tensor(mteach.ema_step(pt.detach().numpy(), ps.detach().numpy(), 0.9)))
        assert abs(l_dev - l_ref) <= 2e-5 * max(1., abs(l_ref)), (step, l_dev, l_ref)
    assert m.global_step == 3 and m.cons_coeff == 20.
    _weights_close(m, g32, bound, lr, 'mean-teacher student %s' % opt)
    _weights_close(m.teacher, t32, bound, lr, 'mean-teacher teacher %s' % opt)
    m.teacher.close()
    m.close()


def test_train_loop(sess, tmp_path):
    m, ld, sk, pars = _dense_model(sess, 'loop', MT_SSL=True, output_perturbation_measure='L2', Gaussian_noise_std=0.05, learning_rate=0.01)
    m.get_optimizer()
    rs = np.random.RandomState(4)

    def gen():
        x = rs.randn(4, 16, 16, 1).astype(np.float32)
        return x, ((x[..., 0] > 0)[..., None] == np.arange(2)).astype(np.float32)
    m.train(sess, 4, gen, [[['av_loss', 'F1'], gen, 2, 'F1']], eval_step=2, save_path=str(tmp_path))
    assert m.global_step == 4
    files = set(os.listdir(str(tmp_path)))
    ext = '.h5' if 'model_pars.h5' in files else '.npz'
    assert {'av_loss_0.txt', 'F1_0.txt', 'model_pars' + ext, 'teacher_pars' + ext} <= files
    assert len(m.valid_metrics_0['av_loss']) == 2 and len(m.valid_metrics_0['F1']) == 2
    assert len(np.loadtxt(str(tmp_path / 'F1_0.txt'))) == 2
    saved = m.teacher.flat_params().copy()
    m.teacher.load_weights(str(tmp_path / ('teacher_pars' + ext)))
    assert m.teacher.flat_params().shape == saved.shape and not np.array_equal(m.teacher.flat_params(), m.flat_params())
    m.teacher.close()
    m.close()


def test_refusals(sess):
    """ALQ_EINVAL / ALQ_EUNSUPPORTED before any launch: the pre-filled outputs are untouched."""
    from nnal_amd import device, netspec
    from nnal_amd._lib import LossT
    torch = sess.torch
    lib, R, c = sess.lib, 140, 2
    rs = np.random.RandomState(0)
    p, q = (sess.to_device(_posteriors(rs, c, R), torch.float32) for _ in range(2))
    lab = sess.to_device(rs.randint(0, c, size=R).astype(np.int32), torch.int32)
    rows = torch.full((R, c), 7., dtype=torch.float32, device=sess.device)
    st = torch.full((3,), 7., dtype=torch.float64, device=sess.device)
    L, soft = LossT(0, -1., 0.7, 1., None, None, None, None), LossT(1, -1., 0.7, 1., None, None, P(p).value, None)
    sess.bind_stream()
    ok = (sess.ctx, P(p), P(q), c, R, P(lab), C.byref(L), 1., 1., 0, P(rows), P(st))
    bad = {0: None, 1: None, 2: None, 5: None, 6: None, 10: None, 11: None}          # a null pointer; 2: the teacher's planes
    calls = [ok[:i] + (v,) + ok[i + 1:] for i, v in bad.items()]
    calls += [ok[:3] + (cc,) + ok[4:] for cc in (1, 9)] + [ok[:4] + (0,) + ok[5:], ok[:9] + (2,) + ok[10:], ok[:6] + (C.byref(soft),) + ok[7:]]
    for args in calls:
        assert lib.alq_mt_cotangent(*args) == EINVAL, args
    sok = (sess.ctx, P(p), P(q), c, R, P(lab), C.byref(L), 0, P(st))
    for args in [sok[:i] + (None,) + sok[i + 1:] for i in (0, 1, 2, 5, 6, 8)] + [sok[:3] + (9,) + sok[4:], sok[:4] + (0,) + sok[5:], sok[:7] + (-1,) + sok[8:]]:
        assert lib.alq_mt_stats(*args) == EINVAL, args
    assert lib.alq_ema_step(sess.ctx, None, P(p), 5, 0.9) == EINVAL and lib.alq_ema_step(sess.ctx, P(rows), None, 5, 0.9) == EINVAL
    assert lib.alq_ema_step(None, P(rows), P(p), 5, 0.9) == EINVAL and lib.alq_ema_step(sess.ctx, P(rows), P(p), -1, 0.9) == EINVAL
    assert lib.alq_ema_step(sess.ctx, P(rows), P(p), 5, 1.5) == EINVAL
    pok = (sess.ctx, P(p), P(rows), 1, 10, 14, 2, 0.1, 0, 0, 1, 0.3)
    for args in [pok[:i] + (None,) + pok[i + 1:] for i in (0, 1, 2)] + [pok[:3] + (0,) + pok[4:], pok[:7] + (-0.1,) + pok[8:], pok[:2] + (P(p),) + pok[3:]]:
        assert lib.alq_perturb_input(*args) == EINVAL, args
    # alq_param_grads_loss_mt: an fc-head model is unsupported; on a dense model the checks of alq_mt_cotangent hold
    ldf, skf = netspec.net_c_2d(2)
    mf = device.DeviceModel(sess, ldf, (16, 16, 1), skf, max_batch=2)
    mf.set_weights(netspec.he_init(ldf, (16, 16, 1), seed=3, skips=skf))
    x = sess.to_device(rs.randn(2, 256).astype(np.float32), torch.float32)
    g = torch.full((mf.num_params,), 7., dtype=torch.float32, device=sess.device)
    assert lib.alq_param_grads_loss_mt(mf._m, P(x), 2, P(lab), C.byref(L), 1., P(q), 0, 1., 1., 0, 0, None, 0, P(g), None, P(st)) == EUNSUPPORTED
    assert (g == 7.).all()
    mf.close()
    md, _, _, _ = _dense_model(sess, 'refuse')
    V = md.out_voxels
    labd = sess.to_device(rs.randint(0, 2, size=2 * V).astype(np.int32), torch.int32)
    tq = sess.to_device(_posteriors(rs, 2, 2 * V), torch.float32)
    gd = torch.full((md.num_params,), 7., dtype=torch.float32, device=sess.device)
    dok = (md._m, P(x), 2, P(labd), C.byref(L), 1., P(tq), 0, 1., 1., 0, 0, None, 0, P(gd), None, P(st))
    for args in [dok[:i] + (None,) + dok[i + 1:] for i in (0, 1, 3, 4, 6, 14)] + [dok[:2] + (0,) + dok[3:], dok[:2] + (99,) + dok[3:],
                                                                                 dok[:7] + (5,) + dok[8:]]:
        assert lib.alq_param_grads_loss_mt(*args) == EINVAL, args
    assert (gd == 7.).all() and (rows == 7.).all() and (st == 7.).all()
    md.close()
