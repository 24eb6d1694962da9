"""The objectives of NN_extended.CNN on the device (csrc/loss.hip: weighted / focal cross-entropy, CE_softclasses, GCE, the
learning-without-forgetting term), RMSProp and the schedules, against nnal_amd.losses and torch autograd over the oracle graph
(GPU box)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests.test_gpu_train import _close  # noqa: E402

LD_C, SK_C = netspec.net_c()
NETS = {'neta': (netspec.net_a(), (20, 20, 1), ()), 'netc': (LD_C, (8, 8, 8, 1), SK_C)}
CW = [0.3, 1.7]
Q = float(np.float32(0.7))
CASES = {
    'wce': dict(bin_class_weights=CW),
    'focal2': dict(bin_class_weights=CW, focal_gamma=2.),
    'focal05': dict(focal_gamma=0.5),
    'soft': dict(loss_name='CE_softclasses'),
    'gce': dict(loss_name='GCE', q=Q),
}
LWF_LR = 0.0005
SAT_SCALE = 40.       # inputs of the saturated kernel case: x * SAT_SCALE (checked on the CPU in the test)


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _mk(sess, net, seed, max_batch=16, **hypers):
    """An NN_extended.CNN with `hypers` (a plain DeviceModel without), its oracle twin and the weights."""
    from nnal_amd import NN_extended, device
    ld, in_shape, sk = NETS[net]
    pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    if hypers:
        m = NN_extended.CNN(in_shape, ld, net, list(sk), sess=sess, max_batch=max_batch, **hypers)
    else:
        m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
    m.set_weights(pars)
    return m, OracleModel(ld, in_shape, pars, skips=sk), pars


def _batch(net, seed, n=12, soft=False):
    """x, targets [2, n] (one-hot; sample 3 unlabelled - or soft rows), sample weights with a zero at n - 2."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, *NETS[net][1]).astype(np.float32)
    lab = rs.randint(0, 2, size=n)
    y = np.zeros((2, n), dtype=np.float32)
    y[lab, np.arange(n)] = 1
    if soft:
        y = (0.8 * y + 0.2 * rs.rand(2, n)).astype(np.float32)
    else:
        y[:, 3] = 0
    sw = (0.25 + rs.rand(n)).astype(np.float32)
    sw[n - 2] = 0
    return x, y, sw


def _objective(hy, z, y, sw=None, lwf=None):
    """The reference's loss written out in torch on logits z [c, N]: (reported value, what the optimiser differentiates).
    NN_extended.get_loss (:1221-1277) with the focal weights of get_FCN_loss; hy None: the batch mean of NN.py:583-588."""
    import torch
    hy = hy or {}
    c, N = z.shape
    logp, p = torch.log_softmax(z, 0), torch.softmax(z, 0)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float32))
    name = hy.get('loss_name', 'CE')
    if name == 'CE':
        lab = y.sum(0) > 0
        ys = torch.as_tensor(np.where(lab, y.argmax(0), 0))
        w = torch.as_tensor(lab.astype(np.float32))
        if hy.get('bin_class_weights') is not None:
            w = w * torch.as_tensor(np.asarray(hy['bin_class_weights'], dtype=np.float32))[ys]
        if sw is not None:
            w = w * torch.as_tensor(np.asarray(sw, dtype=np.float32))
        cols = torch.arange(N)
        if hy.get('focal_gamma') is not None:
            w = w * (1. - p[ys, cols]) ** float(hy['focal_gamma'])          # no stop_gradient, as in TF
        div = max(int((w.detach() != 0).sum()), 1) if hy else N              # SUM_BY_NONZERO_WEIGHTS / reduce_mean
        val = diff = -(w * logp[ys, cols]).sum() / div
    elif name == 'CE_softclasses':
        val = diff = -(yt * logp).sum(0).mean()
    else:
        q = float(hy['q'])
        per = (yt * (1. - torch.clamp(p, 1e-4, 1 - 1e-4) ** q) / q).mean(0)
        val, diff = per.mean(), per.sum()
    if lwf is not None:
        old, lam, T = lwf
        tau = torch.softmax(torch.as_tensor(np.asarray(old, dtype=np.float32)) / T, 0)
        extra = lam * (-(tau * torch.log_softmax(z / T, 0)).sum(0)).mean()
        val, diff = val + extra, diff + extra
    return val, diff


def _oracle(om, hy, x, y, sw=None, lwf=None):
    import torch
    z = om._graph(om._as_input(x))['output']
    val, diff = _objective(hy, z, y, sw, lwf)
    plist = [p for pair in om.params.values() for p in pair]
    grads = torch.autograd.grad(diff, plist, allow_unused=True)
    return float(val.detach()), [np.zeros(tuple(p.shape), np.float32) if g is None else g.numpy() for p, g in zip(plist, grads)]


class _TorchStep(object):
    """SGD / Adam(beta1, beta2) / RMSProp(decay, momentum, eps; rms slot from ones) restated in fp32 NumPy on the oracle's
    variables (TF 1.x documentation of the three optimisers)."""

    def __init__(self, om, hy, lr, train_layers=()):
        self.om, self.hy, self.lr, self.t, self.slots, self.train_layers = om, hy, lr, 0, None, list(train_layers)

    def step(self, x, y, sw=None, lwf=None):
        import torch
        f = np.float32
        hy = self.hy or {}
        lr = f(self.lr(self.t) if callable(self.lr) else self.lr)
        loss, grads = _oracle(self.om, self.hy, x, y, sw, lwf)
        self.t += 1
        name = hy.get('optimizer_name', 'SGD')
        if self.slots is None:
            self.slots = [[np.zeros_like(g), np.zeros_like(g), np.ones_like(g), np.zeros_like(g)] for g in grads]
        names = list(self.om.params.keys())
        for k, g in enumerate(grads):
            if self.train_layers and names[k // 2] not in self.train_layers:
                continue
            pr = self.om.params[names[k // 2]][k % 2]
            th = pr.detach().numpy().copy()
            sl = self.slots[k]
            if name == 'SGD':
                th = th - lr * g
            elif name == 'Adam':
                b1, b2 = f(hy['beta1']), f(hy['beta2'])
                lr_t = f(float(lr) * np.sqrt(1.0 - float(b2) ** self.t) / (1.0 - float(b1) ** self.t))
                sl[0] = b1 * sl[0] + (f(1) - b1) * g
                sl[1] = b2 * sl[1] + (f(1) - b2) * g * g
                th = th - lr_t * sl[0] / (np.sqrt(sl[1]) + f(1e-8))
            else:
                d, mo, eps = f(hy.get('decay', 0.9)), f(hy.get('momentum', 0.)), f(hy.get('epsilon', 1e-10))          # DEFAULT_HYPERS
                sl[2] = d * sl[2] + (f(1) - d) * g * g
                sl[3] = mo * sl[3] + lr * g / np.sqrt(sl[2] + eps)
                th = th - sl[3]
            with torch.no_grad():
                pr.copy_(torch.as_tensor(th))
        return loss


def _weights_close(m, om, bound, lr, tag=''):
    worst = 0.
    for n in m.var_names:
        for a, b in zip(m.var_dict[n], om.params[n]):
            b = b.detach().numpy()
            tol = bound * max(np.abs(b).max(), lr)
            err = np.abs(a - b).max()
            worst = max(worst, err / max(np.abs(b).max(), lr))
            assert err <= tol, '%s %s: max err %.3e > %.3e' % (tag, n, err, tol)
    print('%s: max weight error / max(|w|max, lr) = %.3e' % (tag, worst))
    return worst


def _raw_pass(sess, m, x, y, hy, sw=None, lwf=None, loss_scale=1., lwf_scale=0.):
    """alq_param_grads_loss called directly on one pass: (device posteriors [c, n], cotangent rows [n, c] read back with
    alq_model_debug_copy from the head's cotangent buffer, statistics [3], LossT keep-alives)."""
    from nnal_amd import losses
    from nnal_amd._lib import LossT, check
    torch = sess.torch
    n = x.shape[0]
    kind = losses.KINDS[(hy or {}).get('loss_name', 'CE')]
    lab = np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)
    t = sess.to_device(x.reshape(n, -1), torch.float32)
    labd = sess.to_device(lab, torch.int32)
    keep = dict(cw=sess.to_device(np.asarray(hy['bin_class_weights'], np.float32), torch.float32) if (hy or {}).get('bin_class_weights') else None,
                sw=sess.to_device(sw, torch.float32) if sw is not None else None,
                tg=sess.to_device(y, torch.float32) if kind != losses.CE else None,
                old=sess.to_device(np.asarray(lwf[0], np.float32), torch.float32) if lwf else None)
    ptr = lambda v: v.data_ptr() if v is not None else None      # noqa: E731
    gamma = (hy or {}).get('focal_gamma')
    L = LossT(kind, -1. if gamma is None else gamma, (hy or {}).get('q', Q), lwf[2] if lwf else 1., ptr(keep['cw']), ptr(keep['sw']),
              ptr(keep['tg']), ptr(keep['old']))
    g = sess.empty((m.num_params,), torch.float32)
    post = sess.empty((m.nclass, n), torch.float32)
    stats = sess.empty((3,), torch.float64)
    arr = (C.c_int32 * 1)()
    sess.bind_stream()
    check(m.lib.alq_param_grads_loss(m._m, C.c_void_p(t.data_ptr()), n, C.c_void_p(labd.data_ptr()), C.byref(L), loss_scale, lwf_scale,
                                     1., 0, 0, arr, 0, C.c_void_p(g.data_ptr()), C.c_void_p(post.data_ptr()), C.c_void_p(stats.data_ptr())))
    rows = sess.empty((n * m.nclass,), torch.float32)
    e = C.c_int64()
    check(m.lib.alq_model_debug_copy(m._m, len(m.layers) - 1, 1, n, C.c_void_p(rows.data_ptr()), C.byref(e)))
    assert e.value == n * m.nclass
    stats2 = sess.empty((3,), torch.float64)
    check(m.lib.alq_loss_stats(sess.ctx, C.c_void_p(post.data_ptr()), m.nclass, n, C.c_void_p(labd.data_ptr()), C.byref(L),
                               C.c_void_p(stats2.data_ptr())))
    assert torch.equal(stats, stats2)              # the statistics do not depend on the entry point
    return post.cpu().numpy(), rows.cpu().numpy().reshape(n, m.nclass), stats.cpu().numpy(), lab, g


def _rows_close(rows, ref, tag):
    """4 fp32 ulp of the row's largest entry."""
    for i in range(rows.shape[0]):
        top = np.abs(ref[i]).max()
        tol = 4 * np.spacing(np.float32(top)) if top > 0 else 0.
        err = np.abs(rows[i].astype(np.float64) - ref[i]).max()
        assert err <= tol, '%s row %d: err %.3e > %.3e (%r vs %r)' % (tag, i, err, tol, rows[i], ref[i])


@pytest.mark.parametrize('case', sorted(CASES) + ['wce+lwf', 'soft+lwf'])
def test_kernel_rows_and_statistics_vs_restatement(sess, case):
    """loss_cotangent_kernel alone: rows and statistics on the device's own posteriors against nnal_amd.losses."""
    from nnal_amd import losses
    name, _, extra = case.partition('+')
    hy = CASES[name]
    m, _, _ = _mk(sess, 'neta', 71)
    x, y, sw = _batch('neta', 21, soft=name in ('soft', 'gce'))
    sw = sw if name in ('wce', 'focal2') else None
    lwf = (np.random.RandomState(5).randn(2, 12).astype(np.float32) * 2, 0.5, 2.) if extra else None
    s, s2 = float(np.float32(1. / 9)), float(np.float32(0.5 / 12)) if extra else 0.
    post, rows, stats, lab, _ = _raw_pass(sess, m, x, y, hy, sw, lwf, s, s2)
    pt = np.where(lab == 1, post[1], post[0])
    assert pt.min() >= 0.02 and pt.max() <= 0.98, pt
    ref = losses.evaluate(post, lab, losses.KINDS[hy.get('loss_name', 'CE')], class_w=hy.get('bin_class_weights'), sample_w=sw,
                          focal_gamma=hy.get('focal_gamma'), targets=y, q=hy.get('q', Q), old_logits=lwf[0] if lwf else None,
                          T=2., loss_scale=s, lwf_scale=s2)
    _rows_close(rows, ref['rows'], case)
    for a, b in zip(stats, ref['stats']):
        assert abs(a - b) <= 1e-6 * max(abs(b), 1e-30) or a == b, (case, stats, ref['stats'])
    if name in ('wce', 'focal2'):
        assert stats[1] == 10.            # 12 samples, one unlabelled, one zero weight
    m.close()


@pytest.mark.parametrize('c,N', [(2, 12), (5, 700), (3, 16384 + 77)])
def test_loss_statistics_on_given_posteriors(sess, c, N):
    """alq_loss_stats on posteriors of the caller: one workgroup, several, and more samples than one sweep of the grid."""
    from nnal_amd import losses
    from nnal_amd._lib import LossT, check
    torch = sess.torch
    rs = np.random.RandomState(c * 1000 + N)
    z = rs.randn(c, N) * 2
    post = (np.exp(z) / np.exp(z).sum(0)).astype(np.float32)
    t = rs.rand(c, N).astype(np.float32)
    old = rs.randn(c, N).astype(np.float32)
    lab = rs.randint(-1, c, size=N).astype(np.int32)
    pd, td, od, ld = (sess.to_device(v, dt) for v, dt in ((post, torch.float32), (t, torch.float32), (old, torch.float32), (lab, torch.int32)))
    sess.bind_stream()
    for kind in (losses.CE, losses.CE_SOFT, losses.GCE):
        L = LossT(kind, -1., Q, 2., None, None, td.data_ptr(), od.data_ptr())
        out = []
        for _ in range(2):
            st = sess.empty((3,), torch.float64)
            check(sess.lib.alq_loss_stats(sess.ctx, C.c_void_p(pd.data_ptr()), c, N, C.c_void_p(ld.data_ptr()), C.byref(L), C.c_void_p(st.data_ptr())))
            out.append(st.cpu().numpy())
        np.testing.assert_array_equal(out[0], out[1])
        ref = losses.evaluate(post, lab, kind, targets=t, q=Q, old_logits=old, T=2.)['stats']
        np.testing.assert_allclose(out[0], ref, rtol=1e-6, atol=0)


def test_saturated_posteriors_give_zero_rows(sess):
    """Inputs scaled until some pt == 1.0f: zero rows there, finite values everywhere for gamma = 0.5, and those samples are
    left out of the count."""
    from nnal_amd import losses
    m, om, _ = _mk(sess, 'neta', 71)
    x, y, _ = _batch('neta', 21)
    x = x * np.float32(SAT_SCALE)
    # the chosen scale, checked with the restatement on the CPU: at least one saturated sample, at least three not
    p_cpu = om.forward(x)['posteriors']
    lab_cpu = np.where(y.sum(0) > 0, y.argmax(0), -1)
    pt_cpu = np.where(lab_cpu == 1, p_cpu[1], p_cpu[0])[lab_cpu >= 0]
    assert (pt_cpu == 1.).sum() >= 1 and (pt_cpu < 1.).sum() >= 3, pt_cpu
    hy = CASES['focal05']
    post, rows, stats, lab, g = _raw_pass(sess, m, x, y, hy, loss_scale=0.125)
    pt = np.where(lab == 1, post[1], post[0])
    sat = (pt == 1.) & (lab >= 0)
    assert sat.sum() >= 1 and ((pt < 1.) & (lab >= 0)).sum() >= 3, pt
    np.testing.assert_array_equal(rows[sat], 0.)
    assert np.isfinite(rows).all() and np.isfinite(stats).all() and bool(sess.torch.isfinite(g).all())
    ref = losses.evaluate(post, lab, losses.CE, focal_gamma=0.5, loss_scale=0.125)
    assert stats[1] == ref['stats'][1] == float(np.count_nonzero((lab >= 0) & (pt < 1.)))
    _rows_close(rows, ref['rows'], 'saturated')
    m.close()


@pytest.mark.parametrize('net', ['neta', 'netc'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_loss_and_gradients_vs_autograd(sess, net, case):
    """mean_loss / mean_loss_grad (batch_eval(..., 'loss'), NN.add_loss_grad) follow the model's objective."""
    hy = CASES[case]
    m, om, _ = _mk(sess, net, 72, **hy)
    soft = case in ('soft', 'gce')
    x, y, sw = _batch(net, 22, soft=soft)
    sw = None if soft else sw
    l_ref, g_ref = _oracle(om, hy, x, y, sw)
    l_dev = m.mean_loss(x, None, targets=y, input_weights=sw)
    g_dev = m.mean_loss_grad(x, None, targets=y, input_weights=sw)
    print('%s %s: loss %.8f vs %.8f' % (net, case, l_dev, l_ref))
    assert abs(l_dev - l_ref) <= 2e-5 * max(1., abs(l_ref)), (l_dev, l_ref)
    _close(g_dev, g_ref, name='%s %s' % (net, case))
    # the sess.run spelling reads the same objective
    fd = {m.x: x, m.y_: y, m.keep_prob: 1.}
    if sw is not None:
        fd[m.input_weights] = sw
    assert sess.run(m.loss, feed_dict=fd) == l_dev
    with pytest.raises(NotImplementedError):
        m.hess_vecp(x, np.zeros(12, np.int32), np.zeros(m.num_params, np.float32))
    m.close()


def test_split_independence_of_the_weighted_focal_step(sess):
    """21 samples in passes of 8 against one pass of 32: the divisor is the whole batch's count of non-zero weights."""
    hy = dict(CASES['focal2'], learning_rate=0.05)
    x, y, sw = _batch('neta', 23, n=21)
    sw[19] = 1.
    sw[10] = 0.               # a zero weight in the second pass
    out = []
    for mb in (8, 32):
        m, om, _ = _mk(sess, 'neta', 73, max_batch=mb, **hy)
        m.get_optimizer()
        loss = sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1., m.input_weights: sw})
        out.append((loss, {n: [a.copy() for a in m.var_dict[n]] for n in m.var_names}, m, om))
    (l8, w8, m8, om8), (l32, w32, m32, _) = out
    assert abs(l8 - l32) <= 2e-6 * max(1., abs(l32)), (l8, l32)
    for n in w8:
        for a, b in zip(w8[n], w32[n]):
            np.testing.assert_allclose(a, b, rtol=0, atol=2e-6 * max(np.abs(b).max(), 0.05))
    ref = _TorchStep(om8, hy, 0.05)
    l_ref = ref.step(x, y, sw)
    assert abs(l8 - l_ref) <= 2e-5 * max(1., abs(l_ref)), (l8, l_ref)
    _weights_close(m8, om8, 2e-5, 0.05, 'split 8')
    m8.close()
    m32.close()


def _sched(t):
    from nnal_amd import NN_extended
    return NN_extended.exponential_decay(0.002, t, 0.1)


STEPS = {
    'sgd_focal': (dict(CASES['focal2'], optimizer_name='SGD', learning_rate=0.003), 0.003, 2e-5, False),
    'adam_soft': (dict(CASES['soft'], optimizer_name='Adam', beta1=0.8, beta2=0.99, learning_rate=0.002), 0.002, 5e-4, True),
    'rmsprop_m0': (dict(CASES['wce'], optimizer_name='RMSProp', decay=0.9, momentum=0., epsilon=1e-10, learning_rate=0.002), 0.002, 5e-4, False),
    'rmsprop_m05': (dict(CASES['wce'], optimizer_name='RMSProp', decay=0.9, momentum=0.5, epsilon=1e-10, lr_schedule=_sched), _sched, 5e-4, False),
}


@pytest.mark.parametrize('net', ['neta', 'netc'])
@pytest.mark.parametrize('tag', sorted(STEPS))
def test_five_train_steps_vs_torch_restatement(sess, net, tag):
    """get_optimizer() from the hypers, five sess.run(model.train_step): losses and every weight against the restatement."""
    hy, lr, bound, soft = STEPS[tag]
    m, om, _ = _mk(sess, net, 74, **hy)
    m.get_optimizer()
    ref = _TorchStep(om, hy, lr)
    for step in range(5):
        x, y, sw = _batch(net, 30 + step, soft=soft)
        fd = {m.x: x, m.y_: y, m.keep_prob: 1.}
        if not soft:
            fd[m.input_weights] = sw
        l_dev = sess.run(m.train_step, feed_dict=fd)
        l_ref = ref.step(x, y, None if soft else sw)
        assert abs(l_dev - l_ref) <= 2e-5 * max(1., abs(l_ref)), (step, l_dev, l_ref)
    _weights_close(m, om, bound, lr(0) if callable(lr) else lr, '%s %s' % (net, tag))
    m.close()


@pytest.mark.parametrize('case', [None, 'focal2'])
def test_lwf_steps_vs_autograd(sess, case):
    """sess.run(model.LwF_train_step, ...) for three steps with lambda_o = 0.5, T = 2.  The step size keeps the three steps a
    descent (loss below 2): on a diverging trajectory the logits spread past 87, posteriors underflow fp32 and pi, which the
    kernel forms from them, is no longer softmax(z / T)."""
    from nnal_amd import model_utils
    hy = dict(CASES[case], learning_rate=LWF_LR) if case else None
    m, om, _ = _mk(sess, 'neta', 75, **(hy or {}))
    if hy:
        m.get_optimizer()
    else:
        m.get_optimizer(LWF_LR, [], 'SGD')
    model_utils.get_LwF(m)
    ref = _TorchStep(om, hy, LWF_LR)
    for step in range(3):
        x, y, _ = _batch('neta', 40 + step)
        old = np.random.RandomState(50 + step).randn(2, 12).astype(np.float32)
        l_dev = sess.run(m.LwF_train_step, feed_dict={m.x: x, m.y_: y, m.y__: old, m.lambda_o: 0.5, m.T: 2., m.keep_prob: 1.})
        l_ref = ref.step(x, y, None, (old, 0.5, 2.))
        assert l_ref < 2.
        assert abs(l_dev - l_ref) <= 2e-5 * max(1., abs(l_ref)), (step, l_dev, l_ref)
    _weights_close(m, om, 2e-5, LWF_LR, 'LwF %s' % case)
    m.close()


def test_lwf_with_lambda_zero_is_the_train_step(sess):
    """lambda_o = 0 reproduces train_step bit for bit: losses and weights."""
    from nnal_amd import model_utils
    res = []
    for lwf in (False, True):
        m, _, _ = _mk(sess, 'neta', 76)
        m.get_optimizer(0.02, [], 'SGD')
        model_utils.get_LwF(m)
        losses_ = []
        for step in range(2):
            x, y, _ = _batch('neta', 60 + step)
            fd = {m.x: x, m.y_: y, m.keep_prob: 1.}
            if lwf:
                fd.update({m.y__: np.random.RandomState(3).randn(2, 12), m.lambda_o: 0., m.T: 2.})
            losses_.append(sess.run(m.LwF_train_step if lwf else m.train_step, feed_dict=fd))
        res.append((losses_, m.flat_params()))
        m.close()
    assert res[0][0] == res[1][0]
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_default_objective_is_unchanged(sess):
    """A model built without hypers steps on alq_param_grads mode 1, as before: its loss and weights equal the entry point called
    directly plus alq_sgd_step, bit for bit; so does an NN_extended.CNN built without training keywords."""
    from nnal_amd import NN_extended
    from nnal_amd._lib import check
    torch = sess.torch
    x, y, _ = _batch('netc', 61)
    lab = np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)
    m, _, pars = _mk(sess, 'netc', 77)
    t = sess.to_device(x.reshape(12, -1), torch.float32)
    g, _, l = m.param_grads_device(t, 12, 1, labels=lab, loss_scale=1. / 12, per_sample=False, want_loss=True)
    theta = sess.to_device(m.flat_params(), torch.float32)
    check(sess.lib.alq_sgd_step(sess.ctx, C.c_void_p(theta.data_ptr()), C.c_void_p(g.data_ptr()), m.num_params, 0.05))
    want_loss, want = float(l.item()) * 12 / 12, theta.cpu().numpy()
    m.close()
    ld, in_shape, sk = NETS['netc']
    for make in (lambda: _mk(sess, 'netc', 77)[0], lambda: NN_extended.CNN(in_shape, ld, 'plain', list(sk), sess=sess, max_batch=16, activation='ReLU')):
        m = make()
        m.set_weights(pars)
        assert m._obj is None
        m.get_optimizer(0.05, [], 'SGD')
        assert m.train_on_batch(x, y) == want_loss
        np.testing.assert_array_equal(m.flat_params(), want)
        m.close()


def test_masks_under_rmsprop_and_state_across_set_weights(sess):
    """train_layers and a PFT mask multiply the gradient before the step: with momentum 0 a masked parameter keeps its bits under
    RMSProp; the slots persist across set_weights like Adam's."""
    hy = dict(CASES['wce'], optimizer_name='RMSProp', momentum=0., learning_rate=0.01)
    m, om, pars = _mk(sess, 'neta', 78, **hy)
    m.train_layers = ['conv2']
    m.get_optimizer()
    assert m.train_layers == ['conv2']
    x, y, sw = _batch('neta', 62)
    before = {n: [a.copy() for a in m.var_dict[n]] for n in m.var_names}
    ref = _TorchStep(om, hy, 0.01, ['conv2'])
    m.train_on_batch(x, y, input_weights=sw)
    ref.step(x, y, sw)
    for n in m.var_names:
        for a, b in zip(m.var_dict[n], before[n]):
            assert np.array_equal(a, b) == (n != 'conv2'), n
    # a PFT mask inside the trained layer
    mask = [np.zeros(s_) for _, ws, bs in m.param_shapes for s_ in (ws, bs)]
    k = 2 * m.var_names.index('conv2')
    mask[k].reshape(-1)[::2] = 1
    m.set_PFT_mask(mask)
    mid = [a.copy() for a in m.var_dict['conv2']]
    m.train_on_batch(x, y, input_weights=sw)
    W, b = m.var_dict['conv2']
    np.testing.assert_array_equal(W.reshape(-1)[1::2], mid[0].reshape(-1)[1::2])
    np.testing.assert_array_equal(b, mid[1])
    assert not np.array_equal(W.reshape(-1)[::2], mid[0].reshape(-1)[::2])
    m.set_PFT_mask(None)
    # weights assigned between steps are what the next step updates; the rms slot is kept
    ms = m._opt['ms'].clone()
    m.set_weights(pars)
    m.train_on_batch(x, y, input_weights=sw)
    assert not sess.torch.equal(ms, m._opt['ms']) and float(m._opt['ms'].min()) < 1.
    assert np.array_equal(m.var_dict['conv1'][0], pars['conv1'][0]) and not np.array_equal(m.var_dict['conv2'][0], pars['conv2'][0])
    m.close()


def test_einval_cases_and_run_to_run_identity(sess):
    from nnal_amd import losses
    from nnal_amd._lib import AlqError, LossT, check
    torch = sess.torch
    m, _, _ = _mk(sess, 'neta', 79, max_batch=4)
    x = sess.to_device(np.random.RandomState(1).randn(6, 400).astype(np.float32), torch.float32)
    lab = sess.to_device(np.array([0, 1, 1, 0, 1, 0], np.int32), torch.int32)
    tg = sess.to_device(np.full((2, 4), 0.5, np.float32), torch.float32)
    post = sess.to_device(np.full((2, 4), 0.5, np.float32), torch.float32)
    g = sess.empty((m.num_params,), torch.float32)
    st = sess.empty((3,), torch.float64)
    arr = (C.c_int32 * 1)()
    sess.bind_stream()

    def grads(L, n=4, xs=x, labels=lab, out=g):
        return m.lib.alq_param_grads_loss(m._m, C.c_void_p(xs.data_ptr()) if xs is not None else None, n,
                                          C.c_void_p(labels.data_ptr()) if labels is not None else None, C.byref(L) if L is not None else None,
                                          0.25, 0., 1., 0, 0, arr, 0, C.c_void_p(out.data_ptr()) if out is not None else None, None, None)

    def stats(L, n=4, p=post, labels=lab, out=st):
        return m.lib.alq_loss_stats(sess.ctx, C.c_void_p(p.data_ptr()) if p is not None else None, 2, n,
                                    C.c_void_p(labels.data_ptr()) if labels is not None else None, C.byref(L) if L is not None else None,
                                    C.c_void_p(out.data_ptr()) if out is not None else None)
    ok = LossT(losses.CE, -1., Q, 1., None, None, None, None)
    bad = [LossT(losses.CE_SOFT, -1., Q, 1., None, None, None, None),             # no targets
           LossT(losses.GCE, -1., Q, 1., None, None, None, None),
           LossT(losses.GCE, -1., 0., 1., None, None, tg.data_ptr(), None),       # q == 0
           LossT(losses.CE, -1., Q, 0., None, None, None, tg.data_ptr()),         # T <= 0 with old logits
           LossT(losses.CE, -1., Q, -1., None, None, None, tg.data_ptr()),
           LossT(7, -1., Q, 1., None, None, None, None)]
    EINVAL = -1
    for L in bad:
        for rc in (grads(L), stats(L)):
            assert rc == EINVAL
            with pytest.raises(AlqError):
                check(rc)
    for rc in (grads(ok, n=0), grads(ok, n=5), grads(None), grads(ok, xs=None), grads(ok, out=None), grads(ok, labels=None),
               stats(ok, n=0), stats(None), stats(ok, p=None), stats(ok, out=None), stats(ok, labels=None)):
        assert rc == EINVAL
    assert grads(ok) == 0 and stats(ok) == 0
    th = sess.empty((5,), torch.float32)
    assert sess.lib.alq_rmsprop_step(sess.ctx, None, None, None, None, 5, 0.1, 0.9, 0., 1e-10) == EINVAL
    assert sess.lib.alq_rmsprop_step(sess.ctx, C.c_void_p(th.data_ptr()), C.c_void_p(th.data_ptr()), C.c_void_p(th.data_ptr()),
                                     C.c_void_p(th.data_ptr()), -1, 0.1, 0.9, 0., 1e-10) == EINVAL
    m.close()
    # two identical runs agree bit for bit (three steps of RMSProp on the focal objective, two passes per step)
    hy = dict(CASES['focal2'], optimizer_name='RMSProp', momentum=0.5, learning_rate=0.005)
    out = []
    for _ in range(2):
        m, _, _ = _mk(sess, 'netc', 80, max_batch=8, **hy)
        m.get_optimizer()
        ls = []
        for step in range(3):
            xb, yb, sw = _batch('netc', 90 + step)
            ls.append(m.train_on_batch(xb, yb, input_weights=sw))
        out.append((ls, m.flat_params()))
        m.close()
    assert out[0][0] == out[1][0]
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_rmsprop_kernel_vector_body_and_tail(sess):
    """alq_rmsprop_step on lengths around the 16-byte body and on a vector that starts off a 16-byte boundary."""
    from nnal_amd._lib import check
    torch = sess.torch
    f = np.float32
    rs = np.random.RandomState(4)
    sess.bind_stream()
    for n, off in ((1, 0), (7, 0), (1024 + 3, 0), (70001, 0), (515, 1)):
        th, g, ms, mom = (rs.randn(n + off).astype(f) for _ in range(4))
        ms = np.abs(ms) + f(0.5)
        d = [sess.to_device(v, torch.float32) for v in (th, g, ms, mom)]
        check(sess.lib.alq_rmsprop_step(sess.ctx, *[C.c_void_p(v.data_ptr() + 4 * off) for v in d], n, 0.01, 0.9, 0.5, 1e-10))
        th, g, ms, mom = (v[off:] for v in (th, g, ms, mom))
        ms2 = f(0.9) * ms + (f(1) - f(0.9)) * g * g
        mom2 = f(0.5) * mom + f(0.01) * g / np.sqrt(ms2 + f(1e-10))
        for dev, ref in zip((d[0], d[2], d[3]), (th - mom2, ms2, mom2)):
            np.testing.assert_allclose(dev.cpu().numpy()[off:], ref, rtol=4e-7, atol=1e-7)


def _fd(base, extra):
    out = dict(base)
    out.update(extra)
    return out


def test_hess_vecp_is_refused_on_every_route(sess):
    """A model with hypers has no Hessian-vector product: the method, the fetch, PW_NN.batch_eval(..., 'hess_vecp') and
    Influence.PW_sample_influence all raise, while 'loss' of the same batch_eval call follows the objective."""
    from nnal_amd import Influence, NN_extended, PW_NN
    from tests.test_gpu_hvp import _pw_patches, _pw_setup
    s = _pw_setup(sess, seed=51, n_inds=9)
    model = s['model']
    hy = dict(NN_extended.CNN.DEFAULT_HYPERS, focal_gamma=2.)
    tr, q = s['inds'][:8], s['inds'][8]
    # before the hypers: the product exists
    model.Hess_layers = [s['names'][-1]]
    Influence.get_hess_vec_product(model, model.Hess_layers)
    v = {h: np.ones([d.value for d in h.shape]) for h in model.v_placeholder}
    args = (model, sess, s['padded'], tr, s['patch_shape'], 4, s['stats'])
    assert len(PW_NN.batch_eval(*args, 'hess_vecp', s['mask'], v)[0]) == 2
    plain = PW_NN.batch_eval(*args, 'loss', s['mask'])[0]
    model.set_hypers(hy)
    with pytest.raises(NotImplementedError):
        PW_NN.batch_eval(*args, 'hess_vecp', s['mask'], v)
    with pytest.raises(NotImplementedError):
        PW_NN.batch_eval(*args, 'hess_vecp', s['mask'], v, _whole_set=True)
    with pytest.raises(NotImplementedError):
        Influence.PW_sample_influence(model, sess, s['padded'], s['mask'], tr, s['stats'], s['padded'], s['mask'], q, s['stats'],
                                      s['patch_shape'], 4, layers=model.Hess_layers, whole_set=True)
    x, lab = _pw_patches(sess, s, tr)
    y = np.zeros((2, 8))
    y[lab, np.arange(8)] = 1
    with pytest.raises(NotImplementedError):
        sess.run(model.hess_vecp, feed_dict=_fd({model.x: x, model.y_: y}, v))
    focal = PW_NN.batch_eval(*args, 'loss', s['mask'])[0]
    assert np.isfinite(focal).all() and (focal < plain).all()          # (1 - pt)^2 < 1 weighs every sample down
    model.close()


def test_handles_aliases_and_error_paths(sess):
    """sess.run(model.labels / model.pt / model.LwF_loss), the input_vox_weights alias, input_weights without hypers, and
    get_optimizer() without what it needs."""
    from nnal_amd import NN_extended, model_utils
    from nnal_amd.device import Handle
    x, y, sw = _batch('neta', 63)
    lab = np.where(y.sum(0) > 0, y.argmax(0), -1)
    m, _, _ = _mk(sess, 'neta', 81, **dict(CASES['wce'], learning_rate=0.001))
    fd = {m.x: x, m.y_: y, m.keep_prob: 1.}
    np.testing.assert_array_equal(sess.run(m.labels, feed_dict=fd), lab)
    post = sess.run(m.posteriors, feed_dict=fd)
    np.testing.assert_array_equal(sess.run(m.pt, feed_dict=fd), np.where(lab == 1, post[1], post[0]))
    # either attribute name switches the sample weights on
    l_w = sess.run(m.loss, feed_dict=_fd(fd, {m.input_weights: sw}))
    m.input_vox_weights = Handle('input_vox_weights')
    assert sess.run(m.loss, feed_dict=_fd(fd, {m.input_vox_weights: sw})) == l_w != sess.run(m.loss, feed_dict=fd)
    # LwF_loss is the value LwF_train_step returns, and leaves the weights alone
    m.get_optimizer()
    model_utils.get_LwF(m)
    fl = _fd(fd, {m.y__: np.random.RandomState(2).randn(2, 12), m.lambda_o: 0.5, m.T: 2., m.input_weights: sw})
    before = m.flat_params()
    l0 = sess.run(m.LwF_loss, feed_dict=fl)
    np.testing.assert_array_equal(m.flat_params(), before)
    assert sess.run(m.LwF_train_step, feed_dict=fl) == l0 and l0 > l_w
    assert not np.array_equal(m.flat_params(), before)
    m.close()
    # a model without hypers: no sample weights, no argument-free get_optimizer, LwF only after get_optimizer
    ld, in_shape, sk = NETS['neta']
    for plain in (_mk(sess, 'neta', 81)[0], NN_extended.CNN(in_shape, ld, 'plain', sess=sess, max_batch=16)):
        with pytest.raises(TypeError):
            plain.get_optimizer()
        with pytest.raises(RuntimeError):
            model_utils.get_LwF(plain)
        plain.set_weights(netspec.he_init(ld, in_shape, seed=81, bias_std=0.05))
        plain.get_optimizer(0.01, [], 'SGD')
        with pytest.raises(ValueError):
            plain.train_on_batch(x, y, input_weights=sw)
        with pytest.raises(ValueError):
            sess.run(plain.train_step, feed_dict={plain.x: x, plain.y_: y, plain.input_weights: sw})
        with pytest.raises(ValueError):
            plain.mean_loss(x, lab, input_weights=sw)
        with pytest.raises(ValueError):
            plain.mean_loss_grad(x, lab, input_weights=sw)
        plain.close()
    m = NN_extended.CNN(in_shape, ld, 'nolr', sess=sess, max_batch=16, loss_name='CE', lr_schedule=None)
    with pytest.raises(ValueError):
        m.get_optimizer()
    with pytest.raises(NotImplementedError):
        m.get_optimizer(0.1, [], 'Adagrad')
    m.close()
