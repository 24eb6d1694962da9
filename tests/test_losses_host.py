"""nnal_amd.losses (the fp64 restatement of csrc/loss.hip's objectives) against torch fp64 autograd, the learning-rate
schedules against their closed forms, and the keyword checks of NN_extended.CNN.  No GPU."""
import numpy as np
import pytest
import torch

import nnal_amd  # noqa: F401
from nnal_amd import NN_extended, losses

RTOL = 1e-12


def _softmax(z):
    return torch.softmax(z, dim=0)


def _check(z, total, res, stats_ref):
    """rows = d total / dz (autograd, [c, N] -> [N, c]) and the three statistics, to 1e-12 relative."""
    ref = torch.autograd.grad(total, z)[0].numpy().T
    scale = np.abs(ref).max()
    assert np.abs(res['rows'] - ref).max() <= RTOL * scale, np.abs(res['rows'] - ref).max() / scale
    for a, b in zip(res['stats'], stats_ref):
        assert abs(a - b) <= RTOL * max(1., abs(b)), (res['stats'], stats_ref)


@pytest.mark.parametrize('gamma', [None, 0.5, 2.])
def test_weighted_focal_ce_vs_autograd(gamma):
    c, N = 2, 7
    rs = np.random.RandomState(1)
    z = torch.tensor(rs.randn(c, N) * 1.5, dtype=torch.float64, requires_grad=True)
    labels = np.array([0, 1, 1, -1, 0, 1, 0])                 # sample 3 is unlabelled
    cw = np.array([0.3, 1.7])
    sw = np.array([1.0, 0.5, 0.0, 2.0, 1.5, 0.25, 0.75])      # sample 2 has a zero weight
    s = 0.37
    p = _softmax(z)
    lab = labels >= 0
    ys = np.where(lab, labels, 0)
    pt = p[torch.as_tensor(ys), torch.arange(N)]
    w = torch.as_tensor(lab * cw[ys] * sw)
    if gamma is not None:
        w = w * (1. - pt) ** gamma                            # differentiated: TF puts no stop_gradient on the focal weights
    per = -w * torch.log(pt)
    res = losses.evaluate(p.detach().numpy(), labels, losses.CE, class_w=cw, sample_w=sw, focal_gamma=gamma, loss_scale=s)
    # hand count: 7 samples, one unlabelled, one with a zero sample weight
    assert res['stats'][1] == 5.
    _check(z, s * per.sum(), res, (float(per.sum().detach()), 5., 0.))
    np.testing.assert_array_equal(res['rows'][[2, 3]], 0.)


def test_focal_weight_zero_is_left_out_of_the_count():
    """pt == 1 under the focal term: weight 0, zero row, not counted; finite everywhere for gamma = 0.5."""
    post = np.array([[1.0, 0.25, 0.5], [0.0, 0.75, 0.5]], dtype=np.float32)
    res = losses.evaluate(post, np.array([0, 1, 0]), losses.CE, focal_gamma=0.5)
    assert res['stats'][1] == 2. and np.isfinite(res['rows']).all() and np.isfinite(res['loss']).all()
    np.testing.assert_array_equal(res['rows'][0], 0.)
    assert losses.evaluate(post, np.array([0, 1, 0]), losses.CE)['stats'][1] == 3.


@pytest.mark.parametrize('c', [2, 5])
def test_ce_softclasses_vs_autograd(c):
    N = 7
    rs = np.random.RandomState(2 + c)
    z = torch.tensor(rs.randn(c, N) * 1.5, dtype=torch.float64, requires_grad=True)
    t = rs.rand(c, N)
    t[:, :4] /= t[:, :4].sum(0)                               # some columns sum to one, the rest do not
    s = 1. / N
    p = _softmax(z)
    per = -(torch.as_tensor(t) * torch.log(p)).sum(0)
    res = losses.evaluate(p.detach().numpy(), None, losses.CE_SOFT, targets=t, loss_scale=s)
    _check(z, s * per.sum(), res, (float(per.sum().detach()), float(N), 0.))


@pytest.mark.parametrize('c', [2, 5])
def test_gce_vs_autograd_with_clipped_columns(c):
    N, q = 7, 0.7
    rs = np.random.RandomState(7 + c)
    zn = rs.randn(c, N)
    zn[:, 0] = 0.
    zn[0, 0] = 12.          # column 0: class 0 above 1 - 1e-4, the others below 1e-4 -> every entry clipped
    zn[:, 1] = 0.
    zn[c - 1, 1] = -12.     # column 1: the last class below 1e-4, the others inside
    z = torch.tensor(zn, dtype=torch.float64, requires_grad=True)
    t = rs.rand(c, N)
    t /= t.sum(0)
    p = _softmax(z)
    pn = p.detach().numpy()
    assert pn[0, 0] > 1 - 1e-4 and (pn[1:, 0] < 1e-4).all() and pn[c - 1, 1] < 1e-4 and (pn[:c - 1, 1] > 1e-4).all()
    Lq = (1. - torch.clamp(p, 1e-4, 1 - 1e-4) ** q) / q
    per = (torch.as_tensor(t) * Lq).mean(0)
    res = losses.evaluate(pn, None, losses.GCE, targets=t, q=q, loss_scale=1.)
    _check(z, per.sum(), res, (float(per.sum().detach()), float(N), 0.))
    np.testing.assert_array_equal(res['rows'][0], 0.)         # clipped at both bounds: the cotangent is exactly zero
    only_last = np.zeros((c, N))
    only_last[c - 1] = 1.
    np.testing.assert_array_equal(losses.evaluate(pn, None, losses.GCE, targets=only_last, q=q)['rows'][1], 0.)
    with pytest.raises(ValueError):
        losses.evaluate(pn, None, losses.GCE, targets=t, q=0.)


@pytest.mark.parametrize('c', [2, 5])
def test_lwf_term_vs_autograd(c):
    N, T = 7, 2.
    rs = np.random.RandomState(11 + c)
    z = torch.tensor(rs.randn(c, N) * 1.5, dtype=torch.float64, requires_grad=True)
    old = rs.randn(c, N) * 2.
    labels = rs.randint(0, c, size=N)
    labels[2] = -1
    s, s2 = 1. / N, 0.5 / N
    p = _softmax(z)
    tau = torch.softmax(torch.as_tensor(old) / T, dim=0)
    per2 = -(tau * torch.log_softmax(z / T, dim=0)).sum(0)
    lab = labels >= 0
    per = -torch.as_tensor(lab * 1.) * torch.log(p[torch.as_tensor(np.where(lab, labels, 0)), torch.arange(N)])
    res = losses.evaluate(p.detach().numpy(), labels, losses.CE, old_logits=old, T=T, loss_scale=s, lwf_scale=s2)
    _check(z, s * per.sum() + s2 * per2.sum(), res, (float(per.sum().detach()), float(N - 1), float(per2.sum().detach())))


def test_schedules_closed_forms():
    for t in (0, 1, 100):
        assert NN_extended.exponential_decay(1e-3, t, 0.1) == pytest.approx(1e-3 * np.exp(-0.1 * t), rel=1e-15)
        up = np.exp(-5. * (1. - t / 40.) ** 2) if t < 40 else 1.
        assert NN_extended.sigmoid_rampup(t, 40) == pytest.approx(up, rel=1e-15)
        down = np.exp(-12.5 * (1. - (120 - t) / 30.) ** 2) if t >= 90 else 1.
        assert NN_extended.sigmoid_rampdown(t, 30, 120) == pytest.approx(down, rel=1e-15)
        assert NN_extended.sigmoid_schedule(t, 0.02, 40, 30, 120) == pytest.approx(up * down * 0.02, rel=1e-15)
    assert NN_extended.sigmoid_rampup(0, 40) == pytest.approx(np.exp(-5.))
    assert NN_extended.CNN.DEFAULT_HYPERS['lr_schedule'](1) == pytest.approx(1e-3 * np.exp(-0.1))


def test_extended_cnn_keyword_checks_need_no_device(monkeypatch):
    from nnal_amd import device

    def no_device(*a, **k):
        raise AssertionError('the device was opened')
    monkeypatch.setattr(device, 'default_session', no_device)
    monkeypatch.setattr(NN_extended, 'default_session', no_device)
    ld2 = {'c1': ['conv', [4, [3, 3]], 'MA'], 'f': ['fc', [2]]}
    ld3 = {'c1': ['conv', [4, [3, 3]], 'MA'], 'f': ['fc', [3]]}
    for kw in (dict(regularizer='L2'), dict(MT_SSL=True), dict(AU_4L=True), dict(BN_decay=0.9), dict(activation='tanh')):
        with pytest.raises(NotImplementedError):
            NN_extended.CNN((8, 8, 1), ld2, 'm', **kw)
    for kw in (dict(loss_name='hinge'), dict(optimizer_name='Adagrad'), dict(loss_name='GCE', q=0), dict(bin_class_weights=[1., 2., 3.]),
               dict(lr_schedule=0.1)):
        with pytest.raises(ValueError):
            NN_extended.CNN((8, 8, 1), ld2, 'm', **kw)
    for kw in (dict(bin_class_weights=[0.3, 1.7]), dict(focal_gamma=2.)):
        with pytest.raises(ValueError):
            NN_extended.CNN((8, 8, 1), ld3, 'm', **kw)


def test_lwf_from_fp32_posteriors_up_to_the_underflow_limit():
    """pi is formed from the fp32 posteriors.  With a logit spread of 80 every posterior is a normal fp32 number and the term
    is softmax(z / T) to fp32 rounding of p: |d log p| <= 2^-24 per entry, so log pi moves by at most 2 * 2^-24 / T.  With a
    spread of 120 the small posterior underflows, log p is held at log 1e-38 and the loss falls short of the true one by
    tau_j (spread - log(1e38)) / T: the documented limit, in figures."""
    T, c = 2., 2
    old = np.array([[0.3, -0.2], [-0.1, 0.4]])
    labels = np.array([0, 1])
    tau = torch.softmax(torch.as_tensor(old) / T, dim=0).numpy()
    for spread, exact in ((80., True), (120., False)):
        z = torch.tensor([[spread, 0.], [0., spread]], dtype=torch.float64, requires_grad=True)      # sample n: class n on top
        p32 = _softmax(z).detach().numpy().astype(np.float32)
        assert (p32.min() > 0) == exact
        per2 = -(torch.as_tensor(tau) * torch.log_softmax(z / T, dim=0)).sum(0)
        ref_rows = torch.autograd.grad(per2.sum(), z)[0].numpy().T
        res = losses.evaluate(p32, labels, losses.CE, old_logits=old, T=T, loss_scale=0., lwf_scale=1.)
        if exact:
            tol = 2 * 2. ** -24 / T
            assert np.abs(res['lwf'] - per2.detach().numpy()).max() <= tol
            assert np.abs(res['rows'] - ref_rows).max() <= tol
        else:
            held = np.log(1e38)      # -log of the floor 1e-38
            short = np.array([tau[1, 0], tau[0, 1]]) * (spread - held) / T
            np.testing.assert_allclose(per2.detach().numpy() - res['lwf'], short, rtol=1e-6)
            assert tau.min() > 0.4 and short.min() > 0.4 * (spread - held) / T > 6.      # far outside any rounding
