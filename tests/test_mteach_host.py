"""Mean-teacher consistency training without a GPU: the NumPy statements of csrc/mteach.hip (nnal_amd.mteach) against torch fp64
autograd of the reference's expressions (NN_extended.py:1337-1396, :1535-1560), the moving average, the rotation, the noise
generator, the keyword checks of NN_extended.CNN and the training loop on a stub model."""
import os

import numpy as np
import pytest
import torch

import nnal_amd  # noqa: F401
from nnal_amd import NN_extended, device, mteach, netspec

ANGLES = (0.3, -1.1, np.pi / 2, 2.0)
SIZES = ((5, 7), (16, 16), (12, 20))


def _case(spatial, N, c, seed):
    rs = np.random.RandomState(seed)
    z = torch.tensor(rs.randn(N, *spatial, c) * 1.5, dtype=torch.float64, requires_grad=True)
    zt = torch.tensor(rs.randn(N, *spatial, c) * 1.5, dtype=torch.float64)
    labels = rs.randint(0, c, size=(N,) + tuple(spatial))
    labels[rs.rand(*labels.shape) < 0.3] = -1          # unlabelled voxels: an all-zero y_ row
    return z, zt, labels


def _labelled(z, labels):
    """get_FCN_loss's cross-entropy with its non-zero-weight divisor: (scalar L, count)."""
    c = z.shape[-1]
    lab = torch.as_tensor(labels >= 0)
    logp = torch.log_softmax(z, dim=-1)
    picked = logp.gather(-1, torch.as_tensor(np.where(labels >= 0, labels, 0))[..., None])[..., 0]
    cnt = int(lab.sum())
    return -(picked * lab).sum() / cnt, cnt


def _columns(t, c):
    return t.detach().numpy().reshape(-1, c).T


@pytest.mark.parametrize('spatial,N,c', [((5, 7), 3, 2), ((5, 7), 3, 3), ((4, 6, 5), 2, 3)])
def test_l2_rows_and_value_vs_autograd(spatial, N, c):
    z, zt, labels = _case(spatial, N, c, 3 + c + len(spatial))
    coeff, V = 0.37, int(np.prod(spatial))
    p, q = torch.softmax(z, -1), torch.softmax(zt, -1)
    L, cnt = _labelled(z, labels)
    if len(spatial) == 2:
        cons = ((p - q) ** 2).mean(3).mean((1, 2))          # the reference's literal axes
    else:
        cons = ((p - q) ** 2).mean(-1).mean((1, 2, 3))      # the generalisation: class axis last, all spatial axes
    loss = L + coeff * cons                                 # a scalar plus a vector [N]
    rows = torch.autograd.grad(loss.sum(), z)[0].numpy().reshape(-1, c)
    res = mteach.evaluate(_columns(p, c), _columns(q, c), labels.reshape(-1), mteach.L2, loss_scale=N / cnt, cons_scale=coeff * 2. / (c * V))
    assert np.abs(res['rows'] - rows).max() <= 1e-12
    value = res['stats'][0] / res['stats'][1] + coeff * res['stats'][2] / (N * V)
    assert res['stats'][1] == cnt
    assert abs(value - float(loss.mean().detach())) <= 1e-12
    assert np.abs(res['div'].reshape(N, V).mean(1) - cons.detach().numpy()).max() <= 1e-12


@pytest.mark.parametrize('c', [2, 3])
def test_ce_measure_adds_to_the_value_only(c):
    N, spatial = 3, (5, 7)
    z, zt, labels = _case(spatial, N, c, 20 + c)
    V = 35
    p = torch.softmax(z, -1)
    L, cnt = _labelled(z, labels)
    div = -(p * torch.log_softmax(zt, -1)).sum(-1)
    res = mteach.evaluate(_columns(p, c), _columns(torch.softmax(zt, -1), c), labels.reshape(-1), mteach.CE, loss_scale=N / cnt,
                          cons_scale=0.9)
    assert abs(res['stats'][2] / (N * V) - float(div.mean().detach())) <= 1e-12
    # TF does not differentiate the labels of softmax_cross_entropy_with_logits: the gradient of sum(L + coeff * cons) is N grad L
    rows = torch.autograd.grad(N * L, z)[0].numpy().reshape(-1, c)
    assert np.abs(res['rows'] - rows).max() <= 1e-12
    assert not res['cons_rows'].any()


def test_ema_closed_form():
    rs = np.random.RandomState(2)
    theta, shadow0 = rs.randn(1000).astype(np.float32), rs.randn(1000).astype(np.float32)
    decay, K = 0.9, 25
    s = shadow0.copy()
    for _ in range(K):
        s = mteach.ema_step(s, theta, decay)
        assert s.dtype == np.float32
    want = theta.astype(np.float64) + (shadow0.astype(np.float64) - theta) * float(np.float32(1) - (np.float32(1) - np.float32(decay))) ** K
    # each step rounds three fp32 operations on values below max(|shadow|, |theta|) = m: at most 1.5 ulp(m) a step, damped by decay
    m = max(np.abs(theta).max(), np.abs(shadow0).max())
    assert np.abs(s - want).max() <= 1.5 * 2. ** -23 * m / (1. - decay)
    assert np.array_equal(mteach.ema_step(theta, theta, 0.5), theta)


def test_rotation_exact_cases():
    rs = np.random.RandomState(0)
    img = rs.randn(2, 16, 16, 3)
    assert np.array_equal(mteach.perturb(img, angle=0.)[0], img)
    got = mteach.perturb(img, angle=np.pi / 2)[0]
    assert np.array_equal(got, np.rot90(img, 1, axes=(1, 2)))          # counter-clockwise
    with pytest.raises(ValueError):
        mteach.perturb(rs.randn(1, 4, 4, 4, 1), angle=0.3)


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('angle', ANGLES)
def test_rotation_cases_have_no_rounding_tie(size, angle):
    """The cases the device test compares exactly: no source coordinate within 1e-3 of a half-integer, most pixels inside."""
    H, W = size
    ys, xs = mteach.rotation_sources(H, W, angle)
    assert ys.dtype == np.float32 and xs.dtype == np.float32
    for v in (ys, xs):
        frac = np.abs(v.astype(np.float64) - np.floor(v.astype(np.float64)) - 0.5)
        assert frac.min() > 1e-3
    iy, ix, inside = mteach.rotation_indices(H, W, angle)
    assert 0.6 <= inside.mean() <= 1.0
    # the gather against a pixel-by-pixel loop
    img = np.random.RandomState(1).randn(1, H, W, 2)
    got = mteach.perturb(img, angle=angle)[0]
    for y in range(H):
        for x in range(W):
            want = img[0, iy[y, x], ix[y, x]] if inside[y, x] else 0.
            assert np.array_equal(got[0, y, x], want * np.ones(2))


def test_noise_moments_and_batch_split():
    n = 2 ** 16
    z = mteach.noise(1, [0], n)[0]
    assert abs(z.mean()) <= 4. / np.sqrt(n)
    assert abs(z.var() - 1.) <= 4. * np.sqrt(2. / n)
    assert np.abs(z).max() <= 5.77
    u1, u2 = mteach.noise_uniforms(1, [0], n)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    x = np.random.RandomState(3).randn(5, 6, 4, 2).astype(np.float32)
    whole = mteach.perturb(x, 0.3, seed=9, first_sample=10, angle=0.3)[0]
    parts = np.concatenate([mteach.perturb(x[:2], 0.3, seed=9, first_sample=10, angle=0.3)[0],
                            mteach.perturb(x[2:], 0.3, seed=9, first_sample=12, angle=0.3)[0]])
    assert np.array_equal(whole, parts)
    assert not np.array_equal(mteach.noise(1, [0], 8), mteach.noise(2, [0], 8))
    assert not np.array_equal(mteach.noise(1, [0], 8), mteach.noise(1, [1], 8))


def test_mean_teacher_keyword_checks_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was opened')
    monkeypatch.setattr(device, 'default_session', no_device)
    monkeypatch.setattr(NN_extended, 'default_session', no_device)
    ld, sk = netspec.net_c_2d_dense(2)
    ld3, sk3 = netspec.net_c_dense(2)
    with pytest.raises(AssertionError, match='the device was opened'):      # a valid mean-teacher model goes on to the device
        NN_extended.CNN((16, 16, 1), ld, 'm', sk, MT_SSL=True, output_perturbation_measure='L2', rotation_angle=0.2,
                        Gaussian_noise_std=0.1, max_cons_coeff=1., rampup_length=10, MT_ema_decay_schedule=lambda t: 0.99)
    with pytest.raises(ValueError):
        NN_extended.CNN((16, 16, 1), ld, 'm', sk, MT_SSL=True, output_perturbation_measure='KL')
    with pytest.raises(ValueError):
        NN_extended.CNN((8, 8, 8, 1), ld3, 'm', sk3, MT_SSL=True, rotation_angle=0.2)
    with pytest.raises(ValueError):
        NN_extended.CNN((16, 16, 1), ld, 'm', sk, MT_SSL=True, MT_ema_decay_schedule=0.99)
    for kw in (dict(AU_4U=True), dict(AU_4L=True), dict(regularizer='L2')):
        with pytest.raises(NotImplementedError):
            NN_extended.CNN((16, 16, 1), ld, 'm', sk, MT_SSL=True, **kw)
    with pytest.raises(NotImplementedError):          # an fc head
        NN_extended.CNN((8, 8, 1), {'c1': ['conv', [4, [3, 3]], 'MA'], 'f': ['fc', [2]]}, 'm', MT_SSL=True)
    assert mteach.cons_coeff(0, 40, 2.) == pytest.approx(2. * np.exp(-5.))
    assert mteach.cons_coeff(40, 40, 2.) == 2.


# ------------------------------------------------------------------------------------------ train() on a stub
class _Stub(object):
    """model + sess in one: every run is logged; a train_step advances global_step."""
    class_num = nclass = 2
    dropout_rate, dropout_layers = 0.25, [1]

    def __init__(self, mt):
        for nme in ('x', 'keep_prob', 'y_', 'posteriors', 'loss', 'train_step', 'ema_apply'):
            setattr(self, nme, device.Handle(nme))
        self.MT_SSL = mt
        self.global_step = 0
        self.log, self.saved = [], []
        if mt:
            self.teacher = _Stub(False)
            self.teacher.save_weights = lambda path: (self.saved.append(os.path.basename(path)), open(path, 'w').close())

    def save_weights(self, path):
        self.saved.append(os.path.basename(path))
        open(path, 'w').close()

    def run(self, fetch, feed_dict=None):
        self.log.append((fetch.name, self.global_step, None if feed_dict is None else feed_dict.get(self.keep_prob)))
        if fetch.name == 'train_step':
            assert feed_dict[self.teacher.keep_prob] == 0.75 if self.MT_SSL else True
            self.global_step += 1
        elif fetch.name == 'ema_apply':
            assert feed_dict is None
        elif fetch.name == 'loss':
            return 1. / (1 + self.global_step)
        elif fetch.name == 'posteriors':
            x = feed_dict[self.x]
            p1 = (x[..., 0] > 0).astype(np.float64)
            return np.stack([1. - p1, p1], axis=-1)


@pytest.mark.parametrize('mt', [True, False])
def test_train_loop_on_a_stub_model(tmp_path, mt):
    st = _Stub(mt)
    rs = np.random.RandomState(0)

    def gen():
        x = rs.randn(2, 4, 4, 1)
        lab = (x[..., 0] > 0.2).astype(int)
        return x, (lab[..., None] == np.arange(2)).astype(np.float32)
    NN_extended.CNN.train(st, st, 4, gen, [[['av_loss', 'F1'], gen, 3, 'F1']], eval_step=2, save_path=str(tmp_path))
    steps = [e for e in st.log if e[0] in ('train_step', 'ema_apply')]
    want = [(nme, k + (nme == 'ema_apply'), 0.75 if nme == 'train_step' else None) for k in range(4)
            for nme in (('train_step', 'ema_apply') if mt else ('train_step',))]
    assert steps == want                                                     # train_step before ema_apply, four iterations
    evals = [e for e in st.log if e[0] == 'loss']
    assert [e[1] for e in evals] == [0] * 3 + [2] * 3 and all(e[2] == 1. for e in evals)      # at steps 0 and eval_step, 3 batches each
    first = [e[0] for e in st.log][:7]
    assert first[:6] == ['loss', 'posteriors'] * 3 and first[6] == 'train_step'      # the evaluation comes before the step
    assert st.valid_metrics_0['av_loss'] == [1., 1. / 3] and len(st.valid_metrics_0['F1']) == 2
    for nme in ('av_loss_0.txt', 'F1_0.txt'):
        assert len(np.loadtxt(str(tmp_path / nme))) == 2
    ext = os.path.splitext(st.saved[0])[1]
    assert set(st.saved) >= {'model_pars' + ext} | ({'teacher_pars' + ext} if mt else set())
    assert ('max_valid_iter.txt' in os.listdir(str(tmp_path))) == ('max_model_pars' + ext in st.saved)
    # a second call resumes the metric lists from the files
    st2 = _Stub(mt)
    st2.global_step = 4
    NN_extended.CNN.train(st2, st2, 4, gen, [[['av_loss', 'F1'], gen, 3, 'F1']], eval_step=2, save_path=str(tmp_path))
    assert len(st2.valid_metrics_0['F1']) == 2 and not st2.log
