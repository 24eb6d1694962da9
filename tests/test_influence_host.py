"""Host logic of the influence functions (nnal_amd.Influence) over stand-ins: no GPU, no libalq compute."""
import os
import re
from collections import OrderedDict

import numpy as np

import nnal_amd  # noqa: F401
from nnal_amd import Influence, _lib


class _H(object):
    def __init__(self, name):
        self.name = name


class QuadModel(object):
    """A stand-in whose Hessian over the chosen layers is a known SPD matrix: two layers ('a': W [2, 3], b [3]; 'b': W [4, 2],
    b [4, 1]), `hess_vecp_device`-free - the evaluators reach it through PW_NN.batch_eval, which the tests rebind."""
    x, y_, keep_prob = _H('x'), _H('y_'), _H('keep_prob')

    def __init__(self):
        self.param_shapes = [('a', (2, 3), (3,)), ('b', (4, 2), (4, 1))]
        self.var_dict = OrderedDict((n, [np.zeros(w, np.float32), np.zeros(b, np.float32)]) for n, w, b in self.param_shapes)


def _spd(n, seed):
    rs = np.random.RandomState(seed)
    A = rs.randn(n, n)
    return A @ A.T / n + np.eye(n)


def test_ravel_unravel_round_trip_on_a_subset():
    m = QuadModel()
    Influence.get_hess_vec_product(m, ['b'])
    vec = np.arange(12, dtype=np.float64)
    parts = Influence.unravel_vec(m, vec)
    assert [p.shape for p in parts] == [(4, 2), (4, 1)]
    np.testing.assert_array_equal(Influence.ravel_tensors(parts), vec)
    Influence.get_hess_vec_product(m, 'all')
    vec = np.random.RandomState(0).randn(21)
    parts = Influence.unravel_vec(m, vec)
    assert [p.shape for p in parts] == [(2, 3), (3,), (4, 2), (4, 1)]
    np.testing.assert_array_equal(Influence.ravel_tensors(parts), vec)


def test_get_hess_vec_product_sets_the_attributes():
    m = QuadModel()
    Influence.get_hess_vec_product(m, 'all')
    assert m.Hess_layers == ['a', 'b'] and len(m.v_placeholder) == 4 and m.hess_vecp.model is m
    assert [[d.value for d in h.shape] for h in m.v_placeholder] == [[2, 3], [3], [4, 2], [4, 1]]
    Influence.get_hess_vec_product(m, ['b'])
    assert m.Hess_layers == ['b'] and len(m.v_placeholder) == 2 and m.hess_vecp.name == 'hess_vecp'
    assert [[d.value for d in h.shape] for h in m.v_placeholder] == [[4, 2], [4, 1]]


def _solve(monkeypatch, whole_set, layers='all'):
    m = QuadModel()
    n = 21 if layers == 'all' else 12
    Hlast, Hall = _spd(n, 1), _spd(n, 2)
    g = np.random.RandomState(3).randn(n)
    seen = []

    def fake_batch_eval(model, sess, img_dat, inds, patch_shape, batch_size, stats, varnames, mask=None, x_feed_dict={}, **kw):
        assert varnames == 'hess_vecp' and model is m
        seen.append(dict(kw))
        vec = Influence.ravel_tensors([x_feed_dict[h] for h in model.v_placeholder])
        H = Hall if kw.get('_whole_set') else Hlast
        return [Influence.unravel_vec(model, H @ vec)]

    monkeypatch.setattr(Influence.PW_NN, 'batch_eval', fake_batch_eval)
    monkeypatch.setattr(Influence, 'eval_loss_grad_q', lambda *a, **k: Influence.unravel_vec(m, g))
    t = Influence.PW_sample_influence(m, None, None, None, np.arange(40), None, None, None, 7, None, (5, 5, 1), 16, layers=layers,
                                      whole_set=whole_set)
    return m, t, g, (Hall if whole_set else Hlast), seen


def test_sample_influence_converges_to_the_solve(monkeypatch):
    """fmin_ncg stops once the mean absolute update falls below avextol = 1e-8 per entry; on an SPD quadratic its Newton step
    is a CG solve to a relative residual <= min(0.5, sqrt |g|) |g| per outer iteration, so ten iterations reach the solution to
    far below 1e-6 of its norm."""
    for layers in ('all', ['b']):
        m, t, g, H, seen = _solve(monkeypatch, True, layers)
        ref = np.linalg.solve(H, g)
        assert np.abs(t - ref).max() <= 1e-6 * np.abs(ref).max(), np.abs(t - ref).max()
        assert len(seen) >= 1 and all(k.get('_whole_set') is True for k in seen)
        assert m.loss_grad.layers == ('all' if layers == 'all' else ['b'])


def test_literal_mode_asks_for_the_last_batch_only(monkeypatch):
    """whole_set = False (the default) is the reference's behaviour: plain batch_eval(..., 'hess_vecp') calls, whose result is
    the last batch's product (PW_NN.py:532-533)."""
    m, t, g, H, seen = _solve(monkeypatch, False)
    assert len(seen) >= 1 and all('_whole_set' not in k for k in seen)
    ref = np.linalg.solve(H, g)
    assert np.abs(t - ref).max() <= 1e-6 * np.abs(ref).max()


def test_f_evaluator_is_the_objective(monkeypatch):
    m = QuadModel()
    Influence.get_hess_vec_product(m, 'all')
    H = _spd(21, 4)
    g = np.random.RandomState(5).randn(21)
    monkeypatch.setattr(Influence.PW_NN, 'batch_eval',
                        lambda model, *a, **k: [Influence.unravel_vec(model, H @ Influence.ravel_tensors([a[8][h] for h in model.v_placeholder]))])
    args = (m, None, None, None, np.arange(3))
    f = Influence.get_f_evaluator(*args, Influence.unravel_vec(m, g), (5, 5, 1), 2, None)
    fp = Influence.get_fprime_evaluator(*args, Influence.unravel_vec(m, g), (5, 5, 1), 2, None)
    hp = Influence.get_hessp_evaluator(*args, (5, 5, 1), 2, None)
    t = np.random.RandomState(6).randn(21)
    assert f.__name__ == 'eval_f'
    assert abs(f(t) - (0.5 * t @ H @ t - g @ t)) <= 1e-12 * (abs(t @ H @ t) + abs(g @ t))
    np.testing.assert_allclose(fp(t), H @ t - g, rtol=0, atol=1e-12)
    np.testing.assert_allclose(hp(None, t), H @ t, rtol=0, atol=1e-12)


def test_exported_names_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'alq.h')).read()
    names = set(re.findall(r'\b(alq_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S)))
    assert 'alq_hess_vecp' in names
    assert sorted(names) == _lib.exported_names()
