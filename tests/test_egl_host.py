"""Expected-gradient-length query (NNAL.py:234-285), host side: the closed-form scores against a literal restatement of
the reference's loop, the class selection, and the new C symbol (no GPU needed)."""
import re
import subprocess

import numpy as np
import pytest


def _reference_loop(grads, sel_posteriors, T):
    """NNAL.py:255-283 as written: `grads[i][str(cls)][t]` = ||g_{cls,t}||^2 of candidate i (the reference squares and
    sums the arrays it gets back; here the sums are given).  The class list is the reference's, with a stable sort."""
    c, B = sel_posteriors.shape
    scores = np.zeros(B)
    for i in range(B):
        if c < 20:
            sel_classes = np.arange(c)
        else:
            sel_classes = np.argsort(-sel_posteriors[:, i], kind='stable')[:10]
        for j in range(len(sel_classes)):
            class_score = 0.
            for t in range(T):
                class_score += grads[i][str(sel_classes[j])][t]
                scores[i] += class_score * sel_posteriors[sel_classes[j], i]
    return scores


def _random_case(rs, c, B, T, ties=False):
    p = rs.dirichlet(np.ones(c), size=B).T                     # [c, B]
    if ties:
        p[:, 0] = 1. / c                                        # every class tied
        p[: c // 2, 1] = p[0, 1]                                # a block of tied classes
    norms = rs.rand(B, c, T) * 10. ** rs.uniform(-3, 2, size=(B, c, T))
    grads = [{str(j): norms[i, j] for j in range(c)} for i in range(B)]
    return p, norms, grads


@pytest.mark.parametrize('c', [2, 12, 21])
@pytest.mark.parametrize('ties', [False, True])
def test_egl_scores_match_the_reference_loop(c, ties):
    from nnal_amd import NNAL_tools
    rs = np.random.RandomState(100 + c + 7 * ties)
    B, T = 9, 8
    p, norms, grads = _random_case(rs, c, B, T, ties)
    classes = NNAL_tools.egl_classes(p)
    assert classes.shape == (B, c if c < 20 else 10)
    if c >= 20:
        for i in range(B):
            np.testing.assert_array_equal(classes[i], np.argsort(-p[:, i], kind='stable')[:10])
    sq = np.take_along_axis(norms, classes[:, :, None], axis=1)
    got = NNAL_tools.egl_scores(sq, p, classes)
    ref = _reference_loop(grads, p, T)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def test_egl_top10_ties_take_the_lower_class():
    from nnal_amd import NNAL_tools
    p = np.full((21, 1), 1. / 21)
    np.testing.assert_array_equal(NNAL_tools.egl_classes(p)[0], np.arange(10))


def test_egl_scores_on_a_grad_layers_subset():
    """With get_gradients(grad_layers) the reference's T = len(grad_log_posts['0']) = 2 L': only the columns of the
    subset enter, weighted T' - t' in their own order."""
    from nnal_amd import NNAL_tools
    rs = np.random.RandomState(5)
    c, B, L = 3, 6, 5
    p, norms, _ = _random_case(rs, c, B, 2 * L)
    keep = [1, 3]
    cols = [2 * t + h for t in keep for h in (0, 1)]
    sub = norms[:, :, cols]
    grads = [{str(j): sub[i, j] for j in range(c)} for i in range(B)]
    classes = NNAL_tools.egl_classes(p)
    np.testing.assert_allclose(NNAL_tools.egl_scores(sub, p, classes), _reference_loop(grads, p, len(cols)), rtol=1e-12)
    assert not np.allclose(NNAL_tools.egl_scores(norms, p, classes), NNAL_tools.egl_scores(sub, p, classes))


def test_egl_binary_scores_are_the_two_class_sum():
    """d log p0 = p1 u, d log p1 = -p0 u: the unit-cotangent form equals the two-class loop on ||g_j||^2 built from u."""
    from nnal_amd import NNAL_tools
    rs = np.random.RandomState(9)
    B, T = 11, 6
    u = rs.rand(B, T)
    p1 = rs.rand(B)
    p = np.stack([1. - p1, p1])
    grads = [{'0': p1[i] ** 2 * u[i], '1': p[0, i] ** 2 * u[i]} for i in range(B)]
    np.testing.assert_allclose(NNAL_tools.egl_binary_scores(u, p1), _reference_loop(grads, p, T), rtol=1e-12)


def test_grad_sqnorms_symbol_is_declared_and_exported():
    import os
    from nnal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'alq.h')).read()
    assert re.search(r'\bint alq_grad_sqnorms\(alq_model \*m, const float \*d_x, int N, int cls, const int32_t \*d_cls,', hdr)
    assert 'alq_grad_sqnorms' in _lib.exported_names()
    _lib.build()
    nm = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert re.search(r'\bT alq_grad_sqnorms\b', nm)
    L = _lib.lib()
    assert L.alq_prof_class_name(9) == b'gnorm'
