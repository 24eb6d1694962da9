"""The dense CRF's host side (no GPU): the symbols of csrc/dcrf.hip, and nnal_amd.dcrf - the NumPy restatement of the model that
every device test is held against - checked against a closed form, against its own structure and against a literal
transcription of the reference's unary lines; then the facts about the test scenes that keep the device tests' exclusion lists
empty."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dcrf_cases as dc


@pytest.fixture(scope='module')
def dcrf():
    import nnal_amd  # noqa: F401
    from nnal_amd import dcrf
    return dcrf


# ------------------------------------------------------------------------------------------------ the symbols
def test_dcrf_symbols_are_declared_and_exported():
    from nnal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'alq.h')).read()
    assert re.search(r'\bsize_t alq_dcrf_work_bytes\(const int64_t dims\[3\]\);', hdr)
    assert re.search(r'\bint alq_dcrf2d\(alq_ctx \*ctx, const float \*d_post, const float \*d_img, const int64_t dims\[3\], '
                     r'const alq_dcrf_params \*par,\s+float \*d_q1, uint8_t \*d_map, void \*d_work\);', hdr)
    assert 'PW_analyze_results.py:539-591' in hdr
    for sym in ('alq_dcrf_work_bytes', 'alq_dcrf2d'):
        assert sym in _lib.exported_names()
    _lib.build()
    nm = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for sym in ('alq_dcrf_work_bytes', 'alq_dcrf2d'):
        assert re.search(r'\bT %s\b' % sym, nm)
    src = open(os.path.join(_lib._HERE, 'csrc', 'build.sh')).read()
    assert len(re.findall(r'\bdcrf\b', src)) == 2                                  # the compile list and the link list
    L = _lib.lib()
    assert L.alq_dcrf_work_bytes((_lib.C.c_int64 * 3)(3, 83, 45)) == 20 * 3 * 83 * 45
    assert L.alq_dcrf_work_bytes((_lib.C.c_int64 * 3)(3, 0, 45)) == 0
    assert L.alq_dcrf_work_bytes((_lib.C.c_int64 * 3)(8, 16384, 16384)) == 0       # 2^31 pixels
    assert _lib.C.sizeof(_lib.DcrfParams) == 32


# ------------------------------------------------------------------------------------------------ the restatement
def test_two_pixels_against_the_closed_form(dcrf):
    """A 1 x 2 image: both pixels see each other at column distance 1, so per kernel the row sums are 1 + k for both and
    K~ = [[1, k], [k, 1]] / (1 + k) with k_smooth = exp(-1/2), k_app = exp(-(1/25 + (a - b)^2) / 2).  Two iterations by hand."""
    a, b = 0.3, 1.1
    p = [0.8, 0.35]
    ks = math.exp(-0.5)
    ka = math.exp(-0.5 * (1. / 25. + (a - b) ** 2))
    U = [[float(np.float32(1. + math.log(v))) for v in p], [float(np.float32(-math.log(v))) for v in p]]      # [label][pixel]

    def softmax2(e0, e1):
        mx = max(e0, e1)
        z0, z1 = math.exp(e0 - mx), math.exp(e1 - mx)
        return z0 / (z0 + z1), z1 / (z0 + z1)

    Q = [softmax2(-U[0][i], -U[1][i]) for i in range(2)]                                                       # [pixel][label]
    want = [Q]
    for _ in range(2):
        new = []
        for i in range(2):
            j = 1 - i
            e = []
            for lab in range(2):
                fs = (Q[i][lab] + ks * Q[j][lab]) / (1. + ks)
                fa = (Q[i][lab] + ka * Q[j][lab]) / (1. + ka)
                e.append(-U[lab][i] + 20. * fs + 30. * fa)
            new.append(softmax2(*e))
        Q = new
        want.append(Q)
    got = dcrf.meanfield_host(np.array([p]), np.array([[a, b]]), niter=2)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.shape == (2, 2) and g.dtype == np.float64
        np.testing.assert_allclose(g, np.array(w).T, rtol=0, atol=1e-14)
    got_w = dcrf.meanfield_host(np.array([p]), np.array([[a, b]]), niter=2, window='cutoff')
    for g, w in zip(got_w, want):
        np.testing.assert_allclose(g, np.array(w).T, rtol=0, atol=1e-14)
    assert dcrf.map_host(np.array([p]), np.array([[a, b]]), niter=2).tolist() == [[int(want[2][0][1] > want[2][0][0]),
                                                                                  int(want[2][1][1] > want[2][1][0])]]


def test_zero_compatibilities_leave_the_unary_softmax(dcrf):
    _, img, post = dc.scene(24, 40, 5)
    for window in (None, 'cutoff'):
        Q = dcrf.meanfield_host(post.copy(), img, niter=3, window=window, params=dict(compat_smooth=0., compat_app=0.))
        U = dcrf.unary(post.copy()).astype(np.float64)
        want = np.exp(-U) / np.exp(-U).sum(axis=0)
        assert len(Q) == 4
        for q in Q:
            np.testing.assert_allclose(q, want, rtol=0, atol=1e-15)


def test_normalised_kernels_are_symmetric_with_unit_top_eigenvalue(dcrf):
    """K~ = D^-1/2 K D^-1/2 with D = diag(row sums of K).  On a constant image both kernels are symmetric, and where every pixel has
    the same row sum (1 x 2, 2 x 2) the row sums of K~ are 1, at most 1 + 1e-12.  On a larger constant image the plain row sums
    of K~ are NOT bounded by 1 - a centre pixel's neighbours at the border have smaller D (three pixels in a row, sdims 1:
    the middle row sums to 1.0697) - what holds there is the weighted form K~ sqrt(D) = sqrt(D), i.e. sum_j K~_ij sqrt(D_j / D_i)
    = 1, and with it a largest eigenvalue of exactly 1: both asserted to 1e-12."""
    for shape in ((1, 2), (2, 2)):
        flt, _ = dcrf.make_filter(np.full(shape, 0.7))
        for Kt in flt.matrices():
            np.testing.assert_array_equal(Kt, Kt.T)
            assert Kt.sum(axis=1).max() <= 1. + 1e-12 and Kt.sum(axis=1).min() >= 1. - 1e-12
    flt, _ = dcrf.make_filter(np.full((1, 3), 0.7))
    assert abs(flt.matrices()[0].sum(axis=1)[1] - 1.0697) < 1e-4
    flt, _ = dcrf.make_filter(np.full((9, 13), -1.25))
    for (K, n), Kt in zip(flt.K, flt.matrices()):
        np.testing.assert_allclose(Kt, Kt.T, rtol=0, atol=1e-16)
        assert np.all(np.diag(K) == 1.)
        rootd = 1. / n
        np.testing.assert_allclose(Kt @ rootd / rootd, np.ones(len(n)), rtol=0, atol=1e-12)
        ev = np.linalg.eigvalsh(Kt)
        assert ev.max() <= 1. + 1e-12 and ev.max() >= 1. - 1e-12 and ev.min() >= -1e-12


def test_unary_is_the_reference_lines_literally(dcrf):
    """PW_analyze_results.py:549-553 transcribed: the guard mutates the caller's array, label 0 gets 1 + log p."""
    _, img, post = dc.scene(24, 40, 5)
    post = post.copy()
    assert (post == 0).sum() == 5
    mine = post.copy()
    # -- the reference's lines
    post_map = post
    post_map[post_map == 0] += 1e-10
    post_map = -np.log(post_map)
    U = np.float32(np.array([1 - post_map, post_map]))
    U = U.reshape((2, -1))
    # --
    got = dcrf.unary(mine)
    assert got.dtype == np.float32 and got.shape == (2, 24 * 40)
    np.testing.assert_array_equal(got, U)
    np.testing.assert_array_equal(mine, post)                      # the same in-place guard on the caller's array
    assert (mine == 1e-10).sum() == 5 and (mine == 0).sum() == 0
    np.testing.assert_array_equal(got[0], np.float32(1. + np.log(mine.ravel())))       # the quirk: not -log(1 - p)
    q0 = dcrf.meanfield_host(dc.scene(24, 40, 5)[2].copy(), img, niter=0)
    assert len(q0) == 1
    np.testing.assert_allclose(q0[0][1], 1. / (1. + np.exp(U[1].astype(np.float64) - U[0])), rtol=0, atol=1e-15)
    through = dc.scene(24, 40, 5)[2].copy()
    dcrf.map_host(through, img, niter=0)
    assert (through == 1e-10).sum() == 5                           # meanfield_host / map_host mutate as the reference does


def test_cutoff_windows_against_all_pairs(dcrf):
    """fp64, scene (80, 48, 11), five iterations: the windows 6 / 29 drop at most 2^-24 of a kernel's peak; 1.5e-7 in Q."""
    assert dcrf.window_radius(1.) == 6 and dcrf.window_radius(5.) == 29
    s = (80, 48, 11)
    full = dc.marginals(*s)
    cut = dc.marginals(*s, window='cutoff')
    diff = max(float(np.abs(a - b).max()) for a, b in zip(full, cut))
    print('cut-off vs all pairs: %.3e' % diff)
    assert diff <= 1e-6


# ------------------------------------------------------------------------------------------------ the scenes
@pytest.mark.parametrize('scene', dc.HOST_SCENES)
def test_scene_facts(scene):
    m, img, post = dc.scene(*scene)
    assert (post == 0).sum() == 5
    Q64 = dc.marginals(*scene)[5]
    Q32 = dc.marginals(*scene, dtype=np.float32)[5]
    assert Q32.dtype == np.float32
    assert int((np.abs(Q64[1] - 0.5) < 1e-2).sum()) == 0                              # no near-tie
    map64, map32 = np.argmax(Q64, axis=0), np.argmax(Q32, axis=0)
    np.testing.assert_array_equal(map32, map64)
    raw = (post > 0.5).ravel()
    changed = float((map64 != raw).mean())
    err_raw, err_crf = float((raw != m.ravel()).mean()), float((map64 != m.ravel()).mean())
    print('%r: labels changed %.3f, error against m %.3f -> %.3f' % (scene, changed, err_raw, err_crf))
    assert changed > 0.10
    assert 0.13 < err_raw < 0.18 and 0.015 < err_crf < 0.065


def test_device_scenes_have_no_near_ties():
    """What the device tests exclude - pixels whose fp64 Q_1 lies within the tolerance of 0.5 - is empty on every device
    shape, after one and after five iterations and under the non-default parameters; the CRF changes more than 10 % of the raw
    labels on each of them."""
    for shape, scenes in dc.GPU_SHAPES.items():
        for it in (1, 5):
            tol, dev32 = dc.tolerance(shape, it)
            q = dc.q1_stack(shape, np.float64, it)
            assert int((np.abs(q - 0.5) <= tol).sum()) == 0, (shape, it)
            assert tol < 2e-4
        raw = dc.stacked(shape, 'post') > 0.5
        assert float(((dc.q1_stack(shape, np.float64, 5) > 0.5) != raw).mean()) > 0.10, shape
    for shape in ((1, 40, 56), (3, 83, 45)):
        tol, _ = dc.tolerance(shape, dc.OTHER_NITER, dc.OTHER_NITER, dc.OTHER_PARAMS)
        q = dc.q1_stack(shape, np.float64, dc.OTHER_NITER, dc.OTHER_NITER, dc.OTHER_PARAMS)
        assert int((np.abs(q - 0.5) <= tol).sum()) == 0
