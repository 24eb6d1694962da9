"""The dense CRF on the device (csrc/dcrf.hip; GPU box): alq_dcrf2d against nnal_amd.dcrf, the fp64 all-pairs restatement of the
model, on the scenes of tests/dcrf_cases.py; then DCRF_postprocess_2D and full_model_pred_DCRF.

Tolerance of a class-1 marginal: tol = 4 x max |Q_fp32 host - Q_fp64| + 1e-6, computed here on the same input
(dcrf_cases.tolerance): the fp32 restatement's own deviation from fp64, the factor 4 for another summation order and the
hardware exp2, 1e-6 for the cut-off windows (they drop 1.5e-7 in fp64).  Labels are compared at every pixel whose fp64 marginal
lies further than tol from 0.5; on these scenes that is every pixel (test_dcrf_host.py), and at most 0.5 % may be left out."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from tests import dcrf_cases as dc  # noqa: E402
from tests.test_committee_host import Expr  # noqa: E402

GUARD = 64
SHAPES = sorted(dc.GPU_SHAPES)


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _cpar(niter, params=None):
    from nnal_amd import _lib, dcrf
    par = dcrf.make_params(**(params or {}))
    return _lib.DcrfParams((C.c_float * 2)(*par['sdims_smooth']), (C.c_float * 2)(*par['sdims_app']), par['schan'],
                           par['compat_smooth'], par['compat_app'], niter)


def _call(sess, post, img, niter, params=None, want_q=True, want_map=True, default_par=False):
    """One alq_dcrf2d call on float32 arrays [S, H, W] with guard cells (NaN / 7) around d_q1, d_map and d_work, all checked
    afterwards together with d_post and d_img being unchanged.  -> (q1 float32 [S, H, W] or None, map uint8 or None)."""
    from nnal_amd._lib import check
    torch = sess.torch
    sess.bind_stream()
    dims = (C.c_int64 * 3)(*post.shape)
    n = int(post.size)
    d_post = sess.to_device(post, torch.float32)
    d_img = sess.to_device(img, torch.float32)
    q = torch.full((GUARD + n + GUARD,), float('nan'), dtype=torch.float32, device=sess.device)
    mp = torch.full((GUARD + n + GUARD,), 7, dtype=torch.uint8, device=sess.device)
    wb = int(sess.lib.alq_dcrf_work_bytes(dims))
    assert wb == 20 * n
    work = torch.full((GUARD + wb + GUARD,), 7, dtype=torch.uint8, device=sess.device)
    par = None if default_par else C.byref(_cpar(niter, params))
    check(sess.lib.alq_dcrf2d(sess.ctx, C.c_void_p(d_post.data_ptr()), C.c_void_p(d_img.data_ptr()), dims, par,
                              C.c_void_p(q.data_ptr() + 4 * GUARD) if want_q else None,
                              C.c_void_p(mp.data_ptr() + GUARD) if want_map else None, C.c_void_p(work.data_ptr() + GUARD)))
    q, mp, work = q.cpu().numpy(), mp.cpu().numpy(), work.cpu().numpy()
    assert np.isnan(q[:GUARD]).all() and np.isnan(q[-GUARD:]).all()
    assert (mp[:GUARD] == 7).all() and (mp[-GUARD:] == 7).all()
    assert (work[:GUARD] == 7).all() and (work[-GUARD:] == 7).all()
    if not want_q:
        assert np.isnan(q).all()
    if not want_map:
        assert (mp == 7).all()
    np.testing.assert_array_equal(d_post.cpu().numpy(), post)
    np.testing.assert_array_equal(d_img.cpu().numpy(), img)
    return (q[GUARD:-GUARD].reshape(post.shape) if want_q else None, mp[GUARD:-GUARD].reshape(post.shape) if want_map else None)


_RESULTS = {}


def _device(sess, shape, niter, params=None):
    """The device's (q1, map) of a device shape, computed once per (shape, niter, params)."""
    key = (shape, niter, dc._key(params))
    if key not in _RESULTS:
        _RESULTS[key] = _call(sess, dc.stacked(shape, 'post'), dc.stacked(shape, 'img'), niter, params)
    return _RESULTS[key]


def _check_labels(got, q64, tol, what):
    """got == [q64 > 0.5] wherever |q64 - 0.5| > tol; at most 0.5 % of the pixels may be left out."""
    decided = np.abs(q64 - 0.5) > tol
    left_out = 1. - float(decided.mean())
    print('%s: %d of %d pixels within tol of a tie' % (what, int((~decided).sum()), decided.size))
    assert left_out <= 0.005, what
    np.testing.assert_array_equal(got[decided], (q64 > 0.5)[decided].astype(got.dtype), err_msg=what)


# ------------------------------------------------------------------------------------------------ marginals and labels
@pytest.mark.parametrize('niter', [1, 5])
@pytest.mark.parametrize('shape', SHAPES)
def test_marginals_and_labels_against_fp64(sess, shape, niter):
    q1, mp = _device(sess, shape, niter)
    assert q1.dtype == np.float32 and mp.dtype == np.uint8 and q1.shape == shape and mp.shape == shape
    q64 = dc.q1_stack(shape, np.float64, niter)
    tol, dev32 = dc.tolerance(shape, niter)
    dev = float(np.abs(q1.astype(np.float64) - q64).max())
    print('%r, %d iteration(s): device %.3e, fp32 host %.3e (ratio %.2f), tol %.3e' % (shape, niter, dev, dev32, dev / max(dev32, 1e-300), tol))
    assert dev <= tol
    _check_labels(mp, q64, tol, '%r niter %d' % (shape, niter))
    np.testing.assert_array_equal(mp, q1 > 0.5)                    # the label is the arg-max of the marginal returned
    if niter == 5:
        raw = dc.stacked(shape, 'post') > 0.5
        changed = float((mp.astype(bool) != raw).mean())
        print('%r: the CRF changed %.3f of the raw labels' % (shape, changed))
        assert changed > 0.10                                      # an identity or unary-only implementation fails here


@pytest.mark.parametrize('shape', SHAPES)
def test_zero_iterations_is_the_unary_softmax(sess, shape):
    q1, mp = _device(sess, shape, 0)
    q64 = dc.q1_stack(shape, np.float64, 0, niter=0)
    tol, _ = dc.tolerance(shape, 0, niter=0)
    assert float(np.abs(q1.astype(np.float64) - q64).max()) <= tol
    np.testing.assert_array_equal(mp, q1 > 0.5)
    _check_labels(mp, q64, tol, '%r niter 0' % (shape,))
    zeros = dc.stacked(shape, 'post') == 0
    assert zeros.sum() == 5 * shape[0]
    # the guarded zeros: p = 1e-10, U = float32(1 + log p, -log p), q1 = softmax(-U)_1
    u0, u1 = float(np.float32(1. + np.log(1e-10))), float(np.float32(-np.log(1e-10)))
    np.testing.assert_allclose(q1[zeros], 1. / (1. + np.exp(u1 - u0)), rtol=1e-4, atol=0)


def test_default_parameters_are_the_references(sess):
    """par = NULL selects sdims (1, 1) / (5, 5), schan 1, compatibilities 20 / 30, 5 iterations: the same bits as spelling them."""
    shape = (1, 40, 56)
    q1, mp = _call(sess, dc.stacked(shape, 'post'), dc.stacked(shape, 'img'), None, default_par=True)
    want_q, want_map = _device(sess, shape, 5)
    np.testing.assert_array_equal(q1, want_q)
    np.testing.assert_array_equal(mp, want_map)


def test_slices_are_independent_and_calls_repeat_bit_for_bit(sess):
    shape = (3, 83, 45)
    q1, mp = _device(sess, shape, 5)
    post, img = dc.stacked(shape, 'post'), dc.stacked(shape, 'img')
    again_q, again_map = _call(sess, post, img, 5)
    np.testing.assert_array_equal(again_q, q1)
    np.testing.assert_array_equal(again_map, mp)
    for s in range(3):
        one_q, one_map = _call(sess, post[s:s + 1], img[s:s + 1], 5)
        np.testing.assert_array_equal(one_q[0], q1[s], err_msg='slice %d' % s)
        np.testing.assert_array_equal(one_map[0], mp[s], err_msg='slice %d' % s)


def test_either_output_alone(sess):
    for shape in ((1, 40, 56), (2, 7, 5)):
        post, img = dc.stacked(shape, 'post'), dc.stacked(shape, 'img')
        q1, mp = _device(sess, shape, 5)
        only_q, none = _call(sess, post, img, 5, want_map=False)
        assert none is None
        np.testing.assert_array_equal(only_q, q1)
        none, only_map = _call(sess, post, img, 5, want_q=False)
        assert none is None
        np.testing.assert_array_equal(only_map, mp)
        none, only_map = _call(sess, post, img, 0, want_q=False)
        np.testing.assert_array_equal(only_map, _device(sess, shape, 0)[1])


@pytest.mark.parametrize('shape', SHAPES)
def test_other_parameters(sess, shape):
    """sdims 2 and 3 (windows 25 x 25 and 37 x 37), schan 0.5, compatibilities 5 and 10, 3 iterations: the same tol rule."""
    q1, mp = _device(sess, shape, dc.OTHER_NITER, dc.OTHER_PARAMS)
    q64 = dc.q1_stack(shape, np.float64, dc.OTHER_NITER, dc.OTHER_NITER, dc.OTHER_PARAMS)
    tol, dev32 = dc.tolerance(shape, dc.OTHER_NITER, dc.OTHER_NITER, dc.OTHER_PARAMS)
    dev = float(np.abs(q1.astype(np.float64) - q64).max())
    print('%r, other parameters: device %.3e, fp32 host %.3e, tol %.3e' % (shape, dev, dev32, tol))
    assert dev <= tol
    _check_labels(mp, q64, tol, '%r other parameters' % (shape,))
    if shape[1] * shape[2] > 100:
        assert float(np.abs(q1 - _device(sess, shape, 5)[0]).max()) > 1e-2        # the parameters reached the kernel


def test_anisotropic_scales(sess):
    """Different scales per axis (rows, columns) of both kernels, against the restatement on one scene."""
    shape, scene = (1, 40, 56), (40, 56, 3)
    params = dict(sdims_smooth=(1., 2.), sdims_app=(4., 2.5))
    q1, mp = _call(sess, dc.stacked(shape, 'post'), dc.stacked(shape, 'img'), 2, params)
    q64 = dc.marginals(*scene, niter=2, params=params)[2][1].reshape(shape)
    q32 = dc.marginals(*scene, dtype=np.float32, niter=2, params=params)[2][1].reshape(shape)
    tol = 4. * float(np.abs(q32.astype(np.float64) - q64).max()) + 1e-6
    assert float(np.abs(q1.astype(np.float64) - q64).max()) <= tol
    _check_labels(mp, q64, tol, 'anisotropic')


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch(sess):
    torch = sess.torch
    sess.bind_stream()
    shape = (2, 7, 5)
    n = 70
    d_post = sess.to_device(dc.stacked(shape, 'post'), torch.float32)
    d_img = sess.to_device(dc.stacked(shape, 'img'), torch.float32)
    q = torch.full((n,), float('nan'), dtype=torch.float32, device=sess.device)
    mp = torch.full((n,), 7, dtype=torch.uint8, device=sess.device)
    dims = (C.c_int64 * 3)(*shape)
    work = torch.full((int(sess.lib.alq_dcrf_work_bytes(dims)),), 7, dtype=torch.uint8, device=sess.device)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    L = sess.lib
    ok = _cpar(5)

    def rc(post=p(d_post), img=p(d_img), dims=dims, par=C.byref(ok), q1=p(q), m=p(mp), w=p(work)):
        return L.alq_dcrf2d(sess.ctx, post, img, dims, par, q1, m, w)

    assert rc(post=None) == -1 and rc(img=None) == -1 and rc(dims=None) == -1 and rc(w=None) == -1
    assert rc(q1=None, m=None) == -1                               # not both
    for bad in ((0, 7, 5), (2, 0, 5), (2, 7, 0), (-1, 7, 5)):
        d = (C.c_int64 * 3)(*bad)
        assert rc(dims=d) == -1
        assert L.alq_dcrf_work_bytes(d) == 0
    assert L.alq_dcrf_work_bytes(None) == 0
    huge = (C.c_int64 * 3)(8, 16384, 16384)                        # 2^31 pixels
    assert rc(dims=huge) == -1 and L.alq_dcrf_work_bytes(huge) == 0
    for niter in (-1, 65):
        assert rc(par=C.byref(_cpar(niter))) == -1
    for field, values in (('sdims_smooth', ((0., 1.), (1., -2.), (float('nan'), 1.), (1., float('inf')))),
                          ('sdims_app', ((0., 5.), (5., -1.), (float('inf'), 5.), (5., float('nan')))),
                          ('schan', (0., -1., float('nan'), float('inf'))),
                          ('compat_smooth', (float('nan'), float('inf'), -float('inf'))),
                          ('compat_app', (float('nan'), float('inf')))):
        for v in values:
            assert rc(par=C.byref(_cpar(5, {field: v}))) == -1, (field, v)
    assert rc(par=C.byref(_cpar(5, dict(sdims_app=(8., 8.))))) == -4          # ALQ_EUNSUPPORTED: the window outgrows the LDS
    torch.cuda.synchronize()
    assert bool(torch.isnan(q).all()) and bool((mp == 7).all()) and bool((work == 7).all())      # nothing was launched
    assert rc(par=C.byref(_cpar(64))) == 0 and rc(par=C.byref(_cpar(0))) == 0                    # the ends of the niter range run
    torch.cuda.synchronize()
    assert not bool(torch.isnan(q).any()) and bool((mp <= 1).all())


# ------------------------------------------------------------------------------------------------ the reference's functions
def test_dcrf_postprocess_2d(sess):
    from nnal_amd import PW_analyze_results as R, dcrf
    scene = (40, 56, 3)
    _, img, post = dc.scene(*scene)
    mine = post.copy()
    assert (mine == 0).sum() == 5
    got = R.DCRF_postprocess_2D(mine, img, sess)
    assert got.shape == (40, 56) and got.dtype.kind == 'i'
    assert (mine == 0).sum() == 0 and (mine == 1e-10).sum() == 5 and np.array_equal(mine[post != 0], post[post != 0])
    want = dcrf.map_host(post.copy(), img)
    q64 = dc.marginals(*scene)[5][1].reshape(40, 56)
    np.testing.assert_array_equal(want, q64 > 0.5)
    tol, _ = dc.tolerance((1, 40, 56), 5)
    _check_labels(got, q64, tol, 'DCRF_postprocess_2D')
    # a float32 map and the default session
    mine32 = post.astype(np.float32)
    got32 = R.DCRF_postprocess_2D(mine32, img.astype(np.float32))
    assert (mine32 == np.float32(1e-10)).sum() == 5
    _check_labels(got32, q64, tol, 'DCRF_postprocess_2D, float32')
    with pytest.raises(ValueError):
        R.DCRF_postprocess_2D(post.copy(), img[:, :-1], sess)


def test_session_wrapper(sess):
    """DeviceSession.dcrf2d: device tensors in, (labels, q1) out, `params` with niter - the same bits as the C call; a [H, W]
    dims is one slice; NumPy inputs are uploaded and the zeros of `post` replaced in the caller's array."""
    torch = sess.torch
    shape = (3, 83, 45)
    post, img = dc.stacked(shape, 'post'), dc.stacked(shape, 'img')
    want_q, want_map = _device(sess, shape, dc.OTHER_NITER, dc.OTHER_PARAMS)
    d_post = sess.to_device(post, torch.float32)
    labels, q1 = sess.dcrf2d(d_post, sess.to_device(img, torch.float32), shape, params=dict(dc.OTHER_PARAMS, niter=dc.OTHER_NITER), want_q=True)
    assert labels.dtype == torch.uint8 and q1.dtype == torch.float32 and tuple(labels.shape) == shape and tuple(q1.shape) == shape
    np.testing.assert_array_equal(q1.cpu().numpy(), want_q)
    np.testing.assert_array_equal(labels.cpu().numpy(), want_map)
    np.testing.assert_array_equal(d_post.cpu().numpy(), post)      # the device tensor is only read: its zeros stay
    mine = post[1].copy()
    one = sess.dcrf2d(mine, img[1], shape[1:])
    assert tuple(one.shape) == (1,) + shape[1:] and (mine == 0).sum() == 0 and (mine == np.float32(1e-10)).sum() == 5
    np.testing.assert_array_equal(one.cpu().numpy()[0], _device(sess, shape, 5)[1][1])
    with pytest.raises(KeyError):
        sess.dcrf2d(mine, img[1], shape[1:], params=dict(sigma=3.))


PSHAPE = (5, 5, 3)
RADS = (2, 2, 1)
SLICES = [1, 4, 5]
WEIGHT_SEED = 96      # of seeds 90 .. 99 the one whose posteriors give mixed labels with no marginal within 4e-3 of a tie (CPU oracle + dcrf.py)


@pytest.fixture(scope='module')
def net(sess):
    from nnal_amd import NN
    ld = netspec.net_a()
    in_shape = (5, 5, 6)
    m = NN.CNN(in_shape, ld, 'dcrf', None, None, sess=sess, max_batch=128)
    m.set_weights(netspec.he_init(ld, in_shape, seed=WEIGHT_SEED, bias_std=0.2))
    yield m
    m.close()


def _subject():
    """A (16, 14, 6) subject of two modalities: an elliptic cylinder m, 2 m + 0.7 noise and pure noise; the mask is m."""
    shp = (16, 14, 6)
    r = np.random.RandomState(2207)
    x, y, _ = np.meshgrid(np.arange(shp[0]), np.arange(shp[1]), np.arange(shp[2]), indexing='ij')
    m = ((x - 7.) / 5.) ** 2 + ((y - 7.5) / 4.5) ** 2 < 1
    a = 2. * m + 0.7 * r.randn(*shp)
    b = r.randn(*shp)
    mods = [np.pad(v, [(q, q) for q in RADS], 'constant') for v in (a, b)]
    return mods, a, m.astype(np.float64)


def test_full_model_pred_dcrf(sess, net, tmp_path):
    from nnal_amd import PW_analyze_results as R, dcrf, nrrd_io
    mods, img, mask = _subject()
    expr = Expr({'patch_shape': PSHAPE, 'ntb': 64, 'stats': [[0., 1.], [0., 1.]]}, None)
    save_dir = str(tmp_path / 'dcrf')
    got, F1 = R.full_model_pred_DCRF(expr, net, sess, mods, mask, SLICES, save_dir=save_dir)
    assert got.dtype == np.float64 and got.shape == mask.shape
    others = [z for z in range(mask.shape[2]) if z not in SLICES]
    assert not got[:, :, others].any()
    posts = R.full_slice_eval(net, sess, mods, SLICES, PSHAPE, 64, expr.pars['stats'], 'posteriors')
    left_out = total = 0
    for ind in SLICES:
        p = posts[:, :, ind]
        q64 = dcrf.meanfield_host(p.copy(), img[:, :, ind])[5][1].reshape(p.shape)
        q32 = dcrf.meanfield_host(p.copy(), img[:, :, ind], dtype=np.float32)[5][1].reshape(p.shape)
        tol = 4. * float(np.abs(q32.astype(np.float64) - q64).max()) + 1e-6
        np.testing.assert_array_equal(dcrf.map_host(p.copy(), img[:, :, ind]), q64 > 0.5)
        decided = np.abs(q64 - 0.5) > tol
        left_out += int((~decided).sum())
        total += decided.size
        np.testing.assert_array_equal(got[:, :, ind][decided], (q64 > 0.5)[decided].astype(np.float64), err_msg='slice %d' % ind)
        print('slice %d: posteriors in [%.3f, %.3f], %.3f labelled 1 (raw %.3f), tol %.2e, min |q - .5| %.2e'
              % (ind, p.min(), p.max(), (q64 > 0.5).mean(), (p > 0.5).mean(), tol, np.abs(q64 - 0.5).min()))
    assert left_out <= 0.005 * total
    assert 0 < got[:, :, SLICES].mean() < 1                        # both labels occur: the comparison above is not vacuous
    assert F1 == R.F1_scores(got[:, :, SLICES], mask[:, :, SLICES]) and 0 < F1 < 1
    assert sorted(os.listdir(save_dir)) == ['F1_score_dcrf.txt', 'dcrf_segs.nrrd']
    segs = nrrd_io.read(os.path.join(save_dir, 'dcrf_segs.nrrd'))[0]
    assert segs.dtype == np.uint8
    np.testing.assert_array_equal(segs, got)
    assert float(np.loadtxt(os.path.join(save_dir, 'F1_score_dcrf.txt'))) == F1
    again, F1_again = R.full_model_pred_DCRF(expr, net, sess, mods, mask, SLICES)
    np.testing.assert_array_equal(again, got)
    assert F1_again == F1
