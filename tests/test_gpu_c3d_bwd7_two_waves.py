"""The 7-k-step backward kernel of the head conv (csrc/c3d.hip) on two waves per SIMD against its one-wave form (GPU box).

The default form is one 512-thread workgroup per patch, four output rows per wave; ALQ_C3D_BWD_WAVES=1 at model creation keeps the
256-thread kernel with eight rows per wave.  Both stage the same LDS image into the same ring of four planes and give every
output voxel the same MFMAs in the same order and the same epilogue arithmetic, so nothing may differ by a bit: up2's cotangent
(the stored half), the channel-sum fields the launch writes (enc1's, up2's) and every output of the Fisher pass are compared byte
for byte between a default model and a one-wave model.  The kernel takes NET-C at 32^3 only, so the net is fixed and the patch
count is what stays small.  `alq_debug_set(10, g)` caps the launch's grid at g workgroups, so that five patches give streams of
three and two patches that cross patch boundaries through the light steps with the ring carried over.

alq_model_engine_info(m, 19) reports the waves per SIMD of that launch (18 stays refused: tests/test_gpu_engine_info_names.py),
index 20 its workgroups: the capped cases assert that the grid really shrank."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import _netc32_models  # noqa: E402

KEYS = ('p1', 'H', 'g0', 'g1', 'A', 'trace', 'Asum')
NMAX = 8
INFO_WAVES = 19
INFO_GRID = 20        # workgroups of the launch


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


@pytest.fixture(scope='module')
def forms(sess):
    """(two-wave model, one-wave model) with the same weights, and NMAX patches: patch 1 scaled by 2^20, patch 2 all zero."""
    from nnal_amd._lib import check
    ld, sk, in_shape, pars, (m2, m1) = _netc32_models(sess, [{}, {'ALQ_C3D_BWD_WAVES': '1'}], max_batch=NMAX, bias_std=0.05)
    x = sess.empty((NMAX, 32 ** 3), sess.torch.float32)
    check(sess.lib.alq_synth_patches(sess.ctx, 1004, 0, NMAX, 32 ** 3, C.c_void_p(x.data_ptr())))
    x[1] *= 2.0 ** 20
    x[2].zero_()
    yield m2, m1, x
    m2.close()
    m1.close()


def _pass(m, x, n):
    r = m.fisher_device(x[:n].contiguous(), n, None, 1e-3, want=KEYS)
    d = {k: r[k].cpu().numpy().copy() for k in KEYS}
    d['up2_dout'] = m.debug_tensor(7, 1, n).copy()
    d['up2_dsum'] = m.debug_tensor(7, 3, n).copy()
    d['enc1_dsum'] = m.debug_tensor(0, 3, n).copy()
    return d


def _same_bytes(a, b, tag):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (tag, k)
        assert a[k].tobytes() == b[k].tobytes(), '%s: %s differs (%d elements)' % (tag, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize('n,cap,start', [(1, 0, 2), (1, 0, 1), (3, 0, 0), (5, 0, 0), (5, 2, 0)])
def test_two_waves_and_one_wave_give_the_same_bits(sess, forms, n, cap, start):
    """1, 3 and 5 patches on the default grid (a workgroup has one patch or none), and 5 patches on two workgroups (streams of three
    and two patches across patch boundaries).  Every batch holds the all-zero patch; a batch of one IS that patch, so a second
    batch of one holds the scaled patch instead."""
    from nnal_amd._lib import check
    m2, m1, x = forms
    info = sess.lib.alq_model_engine_info
    xb = x[start:start + n]
    assert (float(xb.abs().amax(dim=1).min()) == 0.0) == (start != 1)
    check(sess.lib.alq_debug_set(10, cap))
    try:
        grid = min(n, cap) if cap else n
        a = _pass(m2, xb, n)
        assert (info(m2._m, 2), info(m2._m, 13), info(m2._m, INFO_WAVES), info(m2._m, INFO_GRID)) == (1, 7, 2, grid)
        b = _pass(m1, xb, n)
        assert (info(m1._m, 2), info(m1._m, 13), info(m1._m, INFO_WAVES), info(m1._m, INFO_GRID)) == (1, 7, 1, grid)
    finally:
        check(sess.lib.alq_debug_set(10, 0))
    for k in ('up2_dout', 'up2_dsum', 'enc1_dsum'):
        assert np.isfinite(a[k]).all(), k
    if start != 2:
        assert np.abs(a['up2_dout']).max() > 0 and np.abs(a['up2_dsum']).max() > 0 and np.abs(a['enc1_dsum']).max() > 0
    _same_bytes(a, b, 'n = %d, grid cap %d' % (n, cap))


def test_grid_cap_does_not_change_the_bits(sess, forms):
    """The same five patches on five workgroups and on two: a patch's bits do not depend on what its workgroup swept before it."""
    from nnal_amd._lib import check
    m2, m1, x = forms
    free = _pass(m2, x, 5)
    assert sess.lib.alq_model_engine_info(m2._m, INFO_GRID) == 5
    check(sess.lib.alq_debug_set(10, 2))
    try:
        capped = _pass(m2, x, 5)
        assert sess.lib.alq_model_engine_info(m2._m, INFO_GRID) == 2
    finally:
        check(sess.lib.alq_debug_set(10, 0))
    _same_bytes(free, capped, 'grid cap 2 against the default grid')


def test_engine_report_names_the_waves(sess, forms):
    """alq_model_engine_info(m, 19): 2 by default, 1 under ALQ_C3D_BWD_WAVES=1, 0 after a general backward sweep - like the other
    backward indices - and 13 is 7 for both forms."""
    m2, m1, x = forms
    info = sess.lib.alq_model_engine_info
    for m in (m2, m1):
        m.fisher_device(x[:2].contiguous(), 2, None, 1e-3, want=('p1',))
    assert (info(m2._m, 13), info(m2._m, INFO_WAVES)) == (7, 2)
    assert (info(m1._m, 13), info(m1._m, INFO_WAVES)) == (7, 1)
    for m in (m2, m1):
        m.param_grads_device(x[:2].contiguous(), 2, 0, cls=1)
        assert (info(m._m, 2), info(m._m, 13), info(m._m, INFO_WAVES), info(m._m, INFO_GRID)) == (0, 0, 0, 0)


def test_two_pipelines_equal_one_pipeline(sess):
    """8 patches in two passes of 4: on two scoring pipelines (the passes share the compute units), run twice, and on one pipeline.
    A pass's bits must not depend on what runs beside it."""
    from nnal_amd._lib import check
    ld, sk, in_shape, pars, (m,) = _netc32_models(sess, [{}], max_batch=4, bias_std=0.05)
    n = 8
    x = sess.empty((n, 32 ** 3), sess.torch.float32)
    check(sess.lib.alq_synth_patches(sess.ctx, 1004, 0, n, 32 ** 3, C.c_void_p(x.data_ptr())))
    x[6].zero_()

    def run():
        r = m.fisher_device(x, n, None, 1e-3, want=KEYS)
        return {k: r[k].cpu().numpy().copy() for k in KEYS}
    try:
        m.lanes = 1
        one = run()
        assert sess.lib.alq_model_engine_info(m._m, INFO_WAVES) == 2
        m.lanes = 2
        for it in range(2):
            _same_bytes(one, run(), 'two pipelines, call %d' % it)
    finally:
        m.close()
