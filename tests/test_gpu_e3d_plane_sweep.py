"""The fused enc2 backward launch (csrc/e3d.hip) as a z plane sweep against its row-sweep form (GPU box).

Both kernels stage the same rows with the same arithmetic and contract every output tile with the same MFMA sequence into the
same accumulators; the plane sweep (default) only stages every row once and streams over whole patches.  So nothing may differ
by a bit: the Fisher outputs of a pass and the two channel-sum fields the launch writes (enc2's, enc1's) are compared byte
for byte between a default model and one created under ALQ_E3D_ROWS=1.  `alq_debug_set(9, g)` caps the plane sweep's grid at g
workgroups, so that a handful of patches gives streams that cross patch boundaries."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import _netc32_models  # noqa: E402

KEYS = ('p1', 'H', 'g0', 'g1', 'A', 'trace', 'Asum')
NMAX = 37


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


@pytest.fixture(scope='module')
def forms(sess):
    """(plane-sweep model, row-sweep model) with the same weights, and NMAX patches: patch 1 scaled by 2^20, patch 2 all zero."""
    from nnal_amd._lib import check
    ld, sk, in_shape, pars, (mz, mr) = _netc32_models(sess, [{}, {'ALQ_E3D_ROWS': '1'}], max_batch=NMAX, bias_std=0.05)
    x = sess.empty((NMAX, 32 ** 3), sess.torch.float32)
    check(sess.lib.alq_synth_patches(sess.ctx, 1004, 0, NMAX, 32 ** 3, C.c_void_p(x.data_ptr())))
    x[1] *= 2.0 ** 20
    x[2].zero_()
    yield mz, mr, x
    mz.close()
    mr.close()


def _pass(m, x, n):
    r = m.fisher_device(x[:n].contiguous(), n, None, 1e-3, want=KEYS)
    d = {k: r[k].cpu().numpy().copy() for k in KEYS}
    d['enc2_dsum'] = m.debug_tensor(2, 3, n).copy()
    d['enc1_dsum'] = m.debug_tensor(0, 3, n).copy()
    return d


def _same_bytes(a, b, tag):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (tag, k)
        assert a[k].tobytes() == b[k].tobytes(), '%s: %s differs (%d elements)' % (tag, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize('n,cap', [(1, 2), (2, 2), (5, 2), (NMAX, 0)])
def test_plane_sweep_and_row_sweep_give_the_same_bits(sess, forms, n, cap):
    """Two workgroups over 1, 2 and 5 patches (a single patch and an idle workgroup; one patch each; streams of three and two patches
    that cross patch boundaries), and the product grid over 37 (the last workgroups hold nothing)."""
    from nnal_amd._lib import check
    mz, mr, x = forms
    check(sess.lib.alq_debug_set(9, cap))
    try:
        a = _pass(mz, x, n)
        assert sess.lib.alq_model_engine_info(mz._m, 17) == 2 and sess.lib.alq_model_engine_info(mz._m, 9) == 1
        b = _pass(mr, x, n)
        assert sess.lib.alq_model_engine_info(mr._m, 17) == 1 and sess.lib.alq_model_engine_info(mr._m, 9) == 1
    finally:
        check(sess.lib.alq_debug_set(9, 0))
    assert np.isfinite(a['enc1_dsum']).all() and np.isfinite(a['enc2_dsum']).all()
    assert np.abs(a['enc1_dsum']).max() > 0 and np.abs(a['enc2_dsum']).max() > 0
    _same_bytes(a, b, 'n = %d, grid cap %d' % (n, cap))


def test_engine_report_names_the_form(sess, forms):
    """alq_model_engine_info(m, 17): 2 = plane sweep by default, 1 = row sweep under ALQ_E3D_ROWS=1, 0 with index 9 at 0 under
    ALQ_NO_E3D=1 (the three launches)."""
    mz, mr, x = forms
    info = sess.lib.alq_model_engine_info
    ld, sk, in_shape, pars, (m3,) = _netc32_models(sess, [{'ALQ_NO_E3D': '1'}], max_batch=2, bias_std=0.05)
    for m in (mz, mr, m3):
        m.fisher_device(x[:2].contiguous(), 2, None, 1e-3, want=('p1',))
    assert (info(mz._m, 9), info(mz._m, 17)) == (1, 2)
    assert (info(mr._m, 9), info(mr._m, 17)) == (1, 1)
    assert (info(m3._m, 9), info(m3._m, 17)) == (0, 0)
    m3.close()


def test_repeated_passes_on_two_pipelines_return_the_first_call_s_bits(sess, forms):
    """48 patches in two passes of 24, one on each of two pipelines, 20 calls: a pass's bits must not depend on what shares the
    compute units with it (the ring rule of the kernel: no staging into a slot that a tile of the same step reads)."""
    from nnal_amd._lib import check
    ld, sk, in_shape, pars, (m,) = _netc32_models(sess, [{}], max_batch=24, bias_std=0.05)
    n = 48
    x = sess.empty((n, 32 ** 3), sess.torch.float32)
    check(sess.lib.alq_synth_patches(sess.ctx, 1004, 0, n, 32 ** 3, C.c_void_p(x.data_ptr())))
    m.lanes = 2

    def run():
        r = m.fisher_device(x, n, None, 1e-3, want=KEYS)
        return {k: r[k].cpu().numpy().copy() for k in KEYS}
    first = run()
    assert sess.lib.alq_model_engine_info(m._m, 17) == 2
    for it in range(1, 20):
        _same_bytes(first, run(), 'call %d' % it)
    m.close()
