"""alq_model_engine_info by name and by number, and when each half of its answer is reset (GPU box).

NET-C at 32^3 with 4 patches: the smallest geometry at which the plane-sweep and row-sweep engines (c3d, d3d, f3d, e3d, t3d) all
apply - a 32^3 first layer and an 8^3 bottleneck.  The forward indices speak of the last forward pass, the backward indices of
the last backward pass of whatever kind: a general sweep (alq_param_grads) runs none of the Fisher pass's fused backward
launches, and a forward-only pass leaves the backward half alone."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import _netc32_models  # noqa: E402

N = 4
# the numbers of the C ABI as callers have used them so far (include/alq.h; bench.py and the other tests pass them bare)
LEGACY = {'SUBNORMALS_OK': 0, 'C3D_FWD': 1, 'C3D_BWD': 2, 'C3D_ONE_ACC': 3, 'FLIP_OVERFLOW': 5, 'F16_DERIVED': 6, 'T3D_FWD': 7, 'T3D_BWD': 8,
          'E3D_BWD': 9, 'D3D_FWD': 10, 'D3D_BWD': 11, 'F3D_FWD': 12, 'C3D_BWD_FORM': 13, 'HOST_PACK_ELEMS': 14, 'LSUM': 15, 'DCP_FORM': 16,
          'E3D_BWD_FORM': 17}
FISHER_BACKWARD = ('C3D_BWD', 'T3D_BWD', 'E3D_BWD', 'D3D_BWD', 'C3D_BWD_FORM', 'E3D_BWD_FORM')      # 2, 8, 9, 11, 13, 17


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _info(sess, m):
    """{name: value}, after checking that the name and its legacy number give the same answer."""
    from nnal_amd._lib import EngineInfo
    assert sorted(e.name for e in EngineInfo) == sorted(LEGACY)
    out = {}
    for name, number in LEGACY.items():
        by_name = sess.lib.alq_model_engine_info(m._m, EngineInfo[name])
        by_number = sess.lib.alq_model_engine_info(m._m, number)
        assert by_name == by_number and by_name >= 0, (name, by_name, by_number)
        out[name] = by_name
    return out


def test_names_numbers_and_resets(sess):
    from nnal_amd._lib import ALQ_EINVAL, EngineInfo, check
    assert {e.name: int(e) for e in EngineInfo} == LEGACY
    assert [LEGACY[n] for n in FISHER_BACKWARD] == [2, 8, 9, 11, 13, 17]
    ld, sk, in_shape, pars, (m,) = _netc32_models(sess, [{}], max_batch=N, bias_std=0.05)
    x = sess.empty((N, 32 ** 3), sess.torch.float32)
    check(sess.lib.alq_synth_patches(sess.ctx, 1004, 0, N, 32 ** 3, C.c_void_p(x.data_ptr())))
    try:
        m.fisher_device(x, N, None, 1e-3, want=('p1',))
        fisher = _info(sess, m)
        # every sweep engine ran, forward and backward
        assert fisher['C3D_FWD'] == 1 and fisher['D3D_FWD'] == 1 and fisher['F3D_FWD'] == 1 and fisher['T3D_FWD'] >= 1 and fisher['DCP_FORM'] > 0
        assert fisher['C3D_BWD'] == 1 and fisher['D3D_BWD'] == 1 and fisher['E3D_BWD'] == 1 and fisher['T3D_BWD'] >= 1
        assert fisher['C3D_BWD_FORM'] == 7 and fisher['E3D_BWD_FORM'] == 2
        for bad in (4, 18):
            assert sess.lib.alq_model_engine_info(m._m, bad) == ALQ_EINVAL

        # a forward-only pass: the backward half still holds the Fisher pass's values, the forward half is this pass's
        m.forward_device(x, N)
        fwd_only = _info(sess, m)
        for k in FISHER_BACKWARD + ('LSUM',):
            assert fwd_only[k] == fisher[k], k
        assert fwd_only['C3D_FWD'] == 1 and fwd_only['D3D_FWD'] == 1 and fwd_only['F3D_FWD'] == 1 and fwd_only['DCP_FORM'] > 0
        assert fwd_only['T3D_FWD'] == fisher['T3D_FWD']      # a count (+= per launch): a forward half that was not reset would double it

        # a general backward sweep on the same model: 2, 8, 9, 11, 13 and 17 are 0, whatever the Fisher pass before it ran
        m.param_grads_device(x, N, 0, cls=1)
        grads = _info(sess, m)
        for k in FISHER_BACKWARD:
            assert grads[k] == 0, (k, grads[k])
        assert grads['LSUM'] == 0
        # (that pass keeps every activation: no fused head, none of the forward sweep engines that skip a tensor)
        assert grads['C3D_FWD'] == 0
        # ... and a forward-only pass after it: the forward half is this pass's again, the backward half still the general sweep's
        m.forward_device(x, N)
        again = _info(sess, m)
        assert again['C3D_FWD'] == 1 and again['D3D_FWD'] == 1 and again['F3D_FWD'] == 1 and again['T3D_FWD'] == fisher['T3D_FWD']
        for k in FISHER_BACKWARD + ('LSUM',):
            assert again[k] == grads[k], k
        for k in ('SUBNORMALS_OK', 'C3D_ONE_ACC', 'FLIP_OVERFLOW', 'HOST_PACK_ELEMS'):      # not per pass
            assert grads[k] == fisher[k] == fwd_only[k] == again[k], k
    finally:
        m.close()
