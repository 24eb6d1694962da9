"""Re-setting weights on a live model (GPU box): model A takes set_weights(P1), runs a pass, then takes set_weights(P2); model
B, fresh, takes set_weights(P2) only.  Every packed form, scale exponent and host bound of A must then be P2's: posteriors,
every fisher_device output, param_grads_device (mode 0) and grad_sqnorms_device equal B's bit for bit.  P2 is P1 from another
seed with one conv layer scaled by 37 and one by 2^-9 (every scale exponent moves) and one layer's bias all zero (out_bmax
moves; the other biases stay non-zero)."""
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from tests.test_gpu_weights_device import WIDE, _same  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _second_set(ld, in_shape, sk, seed, up, down, zero_bias):
    p2 = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    out = OrderedDict((n, [np.array(W, dtype=np.float32), np.array(b, dtype=np.float32)]) for n, (W, b) in p2.items())
    out[up][0] *= np.float32(37.0)
    out[down][0] *= np.float32(2.0 ** -9)
    assert np.abs(out[zero_bias][1]).max() > 0
    out[zero_bias][1][...] = 0.0
    assert all(np.abs(b).max() > 0 for n, (_, b) in out.items() if n != zero_bias)
    return out


def _outputs(sess, m, x, info=None):
    torch = sess.torch
    n = int(x.shape[0])
    t = sess.to_device(x.reshape(n, -1), torch.float32)
    out = OrderedDict()
    out['post'] = m.forward_device(t, n)[0]
    r = m.fisher_device(t, n, None, 1e-3)
    for k in ('p1', 'g0', 'g1', 'A', 'trace', 'Asum'):
        out['fisher_' + k] = r[k]
    if info is not None:      # what the Fisher pass ran (a later backward sweep resets the backward half)
        from nnal_amd._lib import EngineInfo
        info.update({e.name: sess.lib.alq_model_engine_info(m._m, int(e)) for e in EngineInfo})
    out['pg0'] = m.param_grads_device(t, n, 0, cls=1)[0]
    out['sqn'] = m.grad_sqnorms_device(t, n)
    torch.cuda.synchronize()
    return out


def _cases():
    ld_c, sk_c = netspec.net_c()
    netb = netspec.net_b_small(width=WIDE)
    # (name, layers, input shape, skips, patches, max_batch, layer scaled by 37, layer scaled by 2^-9, layer with zero bias, debug knob)
    return [('netc32', ld_c, (32, 32, 32, 1), sk_c, 3, 4, 'dec2', 'enc2', 'up2', 0),      # c3d, d3d, f3d, e3d, t3d
            ('netc8', ld_c, (8, 8, 8, 1), sk_c, 5, 8, 'bott', 'dec1', 'enc1', 0),         # the two-slot engine, t3d8b
            ('netb32', netb, (32, 32, 32), (), 4, 4, 'conv4', 'conv2', 'fc1', 0),         # streaming GEMM, igemm3, output-channel slices
            ('netb32_knob4', netb, (32, 32, 32), (), 4, 4, 'conv4', 'conv2', 'fc1', 4),   # ... and the fallback forms behind it
            ('netb32_knob5', netb, (32, 32, 32), (), 4, 4, 'conv4', 'conv2', 'fc1', 5)]


@pytest.mark.parametrize('case', _cases(), ids=lambda c: c[0])
def test_second_set_equals_a_fresh_model(sess, case):
    name, ld, in_shape, sk, n, max_batch, up, down, zero_bias, knob = case
    from nnal_amd import device
    from nnal_amd._lib import check
    p1 = netspec.he_init(ld, in_shape, seed=81, skips=sk, bias_std=0.05)
    p2 = _second_set(ld, in_shape, sk, 82, up, down, zero_bias)
    x = np.random.RandomState(83).randn(n, *in_shape).astype(np.float32)
    A = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
    B = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
    if knob:
        check(sess.lib.alq_debug_set(knob, 1))
    try:
        A.set_weights(p1)
        first = _outputs(sess, A, x)          # A is live: under a knob this packs the fallback forms from P1
        A.set_weights(p2)
        B.set_weights(p2)
        info = {}
        oa, ob = _outputs(sess, A, x, info), _outputs(sess, B, x)
        if name == 'netc32':      # the geometry that reaches every sweep engine did
            assert info['C3D_FWD'] == 1 and info['D3D_FWD'] == 1 and info['F3D_FWD'] == 1 and info['T3D_FWD'] >= 1, info
            assert info['C3D_BWD'] == 1 and info['D3D_BWD'] == 1 and info['E3D_BWD'] == 1 and info['T3D_BWD'] >= 1, info
    finally:
        if knob:
            check(sess.lib.alq_debug_set(knob, 0))
    _same(oa, ob, name)
    assert not sess.torch.equal(first['post'], oa['post'])          # the second set did change the model
    A.close()
    B.close()
