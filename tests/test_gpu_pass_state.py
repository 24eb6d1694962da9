"""What one pass leaves behind must not reach the next one (GPU box).

The routing state of a forward pass and of the Fisher backward sweep (which launches handed maxima or sign fields to which,
the static cotangent bounds, the head's mask-bit hand-off) belongs to the pass that built it; the model keeps only what
alq_model_engine_info and alq_model_debug_copy report about the LAST pass.  NET-C at 32^3 with 4 patches - the smallest
geometry at which every sweep engine applies (tests/test_gpu_engine_info_names.py):
  (a) the Fisher outputs of a fresh model, byte for byte, after every other kind of pass has run on the same model;
  (b) the sign field of the first conv's output (alq_model_debug_copy, what = 12) is there after a Fisher pass and refused
      after the passes that write none."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_engine_info_names import _info  # noqa: E402
from tests.test_gpu_parity import _netc32_models  # noqa: E402

N = 4
ELEMS = 32 ** 3
EUNSUPPORTED = -4
OUTPUTS = ('p1', 'g0', 'g1', 'A', 'trace')


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _synth(sess, first):
    from nnal_amd._lib import check
    x = sess.empty((N, ELEMS), sess.torch.float32)
    check(sess.lib.alq_synth_patches(sess.ctx, 1004, first, N, ELEMS, C.c_void_p(x.data_ptr())))
    return x


def _fisher(m, x):
    r = m.fisher_device(x, N, None, 1e-3, want=OUTPUTS)
    return {k: r[k].cpu().numpy() for k in OUTPUTS}


def _dropout_grads(m, x):
    m.dropout_layers = [0, 2, 6]      # enc1 (the first conv + pool kernel steps aside), enc2, dec1
    g, _, _ = m.param_grads_device(x, N, 1, labels=np.array([0, 1, 1, 0], np.int32), loss_scale=300., keep_prob=0.5, seed=7,
                                   per_sample=False)
    assert np.isfinite(g.cpu().numpy()).all()


def test_fisher_outputs_do_not_depend_on_earlier_passes(sess):
    torch = sess.torch
    ld, sk, in_shape, pars, (m,) = _netc32_models(sess, [{}], max_batch=N, bias_std=0.05)
    x, other = _synth(sess, 0), _synth(sess, 1000)
    labels = sess.to_device(np.array([1, 0, 0, 1], np.int32), torch.int32)
    v = sess.to_device(np.random.RandomState(3).randn(m.num_params).astype(np.float32), torch.float32)
    try:
        fresh = _fisher(m, x)
        info = _info(sess, m)
        for k in OUTPUTS:
            assert np.isfinite(fresh[k]).all(), k
        between = [('param_grads with dropout', lambda: _dropout_grads(m, x)),
                   ('forward-only', lambda: m.forward_device(x, N)),
                   ('hess_vecp', lambda: m.hess_vecp_device(x, N, labels, v)),
                   ('Fisher pass on other patches', lambda: _fisher(m, other))]
        for name, run in between:
            run()
            again = _fisher(m, x)
            for k in OUTPUTS:
                np.testing.assert_array_equal(again[k], fresh[k], err_msg='%s after %s' % (k, name))
        assert _info(sess, m) == info
    finally:
        m.close()


def test_sign_field_copy_follows_the_last_pass(sess):
    torch = sess.torch
    ld, sk, in_shape, pars, (m,) = _netc32_models(sess, [{}], max_batch=N, bias_std=0.05)
    x = _synth(sess, 0)
    cap = N * ELEMS      # 4-byte words: enc1's rows hold at most 16 channels (its own 8 and the concat's other half), 1 byte per 4
    buf = torch.zeros((cap,), dtype=torch.float32, device=sess.device)

    def copy():
        e = C.c_int64(-1)
        rc = sess.lib.alq_model_debug_copy(m._m, 0, 12, N, C.c_void_p(buf.data_ptr()), C.byref(e))
        torch.cuda.synchronize()
        return rc, e.value

    try:
        m.fisher_device(x, N, None, 1e-3, want=('p1',))
        rc, words = copy()
        assert rc == 0 and N * ELEMS * 8 // 16 <= words <= cap
        assert buf[:words].view(torch.uint8).any().item()      # some unit of enc1 is positive
        m.forward_device(x, N)
        assert copy()[0] == EUNSUPPORTED
        m.fisher_device(x, N, None, 1e-3, want=('p1',))
        assert copy()[0] == 0
        m.param_grads_device(x, N, 0, cls=1)
        assert copy()[0] == EUNSUPPORTED
    finally:
        m.close()
