"""The first conv + pool kernel on whole-row tiles (csrc/direct.hip) and up2's backward with paired sum stores
(csrc/t3d.hip): a change of the store layout must not change a bit (GPU box).

What the fused kernel writes - enc1's activation, channel sums and sign bytes, pool1's output, channel sums, sign bytes and
arg-max - is compared bit for bit with references that share none of the changed code:
  * the voxel-per-thread `direct_conv_kernel` + the pool launch (alq_debug_set(7, 1)), whose accumulation order the fused
    kernel promises (bias, then taps z, y, x ascending, one fma each): activations, pooled values, both sum fields, arg-max;
  * the host, from the activation that was just compared: the sums in the association the kernels use, the sign bytes
    (bit k of byte b = channel 4 b + k > 0) and the first maximum of every window - that route writes no sign field.
The Fisher outputs of a pass cannot be compared bitwise with that route: without the fused kernel nothing measures enc1's
per-patch maximum, and the layers behind it contract on other engines (bf16 triples instead of fp16 pairs).  They are
compared bitwise with the kernel's narrow form (alq_debug_set(8, 1): 8 x 16 x 16 tile, one 4-byte sum store and one 2-byte
sign store per voxel everywhere - the form every volume ran before the wide tile), under which every later launch is the
same; `alq_model_engine_info(m, 16)` says which instantiation a pass ran, and the test checks it is the intended one."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _model(sess, ld, in_shape, sk, pars, max_batch):
    from nnal_amd import device
    m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
    m.set_weights(pars)
    return m


def _copy(sess, m, layer, what, n):
    """alq_model_debug_copy of the last pass: what = 0 activation of `layer`, 11 = channel sums of its output, 12 = sign
    field of the rows its output lies in, 13 = arg-max bytes of a pool layer (12, 13: view the result as bytes)."""
    from nnal_amd._lib import check
    torch = sess.torch
    e = C.c_int64()
    cap = n * int(np.prod(m.in_shape)) * 16
    buf = torch.zeros((cap,), dtype=torch.float32, device=sess.device)
    check(m.lib.alq_model_debug_copy(m._m, int(layer), int(what), int(n), C.c_void_p(buf.data_ptr()), C.byref(e)))
    torch.cuda.synchronize()
    assert 0 < e.value <= cap
    return buf[:e.value].cpu().numpy()


def _synth(sess, n, elems, seed=1004):
    from nnal_amd._lib import check
    x = sess.empty((n, elems), sess.torch.float32)
    check(sess.lib.alq_synth_patches(sess.ctx, seed, 0, n, elems, C.c_void_p(x.data_ptr())))
    return x


class _knob(object):
    """alq_debug_set(key, 1) for the block."""

    def __init__(self, sess, key):
        self.sess, self.key = sess, key

    def __enter__(self):
        from nnal_amd._lib import check
        check(self.sess.lib.alq_debug_set(self.key, 1))

    def __exit__(self, *exc):
        from nnal_amd._lib import check
        check(self.sess.lib.alq_debug_set(self.key, 0))


def _form(m):
    """Instantiation of the first conv + pool kernel in the last forward pass: 0 = it did not run, 1 / 2 = narrow tile with scalar /
    16-byte row loads, 4 / 5 = wide tile, 6 = wide tile on whole-tile volumes (16-byte sum and sign stores)."""
    return int(m.lib.alq_model_engine_info(m._m, 16))


def _want_form(dhw, cs):
    D, H, W = dhw
    wide = -(-W // 32) * 32 <= -(-W // 16) * 16
    aligned = W % 4 == 0
    full = wide and aligned and D % 8 == 0 and H % 16 == 0 and W % 32 == 0 and cs == 8
    return 1 + (3 if wide else 0) + (2 if full else 1 if aligned else 0)


def _sign_bytes(act):
    """[..., 8] activation -> [..., 2] sign bytes."""
    b = (act > 0).astype(np.uint8)
    w = np.array([1, 2, 4, 8], np.uint8)
    return np.stack([(b[..., :4] * w).sum(-1), (b[..., 4:] * w).sum(-1)], -1).astype(np.uint8)


def _chan_sums(act):
    o = [act[..., c] for c in range(8)]      # float32 adds, the kernels' association
    return ((o[0] + o[1]) + (o[2] + o[3])) + ((o[4] + o[5]) + (o[6] + o[7]))


def _first_conv_fields(sess, m, n, dhw, signs):
    """Everything the first conv + pool launch(es) of the last pass wrote for the first n patches."""
    D, H, W = dhw
    vox = D * H * W
    f = {'enc1': _copy(sess, m, 0, 0, n).reshape(n, D, H, W, 8), 'pool1': _copy(sess, m, 1, 0, n).reshape(n, D // 2, H // 2, W // 2, 8),
         'enc1_sums': _copy(sess, m, 0, 11, n).reshape(n, D, H, W), 'pool1_sums': _copy(sess, m, 1, 11, n).reshape(n, D // 2, H // 2, W // 2),
         'argmax': _copy(sess, m, 1, 13, n).view(np.uint8).reshape(n, D // 2, H // 2, W // 2, 8)}
    if signs:
        s0 = _copy(sess, m, 0, 12, n).view(np.uint8)
        assert s0.size % (n * vox) == 0
        f['cs'] = 4 * s0.size // (n * vox)      # channels of the allocation enc1 lies in (8, or 16 next to up1's output)
        f['enc1_signs'] = s0.reshape(n, D, H, W, f['cs'] // 4)[..., :2]
        s1 = _copy(sess, m, 1, 12, n).view(np.uint8)
        assert s1.size == n * vox // 8 * 2
        f['pool1_signs'] = s1.reshape(n, D // 2, H // 2, W // 2, 2)
    return f


def _check_fields_against_host(f, n, dhw):
    D, H, W = dhw
    enc1, pool1 = f['enc1'], f['pool1']
    assert (enc1 > 0).mean() > 0.2 and (enc1 == 0).mean() > 0.2
    np.testing.assert_array_equal(f['enc1_sums'].view(np.uint32), _chan_sums(enc1).view(np.uint32), err_msg='enc1 sums')
    np.testing.assert_array_equal(f['pool1_sums'].view(np.uint32), _chan_sums(pool1).view(np.uint32), err_msg='pool1 sums')
    np.testing.assert_array_equal(f['enc1_signs'], _sign_bytes(enc1), err_msg='enc1 sign bytes')
    np.testing.assert_array_equal(f['pool1_signs'], _sign_bytes(pool1), err_msg='pool1 sign bytes')
    # windows in (dz, dy, dx) order; np.argmax returns the first maximum, as the kernels keep it
    win = enc1.reshape(n, D // 2, 2, H // 2, 2, W // 2, 2, 8).transpose(0, 1, 3, 5, 2, 4, 6, 7).reshape(n, D // 2, H // 2, W // 2, 8, 8)
    np.testing.assert_array_equal(pool1.view(np.uint32), win.max(axis=4).view(np.uint32), err_msg='pool1')
    np.testing.assert_array_equal(f['argmax'], win.argmax(axis=4).astype(np.uint8), err_msg='arg-max')


KEYS = ('p1', 'H', 'g0', 'g1', 'A', 'trace', 'Asum')


def test_netc32_same_bits_across_pass_cuts_pipelines_and_kernel_forms(sess):
    """NET-C at 32^3 (the bench path: whole-row tiles, 16-byte sum / sign stores, paired sum stores in up2's backward): 75
    patches in one pass, in passes of 19 and of 8 (ragged last pass, ragged last workgroups of the row-sweep kernels), on one
    and on two pipelines, with the first conv on the whole-tile wide form (engine info 16 = 6) and on the narrow per-voxel
    form (2): every Fisher output is the same bits.  Asum is a pass-ordered fp64 sum: exact for one cut whatever the
    pipelines and the form, and equal to rounding (1e-12) between cuts, whose order of summation differs.  Then the fields
    the first conv wrote in a single pass of 5, both forms, against the host."""
    ld, sk = netspec.net_c()
    in_shape = (32, 32, 32, 1)
    pars = netspec.he_init(ld, in_shape, seed=14, skips=sk, bias_std=0.05)
    n = 75
    x = _synth(sess, n, 32 ** 3)
    ref = None
    for max_batch in (75, 19, 8):
        m = _model(sess, ld, in_shape, sk, pars, max_batch)
        cut_asum = None
        for lanes in (1, 2):
            for narrow in (False, True):
                m.lanes = lanes
                tag = 'max_batch %d, %d pipelines, %s form' % (max_batch, lanes, 'narrow' if narrow else 'wide')
                if narrow:
                    with _knob(sess, 8):
                        r = m.fisher_device(x, n, None, 1e-3, want=KEYS)
                else:
                    r = m.fisher_device(x, n, None, 1e-3, want=KEYS)
                assert _form(m) == (2 if narrow else 6), tag
                cur = {k: r[k].cpu().numpy() for k in KEYS}
                if ref is None:
                    ref = cur
                    assert np.isfinite(ref['A']).all() and np.abs(ref['g0']).max() > 0
                if cut_asum is None:
                    cut_asum = cur['Asum']
                for k in KEYS:
                    if k == 'Asum':
                        np.testing.assert_array_equal(cur[k], cut_asum, err_msg=tag)
                        np.testing.assert_allclose(cur[k], ref[k], rtol=1e-12, err_msg=tag)
                    else:
                        np.testing.assert_array_equal(cur[k], ref[k], err_msg=tag + ': ' + k)
        m.close()
    m = _model(sess, ld, in_shape, sk, pars, 8)
    nf = 5
    fields = {}
    for narrow in (False, True):
        if narrow:
            with _knob(sess, 8):
                m.fisher_device(x, nf, None, 1e-3, want=('p1',))
        else:
            m.fisher_device(x, nf, None, 1e-3, want=('p1',))
        assert _form(m) == (2 if narrow else 6)
        f = fields[narrow] = _first_conv_fields(sess, m, nf, (32, 32, 32), signs=True)
        assert f['cs'] == 8      # (split concat: what the whole-tile form needs)
        _check_fields_against_host(f, nf, (32, 32, 32))
    for k in fields[False]:
        np.testing.assert_array_equal(fields[False][k], fields[True][k], err_msg=k)
    m.close()


# (D, H, W): W = 30, 18: rows that are no multiple of 4 voxels (scalar block loads) on the 32-voxel tile with half-empty
# lanes; 24: float4 loads, partial tile in x; 34, 40: the 16-voxel tile (three of them); 32 and 16 wide with partial tiles
# in y and z; (8, 16, 32), (16, 32, 64): whole wide tiles only (16-byte sum / sign stores where enc1 has its rows to itself);
# (8, 16, 16): whole narrow tiles
SHAPES = [(10, 12, 30), (6, 20, 18), (12, 10, 24), (4, 6, 34), (6, 4, 40), (10, 12, 32), (6, 20, 16), (8, 16, 32), (8, 16, 16),
          (16, 32, 64)]
FKEYS = ('p1', 'H', 'g0', 'g1', 'A', 'trace')


@pytest.mark.parametrize('skip', [True, False], ids=['skip', 'noskip'])
@pytest.mark.parametrize('dhw', SHAPES)
def test_first_conv_pool_tiles_against_the_voxel_per_thread_kernel(sess, dhw, skip):
    """A small U-net on volumes that leave partial tiles of either width and on whole-tile volumes, with enc1's output as the
    skip source of dec1 (its rows shared with up1's output unless the layout is split) and without (rows of 8 channels:
    whole-tile volumes must then take the 16-byte sum / sign stores, engine info 16 = 6).  Three routes: the fused kernel as
    launched by default, its narrow per-voxel form, and `direct_conv_kernel` + the pool launch.  Everything the first conv
    writes is the same bits on all three and equals what the host derives from the activation; every Fisher output is the same
    bits on the two forms of the fused kernel, and on a second run."""
    in_shape = tuple(dhw) + (1,)
    k3, s2 = [3, 3, 3], [2, 2, 2]
    ld = OrderedDict([('enc1', ['conv', [8, k3], 'MA']), ('pool1', ['pool', s2]), ('enc2', ['conv', [16, k3], 'MA']),
                      ('up1', ['conv_transpose', [8, k3, s2], 'M']), ('dec1', ['conv', [8, k3], 'MA']), ('fc', ['fc', [2]])])
    sk = [[0, [4], 'con']] if skip else []
    pars = netspec.he_init(ld, in_shape, seed=23, skips=sk, bias_std=0.05)
    n = 5
    m = _model(sess, ld, in_shape, sk, pars, max_batch=8)
    x = _synth(sess, n, int(np.prod(in_shape)), seed=78)

    def run(signs=True):
        r = m.fisher_device(x, n, None, 1e-3, want=FKEYS)
        out = {k: r[k].cpu().numpy() for k in FKEYS}
        return out, _first_conv_fields(sess, m, n, dhw, signs), _form(m)
    wide, wide_f, wide_form = run()
    with _knob(sess, 8):
        narrow, narrow_f, narrow_form = run()
    with _knob(sess, 7):
        plain, plain_f, plain_form = run(signs=False)
    again, again_f, again_form = run()
    cs = wide_f['cs']
    print(dhw, 'skip' if skip else 'no skip', 'channels per row of enc1:', cs, 'forms:', wide_form, narrow_form, plain_form)
    assert cs == 8 or (skip and cs == 16)
    assert wide_form == again_form == _want_form(dhw, cs)
    if not skip and dhw in ((8, 16, 32), (16, 32, 64)):
        assert wide_form == 6
    assert narrow_form == (2 if dhw[2] % 4 == 0 else 1) and plain_form == 0
    _check_fields_against_host(wide_f, n, dhw)
    for k in ('enc1', 'pool1', 'enc1_sums', 'pool1_sums', 'argmax'):
        np.testing.assert_array_equal(wide_f[k].view(np.uint8), plain_f[k].view(np.uint8), err_msg='against direct_conv_kernel: ' + k)
    for k in wide_f:
        np.testing.assert_array_equal(wide_f[k], narrow_f[k], err_msg='narrow form: ' + k)
        np.testing.assert_array_equal(wide_f[k], again_f[k], err_msg='second run: ' + k)
    for k in FKEYS:
        np.testing.assert_array_equal(wide[k], narrow[k], err_msg='narrow form: ' + k)
        np.testing.assert_array_equal(wide[k], again[k], err_msg='second run: ' + k)
    # the other engines behind `direct_conv_kernel` (see the module's docstring) keep the scores within the 5e-4 of a layer's
    # scale that the engines' own tests allow each other; a wrong sign byte or sum would move them by far more
    for k in ('g0', 'g1'):
        scale = np.abs(plain[k]).max(axis=0, keepdims=True)
        err = np.abs(wide[k] - plain[k])
        print(dhw, k, 'max err / scale per layer:', (err / np.maximum(scale, 1e-30)).max(axis=0))
        assert (err <= 5e-4 * scale + 1e-9).all(), err.max()
    assert np.abs(wide['p1'] - plain['p1']).max() <= 5e-6
    m.close()
