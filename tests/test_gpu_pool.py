"""The max-pool kernels of csrc/kernels.hip on their own, every launch form, against tests/pool_ref.py (GPU box).

Max pooling selects and moves values, so pooled values, arg-max bytes and routed cotangents are compared on EQUAL BITS;
tolerances appear only on channel sums (what = 3 / 11 of alq_model_debug_copy), where the bound is
(C - 1) 2^-24 sum |terms| per voxel - an fp32 sum of C terms in any order, the kernels use several associations - and in
the accumulate cases, which are held to the fp64 oracle with the bars of tests/test_gpu_grads_fp64.py.

Two model shapes, built through device.DeviceModel and read with alq_model_debug_copy:
  * P-first, pool -> fc(2): the pool reads the caller's x, so the inputs are designed (exact ties, +0 and -0, a patch that is
    negative throughout - its windows next to a padded edge must give the negative maximum, not 0 -, mixed magnitudes);
  * conv-below, conv(C) -> pool -> fc(2) and conv(8) -> conv(C) -> pool -> fc(2): the conv's activation and the pool's own
    cotangent are read from the device and taken as given; the pool's output, its arg-max bytes and the conv's cotangent
    (the routed cotangent, times the ReLU mask where the conv has one) follow from them exactly.
k_pool_fwd / k_pool_bwd / k_pool_bwd_first choose the kernel from the channel count, the alignment, whether the layer below
is the first parameterised layer, whether it has a ReLU and whether it is a skip source; the tables below note the form
each case is meant to reach (there is no engine-info index for these kernels: a kernel trace of this file lists them).

Forms no case can reach: pool_bwd_vox<4> and <8> did not exist behind k_pool_bwd's guard (4 and 8 channels only) and are
no longer instantiated."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import alpath, netspec  # noqa: E402
from tests import pool_ref  # noqa: E402
from tests.pool_ref import GEOMETRIES  # noqa: E402

GRID_CAP_THREADS = 8192 * 256      # grid_for: at most 8192 workgroups of 256 threads; beyond it the kernels stride


def _fwd_form(C_):
    if C_ % 4:
        return 'pool_fwd (scalar)'
    return 'pool_fwd_vox<%d>' % (C_ // 4) if C_ in (4, 8, 16, 32) else 'pool_fwd_vec'


# ---- forward, P-first: every geometry with one channel count of each of the three families: (geometry, C, form)
_SCALAR_C, _VOX_C, _VEC_C = (1, 3, 5, 6), (4, 8, 16, 32), (12, 20, 64)
FWD_CASES = [(g, cs[i % len(cs)], _fwd_form(cs[i % len(cs)]))
             for i, g in enumerate(GEOMETRIES) for cs in (_SCALAR_C, _VOX_C, _VEC_C)]

# ---- backward, conv-below: (geometry, C of the pooled conv, its kernel size, its op order, a conv(8) below it?, path, form).
# `general`: alq_param_grads (every cotangent stored, no mask or sum in the pool launch); `fisher`: model.fisher_device.
BWD_CASES = [
    ('7x5_w2', 6, 3, 'MA', False, 'general', 'pool_bwd (scalar)'),
    ('5x7x3_w222', 6, 1, 'M', True, 'general', 'pool_bwd (scalar)'),
    ('4x4_w3', 8, 3, 'MA', False, 'general', 'pool_bwd_vec<0>'),
    ('5x5_w4', 12, 1, 'M', True, 'general', 'pool_bwd_vec<0>'),
    ('7x7x7_w333', 4, 3, 'MA', False, 'general', 'pool_bwd_vec<0>'),
    ('7x7x7_w666', 16, 1, 'MA', True, 'general', 'pool_bwd_vec<0>'),
    ('7x7x7_w666', 6, 1, 'MA', True, 'general', 'pool_bwd (scalar): bytes above 127'),
    ('7x5_w2', 6, 3, 'MA', False, 'fisher', 'pool_bwd (scalar)'),
    ('5x5_w3', 6, 1, 'M', True, 'fisher', 'pool_bwd (scalar)'),
    ('5x5_w3', 12, 3, 'MA', True, 'fisher', 'pool_bwd_vec<0>, then the mask and sum kernels'),
    ('4x6x6_w122', 12, 3, 'M', False, 'fisher', 'pool_bwd_vec<0>, then the sum kernel'),
    ('8x8_w2', 4, 3, 'MA', True, 'fisher', 'pool_bwd_vec<1>'),
    ('7x5_w2', 8, 1, 'MA', True, 'fisher', 'pool_bwd_vec<2>'),
    ('5x5_w4', 8, 3, 'M', True, 'fisher', 'pool_bwd_vec<2>, no mask'),
    ('4x4_w3', 16, 3, 'MA', True, 'fisher', 'pool_bwd_vec<4>'),
    ('7x7x7_w333', 32, 1, 'MA', True, 'fisher', 'pool_bwd_vec<8>'),
    ('7x7x7_w666', 32, 1, 'M', True, 'fisher', 'pool_bwd_vec<8>, no mask'),
    ('7x5_w2', 4, 3, 'MA', False, 'fisher', 'pool_bwd_vox<1>: first layer, odd sizes'),
    ('4x4_w3', 8, 3, 'MA', False, 'fisher', 'pool_bwd_vox<2>: first layer, window 3'),
    ('8x8_w2', 4, 3, 'M', False, 'fisher', 'pool_bwd_vox<1>: first layer without ReLU, no mask'),
    ('5x7x3_w222', 8, 3, 'MA', False, 'fisher', 'pool_bwd_vox<2>: first layer, odd sizes in 3-D'),
    ('7x7x7_w666', 8, 3, 'MA', False, 'fisher', 'pool_bwd_vox<2>: first layer, bytes above 127'),
]
# ---- pool_bwd_first<C / 4>: first layer with ReLU, even sizes, window 2: (geometry, C); wz = 1 in 2-D, 2 in 3-D
FIRST_CASES = [(g, c) for g in ('8x8_w2', '6x6x6_w222') for c in (4, 8, 16)]

# ---- grid stride: more threads than grid_for's cap, window [1, 1, 2] (extended 2-D schema): (form, input (H, W, C), N)
STRIDE_FWD = [('pool_fwd (scalar)', (64, 64, 3), 350), ('pool_fwd_vec', (64, 64, 12), 350), ('pool_fwd_vox<1>', (64, 64, 4), 1030)]
# the general path reaches the scalar kernel and pool_bwd_vec<0>: (form, C of the 1x1 conv on a 64 x 64 x 1 input, N)
STRIDE_BWD = [('pool_bwd (scalar)', 6, 90), ('pool_bwd_vec<0>', 12, 175)]

# ---- accumulate: enc1's width in netspec.net_c_2d -> the message of the library's refusal (ALQ_EUNSUPPORTED = -4), or None.
# 6 channels next to up1's 8 are a concat slice that starts at float 6: every contraction engine wants 16-byte slices, so
# the scalar kernel's accumulate branch cannot be reached through a model
ACCUMULATE = OrderedDict([(6, 'igemm4: channel slice not 16-byte aligned'), (12, None), (8, None)])


# ------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _model(sess, ld, in_shape, pars, max_batch, sk=()):
    from nnal_amd import device
    m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
    assert m.max_batch == max_batch
    m.set_weights(pars)
    return m


def _copy(sess, m, layer, what, n, expect):
    """alq_model_debug_copy of the last pass; `expect` 4-byte words must come back."""
    from nnal_amd._lib import check
    torch = sess.torch
    e = C.c_int64()
    buf = torch.zeros((int(expect) + 64,), dtype=torch.float32, device=sess.device)
    check(m.lib.alq_model_debug_copy(m._m, int(layer), int(what), int(n), C.c_void_p(buf.data_ptr()), C.byref(e)))
    torch.cuda.synchronize()
    assert e.value == expect, (layer, what, e.value, expect)
    return buf[:e.value].cpu().numpy()


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


def _dev(sess, x):
    return sess.to_device(np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1), sess.torch.float32)


def _pick_n(elems_per_patch, threads_per_patch):
    """A batch of 3 .. 8 patches whose arg-max field is whole 4-byte words (what = 13) and whose launches end in a ragged
    wave (no multiple of 64 threads) where some N allows both."""
    ok = [n for n in (5, 3, 7, 6, 4, 8) if (n * elems_per_patch) % 4 == 0]
    assert ok, elems_per_patch
    ragged = [n for n in ok if all((n * t) % 64 for t in threads_per_patch)]
    return (ragged or ok)[0]


def _fwd_threads(outvox, C_):
    """Threads per patch of k_pool_fwd's launch: one per element, per voxel (4, 8, 16, 32 channels) or per 4 channels."""
    return outvox * C_ if C_ % 4 else outvox if C_ in _VOX_C else outvox * C_ // 4


def _geom(name):
    """(size as (D, H, W), window as [wz, wy, wx], pooled size) of a geometry of the table."""
    size, w = GEOMETRIES[name]
    size3 = (1,) * (3 - len(size)) + tuple(size)
    w3 = pool_ref.win3(w)
    return size3, w3, pool_ref.geometry(size3, w3)[0]


def _pool_spec(name, extended):
    size, w = GEOMETRIES[name]
    if extended:
        return ['pool', list(w)]
    assert len(size) == 2 and w[0] == w[1]
    return [[w[0], w[0]], 'pool']      # NN.CNN: [[window, stride], 'pool']


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same_bits(got, want, msg):
    g, w = _bits(got).ravel(), _bits(want).ravel()
    assert g.shape == w.shape, (msg, got.shape, want.shape)
    bad = np.flatnonzero(g != w)
    if bad.size:      # where, and what: a failure here is a wrong window origin, offset or routing, never rounding
        gf, wf = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
        first = ', '.join('[%d] %r != %r' % (i, float(gf[i]), float(wf[i])) for i in bad[:8])
        raise AssertionError('%s: %d of %d elements differ, flat indices %d .. %d: %s' % (msg, bad.size, g.size, bad[0], bad[-1], first))


def _assert_sums(got, terms, msg):
    """Channel sums [N, D, H, W] against the fp64 sum of the exact fp32 terms [N, D, H, W, C]."""
    s, a = pool_ref.chan_sums64(terms)
    bound = pool_ref.sum_bound(a, terms.shape[-1])
    err = np.abs(got.astype(np.float64).reshape(s.shape) - s)
    print('%s: max err %.3e, max bound %.3e, worst err / bound %.3f'
          % (msg, err.max(), bound.max(), np.max(err / np.maximum(bound, 1e-300) * (err > 0))))
    assert np.all(err <= bound), (msg, float((err - bound).max()))


def _designed_input(n, size, C_, seed):
    """[n, *size, C]: a palette with many exact ties, zeros of both signs and magnitudes from 1e-3 to 1e4, mixed with
    normal draws; patch 0 is negative throughout, patch 1 mostly zeros of either sign."""
    rs = np.random.RandomState(seed)
    shape = (n,) + tuple(size) + (C_,)
    palette = np.array([-1e4, -2.5, -1., -1e-3, -0., 0., 1e-3, 1., 2.5, 1e4], np.float32)
    x = palette[rs.randint(len(palette), size=shape)]
    draws = (rs.randn(*shape) * 10. ** rs.randint(-2, 3, size=shape)).astype(np.float32)
    x = np.where(rs.rand(*shape) < 0.3, draws, x).astype(np.float32)
    x[0] = -np.abs(x[0]) - np.float32(0.25)
    zeros = np.where(rs.rand(*shape[1:]) < 0.5, np.float32(-0.), np.float32(0.))
    x[1] = np.where(rs.rand(*shape[1:]) < 0.8, zeros, x[1])
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    return x


def _check_forward(sess, m, n, layer, x5, w3, sums, tag):
    """The pool at `layer` of the last pass against its input x5 [n, D, H, W, C]: values and arg-max bytes on equal bits, the
    channel sums of its output (Fisher passes) within the sum bound.  Returns (out, argmax) of the reference."""
    want, arg = pool_ref.pool_fwd(x5, w3)
    cnt = want.size
    got = _copy(sess, m, layer, 0, n, cnt).reshape(want.shape)
    _assert_same_bits(got, want, tag + ': pooled values')
    got_arg = _copy(sess, m, layer, 13, n, cnt // 4).view(np.uint8).reshape(arg.shape)
    np.testing.assert_array_equal(got_arg, arg, err_msg=tag + ': arg-max bytes')
    if sums:
        _assert_sums(_copy(sess, m, layer, 11, n, cnt // want.shape[-1]), want, tag + ': sums of the pooled output')
    return want, arg


# ------------------------------------------------------------------------------------------ 1. forward, P-first
def _p_first(name, C_):
    size, w = GEOMETRIES[name]
    ext = len(size) == 3
    ld = OrderedDict([('pool1', _pool_spec(name, ext)), ('fc', ['fc', [2]] if ext else [2, 'fc'])])
    in_shape = tuple(size) + (C_,)
    return ld, in_shape, netspec.he_init(ld, in_shape, seed=31, bias_std=0.05)


@pytest.mark.parametrize('geom,C_,form', FWD_CASES, ids=['%s-C%d' % c[:2] for c in FWD_CASES])
def test_pool_forward_on_designed_inputs(sess, geom, C_, form):
    """pool -> fc(2) in the NN.CNN schema (2-D) / the extended schema (3-D), a forward-only pass (no sums) and a Fisher pass
    (sums: in-thread in the voxel-per-thread form, the channel-sum kernel behind the others)."""
    size3, w3, out3 = _geom(geom)
    outvox = int(np.prod(out3))
    n = _pick_n(outvox * C_, [_fwd_threads(outvox, C_)])
    ld, in_shape, pars = _p_first(geom, C_)
    x = _designed_input(n, in_shape[:-1], C_, seed=500 + C_)
    x5 = x.reshape((n,) + size3 + (C_,))
    m = _model(sess, ld, in_shape, pars, n)
    t = _dev(sess, x)
    tag = '%s C=%d N=%d (%s)' % (geom, C_, n, form)
    m.forward_device(t, n)
    want, arg = _check_forward(sess, m, n, 0, x5, w3, False, tag + ', forward only')
    r = m.fisher_device(t, n, None, 1e-3, want=('p1', 'g0', 'g1'))
    _check_forward(sess, m, n, 0, x5, w3, True, tag + ', Fisher pass')
    assert np.isfinite(r['p1'].cpu().numpy()).all()
    m.close()
    assert (want[0] < 0).all(), 'patch 0 is negative throughout: no padding cell may win'
    if int(np.prod(w3)) > 128 and n * outvox * C_ >= 64:
        assert arg.max() > 127


def test_layer_0_pool_under_a_fisher_pass(sess):
    """A pool on the network input has nothing below it that takes a cotangent: the Fisher pass launches no pool backward for
    it (as the general path) and its outputs are finite and the same bits on every run."""
    geom, C_, n = '7x5_w2', 8, 6
    ld, in_shape, pars = _p_first(geom, C_)
    x = np.random.RandomState(77).randn(n, *in_shape).astype(np.float32)      # moderate logits: neither saturation branch
    m = _model(sess, ld, in_shape, pars, n)
    t = _dev(sess, x)
    keys = ('p1', 'g0', 'g1', 'A', 'trace', 'Asum')
    runs = []
    for _ in range(2):
        r = m.fisher_device(t, n, None, 1e-3, want=keys)
        runs.append({k: r[k].cpu().numpy() for k in keys})
    g, _, _ = m.param_grads_device(t, n, 0, cls=1)
    assert np.isfinite(g.cpu().numpy()).all()
    m.close()
    for k in keys:
        assert np.isfinite(runs[0][k]).all(), k
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
    assert runs[0]['A'].shape == (n, 1, 1) and np.all((runs[0]['p1'] > 0) & (runs[0]['p1'] < 1))


# ------------------------------------------------------------------------------------------ 2. backward, conv-below
def _conv_below(name, C_, k, order, extra):
    size, w = GEOMETRIES[name]
    nd = len(size)
    ld = OrderedDict()
    if extra:
        ld['conv0'] = ['conv', [8, [3] * nd], 'MA']
    ld['conv1'] = ['conv', [C_, [k] * nd], order]
    ld['pool1'] = _pool_spec(name, True)
    ld['fc'] = ['fc', [2]]
    in_shape = tuple(size) + (1,)
    return ld, in_shape, netspec.he_init(ld, in_shape, seed=41 + C_, bias_std=0.05), (1 if extra else 0)


def _run(sess, m, t, n, path):
    if path == 'general':
        g, _, _ = m.param_grads_device(t, n, 0, cls=1)
        assert np.isfinite(g.cpu().numpy()).all()
    else:
        r = m.fisher_device(t, n, None, 1e-3, want=('p1', 'g0', 'g1'))
        assert np.isfinite(r['g0'].cpu().numpy()).all()


def _check_conv_below(sess, m, n, li, size3, w3, C_, relu, fisher, stored, tag):
    """After a pass: the pool at li + 1 against the conv's activation, the conv's cotangent and its channel sums against the
    pool's own cotangent routed through the reference.  Returns the device's sums of the conv's cotangent."""
    act = _copy(sess, m, li, 0, n, n * int(np.prod(size3)) * C_).reshape((n,) + size3 + (C_,))
    want, arg = _check_forward(sess, m, n, li + 1, act, w3, fisher, tag)
    dpool = _copy(sess, m, li + 1, 1, n, want.size).reshape(want.shape)
    assert np.abs(dpool).max() > 0
    din = pool_ref.pool_bwd(dpool, arg, size3, w3, act=act if relu else None)
    assert np.count_nonzero(din) > 0
    if stored:
        _assert_same_bits(_copy(sess, m, li, 1, n, din.size).reshape(din.shape), din, tag + ": the conv's cotangent")
    dsum = _copy(sess, m, li, 3, n, din.size // C_)
    _assert_sums(dsum, din, tag + ": sums of the conv's cotangent")
    return dsum, din


def _bwd_threads(form, invox, C_):
    """Threads per patch of a backward form: one per element, per 4 channels, or per voxel."""
    return invox * C_ if 'scalar' in form else invox * C_ // 4 if 'vec' in form else invox


@pytest.mark.parametrize('geom,C_,k,order,extra,path,form', BWD_CASES, ids=['%s-C%d-%s-%s' % (c[0], c[1], c[3], c[5]) for c in BWD_CASES])
def test_pool_backward_below_a_conv(sess, geom, C_, k, order, extra, path, form):
    size3, w3, out3 = _geom(geom)
    invox, outvox = int(np.prod(size3)), int(np.prod(out3))
    n = _pick_n(outvox * C_, [_bwd_threads(form, invox, C_)])
    ld, in_shape, pars, li = _conv_below(geom, C_, k, order, extra)
    m = _model(sess, ld, in_shape, pars, n)
    x = np.random.RandomState(600 + C_).randn(n, *in_shape).astype(np.float32)
    _run(sess, m, _dev(sess, x), n, path)
    # a Fisher pass stores nothing but the sums for the first parameterised layer where the voxel-per-thread form runs
    stored = not (path == 'fisher' and li == 0 and C_ in (4, 8))
    assert stored == (not form.startswith('pool_bwd_vox'))
    _check_conv_below(sess, m, n, li, size3, w3, C_, 'A' in order, path == 'fisher', stored, '%s C=%d N=%d %s (%s)' % (geom, C_, n, path, form))
    m.close()


@pytest.mark.parametrize('geom,C_', FIRST_CASES, ids=['%s-C%d' % c for c in FIRST_CASES])
def test_pool_backward_first_layer_scatter(sess, geom, C_):
    """pool_bwd_first<C / 4> (one thread per pooled voxel scatters the masked cotangent into the first conv's sums; nothing
    else is stored) and, under alq_debug_set(6, 1), the route without it (pool_bwd_vox<1, 2> for 4 and 8 channels, sums only;
    pool_bwd_vec<4> for 16, which stores the cotangent).  Both against the reference; the two associate the sums differently,
    so they agree within the sum bound, not bit for bit."""
    size3, w3, out3 = _geom(geom)
    invox, outvox = int(np.prod(size3)), int(np.prod(out3))
    n = _pick_n(outvox * C_, [outvox, invox])
    ld, in_shape, pars, li = _conv_below(geom, C_, 3, 'MA', False)
    m = _model(sess, ld, in_shape, pars, n)
    t = _dev(sess, np.random.RandomState(700 + C_).randn(n, *in_shape).astype(np.float32))
    tag = '%s C=%d N=%d ' % (geom, C_, n)
    _run(sess, m, t, n, 'fisher')
    first, din = _check_conv_below(sess, m, n, li, size3, w3, C_, True, True, False, tag + 'pool_bwd_first<%d>' % (C_ // 4))
    with _knob(sess, 6):
        _run(sess, m, t, n, 'fisher')
        plain, din2 = _check_conv_below(sess, m, n, li, size3, w3, C_, True, True, C_ == 16, tag + 'without pool_bwd_first')
    m.close()
    _assert_same_bits(din2, din, 'the two passes see the same tensors')
    bound = pool_ref.sum_bound(pool_ref.chan_sums64(din)[1], C_).ravel()
    assert np.all(np.abs(first.astype(np.float64) - plain.astype(np.float64)) <= bound)


# ------------------------------------------------------------------------------------------ 3. accumulate
@pytest.mark.parametrize('width', list(ACCUMULATE))
def test_pool_backward_accumulates_into_a_skip_source(sess, width):
    """netspec.net_c_2d with enc1 - pooled AND the skip source of dec1 - at 6, 12 and 8 channels: the pool's backward adds to
    what dec1's backward wrote (accumulate = 1: pool_bwd_vec<0>, and in a Fisher pass at 8 channels pool_bwd_first<2>; at 6
    channels - the scalar kernel - the library refuses the model's concat, see ACCUMULATE).  The consumer's part cannot be read on its own after the pass, so alq_param_grads and the Fisher
    pass's shrunk gradients are held to the fp64 oracle as tests/test_gpu_grads_fp64.py holds NET-C: patches without a
    fragile decision in fp64, the parameter gradients under that file's grad_bar, the shrunk gradients under the bar of its
    layer-sum check (2 e(rows of the general path) + 6e-8 mean |entry|)."""
    import torch
    from nnal_amd._lib import AlqError
    from oracle.model import OracleModel
    from tests.test_gpu_grads_fp64 import grad_bar, mode1_refs
    from tests.test_gpu_hvp import fragile_units
    ld, sk = netspec.net_c_2d()
    ld['enc1'] = ['conv', [width, [3, 3]], 'MA']
    in_shape, n = (8, 12, 1), 4
    pars = netspec.he_init(ld, in_shape, seed=90 + width, skips=sk, bias_std=0.05)
    if ACCUMULATE[width] is not None:      # a refused geometry stays in the table: the refusal and its message are the check
        m = _model(sess, ld, in_shape, pars, n, sk)
        t = _dev(sess, np.random.RandomState(190 + width).randn(n, *in_shape).astype(np.float32))
        for call in (lambda: m.param_grads_device(t, n, 0, cls=0), lambda: m.fisher_device(t, n, None, 1e-3, want=('p1', 'g0', 'g1'))):
            with pytest.raises(AlqError) as ei:
                call()
            print('width %d refused: %s' % (width, ei.value))
            assert str(ei.value) == 'libalq error -4: ' + ACCUMULATE[width]
        m.close()
        return
    om64 = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
    om32 = OracleModel(ld, in_shape, pars, skips=sk)
    xs = np.random.RandomState(190 + width).randn(16, *in_shape).astype(np.float32)
    chosen = [i for i in range(len(xs)) if fragile_units(om64, xs[[i]]) == 0][:n]
    assert len(chosen) == n, 'too few patches without a fragile decision: pick another seed'
    x = xs[chosen]
    labels = np.array([0, 1, 1, 0], np.int32)
    g64 = [[[np.asarray(a, np.float64) for a in om64.grad_log_post(j, x[[i]])] for j in (0, 1)] for i in range(n)]
    g32 = [[[np.asarray(a) for a in om32.grad_log_post(j, x[[i]])] for j in (0, 1)] for i in range(n)]
    names = list(pars.keys())
    arrays = [nme + s for nme in names for s in ('/W', '/b')]
    d = dict(n=n, labels=labels, g64=g64, g32=g32, om32=om32, x=x)
    m = _model(sess, ld, in_shape, pars, n, sk)
    t = _dev(sess, x)
    variants = []
    for cls in (0, 1):
        rows = m.param_grads_device(t, n, 0, cls=cls)[0].cpu().numpy()
        variants.append(('mode 0 class %d' % cls, [m.unflatten(rows[i]) for i in range(n)], [g64[i][cls] for i in range(n)],
                         [g32[i][cls] for i in range(n)]))
    rows64, rows32, sum64, sum32 = mode1_refs(d)
    rows = m.param_grads_device(t, n, 1, labels=labels, loss_scale=1. / n)[0].cpu().numpy()
    variants.append(('mode 1 rows', [m.unflatten(rows[i]) for i in range(n)], rows64, rows32))
    g = m.param_grads_device(t, n, 1, labels=labels, loss_scale=1. / n, per_sample=False)[0].cpu().numpy()
    variants.append(('mode 1 sum', [m.unflatten(g)], [sum64], [sum32]))
    bad = []
    for what, gd, r64, r32 in variants:
        for k, arr in enumerate(arrays):
            a64, ad, a32 = (np.stack([r[k] for r in rr]) for rr in (r64, gd, r32))
            assert ad.shape == a64.shape == a32.shape and ad.dtype == np.float32, (what, arr)
            e_dev, e_32 = np.abs(ad - a64).max(), np.abs(a32 - a64).max()
            bar = grad_bar(e_32, a64)
            print('width %d | %s | %s | e_dev %.3e | e_32 %.3e | bar %.3e' % (width, what, arr, e_dev, e_32, bar))
            if not e_dev <= bar:
                bad.append((what, arr, e_dev, bar))
    assert not bad, (width, bad)
    # the Fisher pass: g0 / g1 = the shrunk gradients of log posteriors[0 / 1]
    L = m.L
    s64 = np.array([[alpath.shrink_gradient(g64[i][j]) for j in (0, 1)] for i in range(n)])
    mean_abs = np.array([[[(np.abs(gr[2 * q]).sum() + np.abs(gr[2 * q + 1]).sum()) / (gr[2 * q].size + gr[2 * q + 1].size)
                           for q in range(L)] for gr in (g64[i][0], g64[i][1])] for i in range(n)]).mean(axis=(0, 1))
    g_rows = m.shrunk_class_gradients(x)[0].cpu().numpy()
    r = m.fisher_device(t, n, None, 1e-3, want=('p1', 'g0', 'g1'))
    p1 = r['p1'].cpu().numpy()
    assert np.all((p1 > 1e-3) & (p1 < 1 - 1e-3)), p1      # no saturation branch: both gradients are produced
    g_fisher = np.stack([r['g0'].cpu().numpy(), r['g1'].cpu().numpy()], axis=1)
    m.close()
    assert g_fisher.shape == g_rows.shape == s64.shape == (n, 2, L)
    e_fisher = np.abs(g_fisher - s64).max(axis=(0, 1))
    e_rows = np.abs(g_rows - s64).max(axis=(0, 1))
    bar = 2 * e_rows + 6e-8 * mean_abs
    for q in range(L):
        print('width %d layer %d (%s): e(Fisher) %.3e  e(rows) %.3e  floor %.3e  bar %.3e' % (width, q, names[q], e_fisher[q], e_rows[q], 6e-8 * mean_abs[q], bar[q]))
    assert np.all(e_fisher <= bar), (width, e_fisher, bar)


# ------------------------------------------------------------------------------------------ 4. grid stride
def _tied_input(n, in_shape, seed):
    """Small integers and zeros of both signs: ties in most windows."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, size=(n,) + tuple(in_shape)).astype(np.float32)
    x[rs.rand(*x.shape) < 0.1] = -0.
    return x


@pytest.mark.parametrize('form,in_shape,n', STRIDE_FWD, ids=[c[0] for c in STRIDE_FWD])
def test_forward_beyond_the_grid_cap(sess, form, in_shape, n):
    H, W, C_ = in_shape
    threads = n * _fwd_threads(H * (W // 2), C_)
    assert threads > GRID_CAP_THREADS and n * H * W * C_ * 4 < 128 << 20
    ld = OrderedDict([('pool1', ['pool', [1, 2]]), ('fc', ['fc', [2]])])
    pars = netspec.he_init(ld, in_shape, seed=32, bias_std=0.05)
    x = _tied_input(n, in_shape, seed=800 + C_)
    m = _model(sess, ld, in_shape, pars, n)
    m.forward_device(_dev(sess, x), n)
    _check_forward(sess, m, n, 0, x.reshape(n, 1, H, W, C_), [1, 1, 2], False, '%s, %d threads' % (form, threads))
    m.close()


@pytest.mark.parametrize('form,C_,n', STRIDE_BWD, ids=[c[0] for c in STRIDE_BWD])
def test_backward_beyond_the_grid_cap(sess, form, C_, n):
    H = W = 64
    threads = n * H * W * (C_ if C_ % 4 else C_ // 4)
    assert threads > GRID_CAP_THREADS
    ld = OrderedDict([('conv1', ['conv', [C_, [1, 1]], 'MA']), ('pool1', ['pool', [1, 2]]), ('fc', ['fc', [2]])])
    in_shape = (H, W, 1)
    pars = netspec.he_init(ld, in_shape, seed=33, bias_std=0.05)
    x = _tied_input(n, in_shape, seed=900 + C_)
    m = _model(sess, ld, in_shape, pars, n)
    labels = (np.arange(n) % 2).astype(np.int32)
    g, _, _ = m.param_grads_device(_dev(sess, x), n, 1, labels=labels, loss_scale=1. / n, per_sample=False)
    assert np.isfinite(g.cpu().numpy()).all()
    _check_conv_below(sess, m, n, 0, (1, H, W), [1, 1, 2], C_, True, False, True, '%s, %d threads' % (form, threads))
    m.close()
