"""The streaming GEMM of the wide fully connected layers (csrc/fcgemm.hip) on its own: every kernel form and scaling regime against
the fp64 statement of the layer (GPU box).

The engine has four kernel instantiations (bf16 triples on 64-unit tiles; fp16 pairs on 64-unit tiles, on 128-unit tiles with
64 x 64 wave tiles and with tall 128 x 32 wave tiles), three scaling regimes (none; per-row maxima measured by fc_rowmax_kernel,
forward launches; the static cotangent bound, backward launches of a Fisher pass) and its own dispatch (fcgemm_build_plan,
fc16_go, plan_fc's swapped backward Gemm, gemm_route under the debug knobs).  The rest of the suite runs it at N % 128 == 0 only,
end to end through a two-class head.  Here: the shapes of SHAPES, through device.DeviceModel, internals read with
alq_model_debug_copy; every case asserts from alq_fcgemm_geometry and from the igemm_f16x2 launch count of the profiler that it is
in the regime it names.

Models (extended schema):
  first-layer   fc_t(K -> N, 'M' | 'MA') -> fc(2) on in_shape (1, 1, K): alq_model_create takes an fc first layer as it is (no conv
                in front was needed).  The layer reads the caller's x.
  below-fc      fc0(64 -> K, 'MA') -> fc_t(K -> N) -> fc(2) on in_shape (1, 1, 64): fc_t has a backward Gemm (K and N swapped).
  whole         conv(16, 3x3) -> pool(2) -> fc(256 -> 320, 'MA') -> fc(320 -> 256, 'MA') -> fc(c) on 8 x 8 inputs.

Checks:
  1  first-layer models, EXACT: tests/fcgemm_ref.py's dense small integers and piece probes (with the row patterns 'one' and
     'mixed': rows 2^-40 .. 2^40 apart, all-zero rows, rows whose maximum is a power of two, rows at 2^-100) - the output must
     equal the fp64 statement bit for bit after alq_forward and after alq_fisher, on every route, every batch size of BATCHES
     under max_batch = 257 and 200 patches as 128 + 72 under max_batch = 128.  The 'mixed' pattern runs without bias: an integer
     bias and a 2^-40 product have no common q (fcgemm_ref, condition 1); with bias the 'one' pattern and the dense sets.
  2  batch invariance on float inputs: a row's bits do not depend on M, its place in the tile or its neighbours.
  3  the tall, square and 64-wide forms give the same bits on float inputs, forward and backward.
  4  below-fc models on float inputs: the layer's input activation and its own cotangent are read from the device and taken as
     given; output, masked cotangent of fc0, dW and db rows follow from them in fp64.  Tolerance below.
  5  below-fc models with integer weights in fc_t and the head: the backward Gemm of a Fisher pass (fp16 pairs under the static
     bound) and under ALQ_NO_FC_F16 (bf16 triples) must equal the fp64 statement exactly; the bound covers the cotangent read.
  6  whole models against OracleModel(dtype=float64) under the bars the suite holds NET-C to.

Tolerance of check 4 (tests/test_gpu_convt.py's convention): per compared array e_dev = max |dev - ref64|, e_32 = max |ref32 -
ref64| with ref32 the same operation in fp32 torch on the same inputs; e_dev <= 4 R e_32 + 6e-8 mean |ref64|, never looser than
2e-4 max |ref64| + 1e-9.  Rows of many magnitudes (test_forward_rows_of_many_magnitudes): the same per row.  Every figure is
printed before it is asserted.  Checks 1, 2, 3 and 5 have no tolerance."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import alpath, netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests import convt_ref, factored_ref, hvp_cases  # noqa: E402
from tests import fcgemm_ref as R  # noqa: E402
from tests.test_gpu_grads_fp64 import grad_bar, mode1_refs, smallest_key  # noqa: E402
from tests.test_gpu_hvp import EPS, bars, fragile_units, oracle_hv  # noqa: E402

# Largest e_dev / e_32 over the 712 figures of check 4 and of test_forward_rows_of_many_magnitudes (every shape, route, pass and
# variant; the per-row test contributes its worst row) whose e_dev exceeds the floor 6e-8 mean |ref64| (below it the floor alone
# carries the assertion and e_32 may be 0), measured on an MI355X on 2026-10-20: 4.398 at 288 -> 384 'MA', rows of many magnitudes,
# row 11 (scaled by 2^-38) on the control arm ALQ_NO_FCGEMM=1 (the general engines; e_dev 2.245e-17, e_32 5.105e-18, max |ref64|
# 2.48e-11: 9.1e-07 relative).  The streaming GEMM's own largest figures are 3.303 (256 -> 256, bf16 triples, row 25), 2.776
# (288 -> 384 'MA', the cotangent below, bf16 triples) and 2.449 on per-row fp16 pairs (256 -> 320, row 215); dW rows 1.000.
# tests/test_gpu_convt.py's figure is 5.092, NET-C's 3.004.  DESIGN.md has the table.
R_DEV_OVER_F32 = 4.398
R_FACTOR = 4.0

# K -> N of the layer under test: (forward wide, forward k-steps, backward wide).  The backward Gemm is N -> K.
SHAPES = OrderedDict([
    ((256, 256), (True, 8, True)),       # 128-unit tiles both ways
    ((256, 320), (True, 8, True)),       # forward: 64-unit tiles by dispatch (320 % 128 != 0); backward 128-unit tiles, 10 k-steps
    ((320, 256), (True, 10, True)),      # the mirror image: the backward Gemm on 64-unit tiles
    ((288, 384), (True, 9, False)),      # an odd number of k-steps, 3 column tiles; backward not wide (288 % 64 != 0)
    ((384, 288), (False, 0, True)),      # forward on the general engines; backward wide, 9 k-steps
    ((512, 256), (True, 16, True)),
    ((224, 256), (False, 0, False)),     # K < 256: never on this engine
])
SHAPE_IDS = ['%dto%d' % s for s in SHAPES]
BATCHES = (1, 63, 64, 65, 127, 128, 129, 257)

# name -> (environment around model creation, alq_debug_set knob around the calls, on fcgemm, fp16 forward, fp16 backward, form)
ROUTES = OrderedDict([
    ('default', ({}, None, True, True, True, 0)),
    ('no_fc_f16_fwd', ({'ALQ_NO_FC_F16_FWD': '1'}, None, True, False, True, 0)),
    ('no_fc_f16', ({'ALQ_NO_FC_F16': '1'}, None, True, True, False, 0)),
    ('square', ({'ALQ_FC_SQUARE': '1'}, None, True, True, True, 1)),
    ('bn64', ({'ALQ_FC_BN64': '1'}, None, True, True, True, 2)),
    ('no_f16x2', ({'ALQ_NO_F16X2': '1'}, None, True, False, False, 0)),
    ('no_fcgemm', ({'ALQ_NO_FCGEMM': '1'}, None, False, False, False, 0)),      # the same layer on the general engines: the control arm
    ('knob4', ({}, 4, False, False, False, 0)),
])
SWITCHES = ('ALQ_NO_FC_F16_FWD', 'ALQ_NO_FC_F16', 'ALQ_FC_SQUARE', 'ALQ_FC_BN64', 'ALQ_NO_F16X2', 'ALQ_NO_FCGEMM')


# ------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


class _env(object):
    """The switches of a route and nothing else of SWITCHES for the block."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in set(SWITCHES) | set(self.env)}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class _knob(object):
    """alq_debug_set(key, 1) for the block (None: nothing)."""

    def __init__(self, sess, key):
        self.sess, self.key = sess, key

    def _set(self, v):
        from nnal_amd._lib import check
        if self.key is not None:
            check(self.sess.lib.alq_debug_set(self.key, v))

    def __enter__(self):
        self._set(1)

    def __exit__(self, *exc):
        self._set(0)


def _make(sess, ld, in_shape, pars, mb, route='default', extra_env=None, device_weights=False):
    from nnal_amd import device
    env = dict(ROUTES[route][0])
    env.update(extra_env or {})
    with _env(env):
        m = device.DeviceModel(sess, ld, in_shape, (), max_batch=mb)
        assert m.max_batch == mb
        _set(sess, m, pars, device_weights)
    m._route_env = env
    return m


def _set(sess, m, pars, device_weights=False):
    """Weights are packed under the model's creation switches."""
    torch = sess.torch
    with _env(getattr(m, '_route_env', {k: v for k, v in os.environ.items() if k in SWITCHES})):
        if device_weights:
            m.set_weights_device(OrderedDict((nme, (sess.to_device(np.ascontiguousarray(W, dtype=np.float32), torch.float32),
                                                    sess.to_device(np.ascontiguousarray(b, dtype=np.float32), torch.float32)))
                                             for nme, (W, b) in pars.items()))
        else:
            m.set_weights(pars)


def _copy(sess, m, layer, what, n, shape, dtype=np.float32):
    """alq_model_debug_copy of the last pass as an array of `shape` (its size must come back)."""
    from nnal_amd._lib import check
    torch = sess.torch
    expect = int(np.prod(shape))
    e = C.c_int64()
    buf = torch.zeros((expect + 64,), dtype=torch.float32, device=sess.device)
    check(m.lib.alq_model_debug_copy(m._m, int(layer), int(what), int(n), C.c_void_p(buf.data_ptr()), C.byref(e)))
    torch.cuda.synchronize()
    assert e.value == expect, (layer, what, e.value, expect)
    return buf[:expect].cpu().numpy().view(dtype).reshape(shape)


def _dev(sess, x):
    return sess.to_device(np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1), sess.torch.float32)


def _passes(n, mb):
    return [(a, min(n, a + mb)) for a in range(0, n, mb)]


def _geometry(sess, K, N, M, route='default'):
    buf = (C.c_int * 6)(*([-1] * 6))
    with _env(ROUTES[route][0]):
        assert sess.lib.alq_fcgemm_geometry(K, N, M, buf) == 0
    return tuple(buf)


def _f16_launches(sess, fn):
    """The igemm_f16x2 launch count of the profiler over fn()."""
    sess.prof_reset()
    sess.prof_enable(1)
    try:
        fn()
        sess.torch.cuda.synchronize()
    finally:
        sess.prof_enable(False)
    return sess.prof_read()['igemm_f16x2']['launches']


def first_layer(K, N, ops):
    return OrderedDict([('fct', ['fc', [N], ops]), ('head', ['fc', [2]])]), (1, 1, K)


def below_fc(K, N, ops):
    return OrderedDict([('fc0', ['fc', [K], 'MA']), ('fct', ['fc', [N], ops]), ('head', ['fc', [2]])]), (1, 1, 64)


def _fc_pars(ld, in_shape, seed, **arrays):
    """he_init with given arrays put in: name -> (W, b)."""
    pars = netspec.he_init(ld, in_shape, seed=seed, bias_std=0.05)
    for nme, (W, b) in arrays.items():
        assert pars[nme][0].shape == np.shape(W), (nme, pars[nme][0].shape, np.shape(W))
        pars[nme] = [np.asarray(W, np.float32), np.asarray(b, np.float32).reshape(pars[nme][1].shape)]
    return pars


def _small_head(N, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(-15, 16, size=(2, N)).astype(np.float32), np.zeros(2, np.float32)


def _assert_regime(sess, K, N, M, route, cell):
    """alq_fcgemm_geometry under the route's switches against the table and the reference arithmetic of the launch."""
    wide, nks = cell
    form = ROUTES[route][5]
    g = _geometry(sess, K, N, M, route)
    assert g == R.geometry(K, N, M, form), (K, N, M, route, g)
    assert g[0] == int(wide) and g[5] == nks, (K, N, route, g)
    if wide:
        want_bn = 64 if (N % 128 or form == 2) else 128
        assert g[1] == want_bn and g[2] == int(want_bn == 128 and form == 0) and g[3] == N // want_bn and g[4] == -(-M // 128), g
    return g


def _bar(e32, a64):
    a64 = np.asarray(a64)
    floor = 6e-8 * np.abs(a64).mean()
    return min(R_FACTOR * R_DEV_OVER_F32 * e32 + floor, 2e-4 * np.abs(a64).max() + 1e-9), floor


def _figure(bad, tag, what, dev, r64, r32):
    """Prints e_dev, e_32 and their ratio, then records a miss of the bar of the module docstring in `bad`."""
    dev, r64, r32 = np.asarray(dev), np.asarray(r64, np.float64), np.asarray(r32)
    assert dev.shape == r64.shape == r32.shape and dev.dtype == np.float32 and r32.dtype == np.float32, (tag, what, dev.shape, r64.shape, r32.shape)
    e_dev, e_32 = np.abs(dev - r64).max(), np.abs(r32 - r64).max()
    bar, floor = _bar(e_32, r64)
    print('FCGEMM_FIG | %s | %s | e_dev %.3e | e_32 %.3e | ratio %.3f | floor %.3e | above_floor %d | max|ref| %.3e | bar %.3e'
          % (tag, what, e_dev, e_32, e_dev / max(e_32, 1e-300), floor, e_dev > floor, np.abs(r64).max(), bar))
    if not e_dev <= bar:
        bad.append((tag, what, e_dev, e_32, bar))


# ------------------------------------------------------------------------------------------ 0. the table's cells
@pytest.mark.parametrize('shape', list(SHAPES), ids=SHAPE_IDS)
def test_table_regimes(sess, shape):
    """Every cell of the table through alq_fcgemm_geometry, and through the profiler on a below-fc model: the fp16-pair launches
    of a Fisher pass with the fc switches on, less those with the forward resp. the backward one off, are the forward resp. the
    backward launch of fc_t exactly where the table says the Gemm is wide (fc0 and the head never run on this engine)."""
    K, N = shape
    fwd_wide, nks, bwd_wide = SHAPES[shape]
    M = 70
    for route in ROUTES:
        _assert_regime(sess, K, N, M, route, (fwd_wide, nks))
        _assert_regime(sess, N, K, M, route, (bwd_wide, N // 32 if bwd_wide else 0))
    ld, in_shape = below_fc(K, N, 'MA')
    pars = netspec.he_init(ld, in_shape, seed=3, bias_std=0.05)
    t = _dev(sess, np.random.RandomState(4).randn(M, 64))
    counts = {}
    for name, env in (('on', {}), ('fwd_off', {'ALQ_NO_FC_F16_FWD': '1'}), ('bwd_off', {'ALQ_NO_FC_F16': '1'}), ('control', {'ALQ_NO_FCGEMM': '1'}),
                      ('control_off', {'ALQ_NO_FCGEMM': '1', 'ALQ_NO_FC_F16_FWD': '1', 'ALQ_NO_FC_F16': '1'})):
        m = _make(sess, ld, in_shape, pars, M, extra_env=env)
        counts[name] = (_f16_launches(sess, lambda: m.fisher_device(t, M, None, 1e-3, want=('p1', 'g0', 'g1'))),
                        _f16_launches(sess, lambda: m.forward_device(t, M)),
                        _f16_launches(sess, lambda: m.param_grads_device(t, M, 0, cls=1)))
        m.close()
    print('FCGEMM_REGIME | %dto%d | igemm_f16x2 launches (Fisher pass, forward pass, alq_param_grads): %r' % (K, N, counts))
    on, fo, bo = counts['on'], counts['fwd_off'], counts['bwd_off']
    assert on[0] - fo[0] == int(fwd_wide) and on[1] - fo[1] == int(fwd_wide) and on[2] - fo[2] == int(fwd_wide)
    assert on[0] - bo[0] == int(bwd_wide)
    assert on[1] == bo[1] and on[2] == bo[2]      # no static bound outside a Fisher pass: the backward launch of alq_param_grads is on triples
    assert counts['control'] == counts['control_off']      # without the engine its switches change nothing


# ------------------------------------------------------------------------------------------ 1. exact forward, first-layer models
_SETS = {}


def exact_sets(K, N):
    """name -> (a [257, K], W, b, the fp64 statement without ReLU): computed once per shape, shared, never modified."""
    if (K, N) not in _SETS:
        sets = OrderedDict()
        for bias in (True, False):
            a, W, b = R.dense_ints(257, K, N, seed=1000 + K + N, bias=bias)
            sets['dense%s' % ('+b' if bias else '')] = (a, W, b)
            a, W, b, _ = R.probe_set(257, K, N, seed=K + N, bias=bias)
            sets['probes/one%s' % ('+b' if bias else '')] = (a, W, b)
        a, W, b, _ = R.probe_set(257, K, N, seed=K + N, bias=False)
        sets['probes/mixed'] = (R.row_pattern(a, 'mixed'), W, b)
        for nme, (a, W, b) in list(sets.items()):
            for form in ('pairs', 'triples'):
                R.assert_exact(a, W, b, form)
            want = R.forward64(a, W, b, False)
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want), nme
            sets[nme] = (a, W, b, want)
        _SETS[(K, N)] = sets
    return _SETS[(K, N)]


def _assert_equal(got, want, msg):
    got = got.astype(np.float64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ('%s: %d of %d outputs differ, first at %r: %r != %r' % (msg, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                                  want[tuple(bad[0])]))


@pytest.mark.parametrize('ops', ['M', 'MA'])
@pytest.mark.parametrize('shape', list(SHAPES), ids=SHAPE_IDS)
def test_exact_forward_on_integers_and_piece_probes(sess, shape, ops):
    K, N = shape
    fwd_wide, nks, _ = SHAPES[shape]
    ld, in_shape = first_layer(K, N, ops)
    sets = exact_sets(K, N)
    head = _small_head(N, 5)
    for route, (_, knob, on_fc, f16_fwd, _, _) in ROUTES.items():
        models = {}
        for sname, (a, W, b, want) in sets.items():
            if 'A' in ops:
                want = np.maximum(want, 0.)
            pars = _fc_pars(ld, in_shape, 1, fct=(W, b), head=head)
            t = _dev(sess, a)
            for mb, runs in ((257, [(0, M) for M in BATCHES]), (128, _passes(200, 128))):
                if mb not in models:
                    models[mb] = _make(sess, ld, in_shape, pars, mb, route)
                else:
                    _set(sess, models[mb], pars)
                m = models[mb]
                with _knob(sess, knob):
                    for lo, hi in runs:
                        n = hi - lo
                        _assert_regime(sess, K, N, n, route, (fwd_wide, nks))
                        for what in ('forward', 'Fisher') if n in (65, 257, 128, 72) else ('forward',):
                            if what == 'forward':
                                cnt = _f16_launches(sess, lambda: m.forward_device(t[lo:hi], n))
                            else:
                                cnt = _f16_launches(sess, lambda: m.fisher_device(t[lo:hi], n, None, 1e-3, want=('p1', 'g0', 'g1')))
                            if fwd_wide and on_fc:      # the model's only contraction launch: fc_t's forward Gemm
                                assert cnt == int(f16_fwd), (shape, ops, route, sname, what, cnt)
                            got = _copy(sess, m, 0, 0, n, (n, N))
                            _assert_equal(got, want[lo:hi], '%dto%d %s, route %s, set %s, %s pass, patches %d..%d under max_batch %d'
                                          % (K, N, ops, route, sname, what, lo, hi - 1, mb))
        for m in models.values():
            m.close()


# ------------------------------------------------------------------------------------------ 2, 3. batch invariance; forms agree
_FLOAT = {}


def float_case(K, N):
    """257 float patches whose rows lie 2^-40 .. 2^40 apart, He weights, biases: computed once, shared."""
    if (K, N) not in _FLOAT:
        ld, in_shape = first_layer(K, N, 'MA')
        pars = netspec.he_init(ld, in_shape, seed=20 + K, bias_std=0.05)
        x = np.random.RandomState(21 + N).randn(257, K).astype(np.float32)
        x = np.ldexp(x, R.spread_exp(np.arange(257))[:, None]).astype(np.float32)
        x[5] = 0
        _FLOAT[(K, N)] = (ld, in_shape, pars, x)
    return _FLOAT[(K, N)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('route', ['default', 'no_fc_f16_fwd', 'bn64'])
@pytest.mark.parametrize('shape', [(256, 256), (256, 320), (288, 384)], ids=['256to256', '256to320', '288to384'])
def test_rows_do_not_depend_on_the_batch(sess, shape, route):
    """Row i of the M = 257 pass == the same patch alone (M = 1) == the same patch in the 128 + 72 run, bit for bit: per-row fp16
    pairs (default; the 64-unit tiles too) and bf16 triples."""
    K, N = shape
    ld, in_shape, pars, x = float_case(K, N)
    t = _dev(sess, x)
    m = _make(sess, ld, in_shape, pars, 257, route)
    cnt = _f16_launches(sess, lambda: m.forward_device(t, 257))
    assert cnt == int(ROUTES[route][3]) and _geometry(sess, K, N, 257, route)[0] == 1
    full = _copy(sess, m, 0, 0, 257, (257, N))
    assert np.isfinite(full).all() and np.count_nonzero(full) > full.size // 4
    for i in (0, 5, 17, 63, 64, 65, 127, 128, 191, 192, 255, 256):
        m.forward_device(t[i:i + 1], 1)
        np.testing.assert_array_equal(_bits(_copy(sess, m, 0, 0, 1, (1, N))), _bits(full[i:i + 1]), err_msg='row %d alone' % i)
    # the same row in another tile position, among other neighbours
    m.forward_device(t[60:200], 140)
    np.testing.assert_array_equal(_bits(_copy(sess, m, 0, 0, 140, (140, N))), _bits(full[60:200]))
    m.close()
    m = _make(sess, ld, in_shape, pars, 128, route)
    for lo, hi in _passes(200, 128):
        for what in ('forward', 'Fisher'):
            if what == 'forward':
                m.forward_device(t[lo:hi], hi - lo)
            else:
                m.fisher_device(t[lo:hi], hi - lo, None, 1e-3, want=('p1', 'g0', 'g1'))
            np.testing.assert_array_equal(_bits(_copy(sess, m, 0, 0, hi - lo, (hi - lo, N))), _bits(full[lo:hi]), err_msg='%s pass %d..%d' % (what, lo, hi))
    m.close()


@pytest.mark.parametrize('shape', [(256, 256), (288, 384)], ids=['256to256', '288to384'])
def test_tile_forms_give_the_same_bits_forward(sess, shape):
    """Tall, square and 64-unit tiles: the same sums in the same order per output element (fcgemm.hip's own claim)."""
    K, N = shape
    ld, in_shape, pars, x = float_case(K, N)
    t = _dev(sess, x)
    outs = {}
    for route in ('default', 'square', 'bn64'):
        g = _geometry(sess, K, N, 257, route)
        assert g[:3] == {'default': (1, 128, 1), 'square': (1, 128, 0), 'bn64': (1, 64, 0)}[route]
        m = _make(sess, ld, in_shape, pars, 257, route)
        assert _f16_launches(sess, lambda: m.forward_device(t, 257)) == 1
        outs[route] = _copy(sess, m, 0, 0, 257, (257, N))
        m.close()
    assert np.isfinite(outs['default']).all() and np.count_nonzero(outs['default']) > 257 * N // 4
    for route in ('square', 'bn64'):
        np.testing.assert_array_equal(_bits(outs[route]), _bits(outs['default']), err_msg=route)


@pytest.mark.parametrize('shape', [(256, 256), (384, 288)], ids=['256to256', '384to288'])
def test_tile_forms_give_the_same_bits_backward(sess, shape):
    """The backward Gemm of a Fisher pass (fp16 pairs under the static bound; N -> K: 256 resp. 384 units, 3 column tiles) in the
    three forms: the cotangent of fc0 bit for bit."""
    K, N = shape
    ld, in_shape = below_fc(K, N, 'MA')
    pars = netspec.he_init(ld, in_shape, seed=31, bias_std=0.05)
    M = 129
    t = _dev(sess, np.random.RandomState(32).randn(M, 64))
    outs = {}
    for route in ('default', 'square', 'bn64', 'no_fc_f16'):
        assert _geometry(sess, N, K, M, route)[:3] == {'default': (1, 128, 1), 'square': (1, 128, 0), 'bn64': (1, 64, 0), 'no_fc_f16': (1, 128, 1)}[route]
        m = _make(sess, ld, in_shape, pars, M, route)
        cnt = _f16_launches(sess, lambda: m.fisher_device(t, M, None, 1e-3, want=('p1', 'g0', 'g1')))
        outs[route] = (_copy(sess, m, 0, 1, M, (M, K)), cnt)
        m.close()
    assert outs['default'][1] == outs['no_fc_f16'][1] + 1
    assert np.isfinite(outs['default'][0]).all() and np.count_nonzero(outs['default'][0]) > M * K // 8
    for route in ('square', 'bn64'):
        assert outs[route][1] == outs['default'][1]
        np.testing.assert_array_equal(_bits(outs[route][0]), _bits(outs['default'][0]), err_msg=route)
    assert not np.array_equal(_bits(outs['no_fc_f16'][0]), _bits(outs['default'][0]))      # the triples are another sum: the arms differ


# ------------------------------------------------------------------------------------------ 4. below-fc models, float
N4 = 70      # one pass; rows 64 .. 69 are the second staging rows of a thread in a ragged 128-row tile


@pytest.mark.parametrize('ops', ['M', 'MA'])
@pytest.mark.parametrize('shape', list(SHAPES), ids=SHAPE_IDS)
def test_forward_backward_and_gradients_below_an_fc_layer(sess, shape, ops):
    import torch
    K, N = shape
    fwd_wide, nks, bwd_wide = SHAPES[shape]
    ld, in_shape = below_fc(K, N, ops)
    seed = 400 + list(SHAPES).index(shape)
    pars = netspec.he_init(ld, in_shape, seed=seed, bias_std=0.05)
    W, b = pars['fct'][0], pars['fct'][1].reshape(-1)
    relu = 'A' in ops
    x = np.random.RandomState(seed + 1000).randn(N4, 64).astype(np.float32)
    labels = (np.arange(N4) % 2).astype(np.int32)
    t = _dev(sess, x)
    bad = []
    f16 = {}
    for route, (_, knob, on_fc, f16_fwd, f16_bwd, _) in ROUTES.items():
        m = _make(sess, ld, in_shape, pars, N4, route)
        variants = OrderedDict([('Fisher', None), ('mode 0 class 1', dict(mode=0, cls=1))])
        if route == 'default':
            variants.update([('mode 0 class 0', dict(mode=0, cls=0)), ('mode 1 rows', dict(mode=1, labels=labels, loss_scale=1. / N4)),
                             ('mode 1 sum', dict(mode=1, labels=labels, loss_scale=1. / N4, per_sample=False))])
        with _knob(sess, knob):
            for vname, kw in variants.items():
                rows = []
                if kw is None:
                    f16[route] = _f16_launches(sess, lambda: m.fisher_device(t, N4, None, 1e-3, want=('p1', 'g0', 'g1')))
                else:
                    cnt = _f16_launches(sess, lambda: rows.append(m.param_grads_device(t, N4, **kw)[0].cpu().numpy()))
                    f16[route + '/grads'] = cnt
                tag = '%dto%d-%s | %s | %s' % (K, N, ops, route, vname)
                act = _copy(sess, m, 0, 0, N4, (N4, K))
                y = _copy(sess, m, 1, 0, N4, (N4, N))
                dy = _copy(sess, m, 1, 1, N4, (N4, N))
                dlow = _copy(sess, m, 0, 1, N4, (N4, K))
                assert np.count_nonzero(act) and np.count_nonzero(dy) and (act >= 0).all(), tag
                y64, y32 = (R.forward_torch(act, W, b, relu, dt) for dt in (torch.float64, torch.float32))
                if relu:
                    assert not dy[y == 0].any(), (tag, 'the cotangent of an ReLU layer is not masked by its own output')
                _figure(bad, tag, 'output', y, y64, y32)
                _figure(bad, tag, 'cotangent below', dlow, R.din64(dy, W, act), R.din_torch(dy, W, act, torch.float32))
                if kw is None or not (route in ('default', 'no_fc_f16_fwd', 'no_fcgemm')):      # the rows are no product of this engine: three routes
                    continue
                rows = rows[0]
                dW64, db64 = R.wgrad64(act, dy)
                dW32, db32 = R.wgrad_torch(act, dy, torch.float32)
                if rows.ndim == 1:
                    rows, dW64, db64 = rows[None], dW64.sum(0, keepdims=True), db64.sum(0, keepdims=True)
                    dW32, db32 = dW32.sum(0, keepdims=True), db32.sum(0, keepdims=True)
                gW = np.stack([m.unflatten(r)[2] for r in rows])
                gb = np.stack([m.unflatten(r)[3].reshape(-1) for r in rows])
                _figure(bad, tag, 'dW', gW, dW64, dW32)
                _figure(bad, tag, 'db', gb, db64, db32)
        m.close()
    print('FCGEMM_REGIME | %dto%d-%s | igemm_f16x2 launches per route: %r' % (K, N, ops, f16))
    # both arms really ran: the Fisher pass's backward launch on fp16 pairs, alq_param_grads's on bf16 triples; the forward likewise
    assert f16['default'] - f16['no_fc_f16'] == int(bwd_wide) and f16['default'] - f16['no_fc_f16_fwd'] == int(fwd_wide)
    assert f16['default/grads'] == f16['no_fc_f16/grads'] and f16['default/grads'] - f16['no_fc_f16_fwd/grads'] == int(fwd_wide)
    assert f16['square'] == f16['bn64'] == f16['default']
    assert not bad, bad


@pytest.mark.parametrize('route', ['default', 'no_fc_f16_fwd', 'bn64', 'no_fcgemm'])
@pytest.mark.parametrize('shape', [(256, 256), (256, 320), (288, 384)], ids=['256to256', '256to320', '288to384'])
def test_forward_rows_of_many_magnitudes(sess, shape, route):
    """Per-row-scaled forward launch on rows 2^-40 .. 2^40 apart (first-layer model, zero bias so that every row keeps its
    magnitude): e_dev, e_32 and the bar per row."""
    import torch
    K, N = shape
    ld, in_shape, pars, x = float_case(K, N)
    pars = _fc_pars(ld, in_shape, 20 + K, fct=(pars['fct'][0], np.zeros(N)))
    W = pars['fct'][0]
    m = _make(sess, ld, in_shape, pars, 257, route)
    m.forward_device(_dev(sess, x), 257)
    y = _copy(sess, m, 0, 0, 257, (257, N))
    m.close()
    y64, y32 = (R.forward_torch(x, W, np.zeros(N, np.float32), True, dt) for dt in (torch.float64, torch.float32))
    bad = []
    worst = (0., None)
    for i in range(257):
        e_dev, e_32 = np.abs(y[i] - y64[i]).max(), np.abs(y32[i] - y64[i]).max()
        bar, floor = _bar(e_32, y64[i])
        if e_dev > floor and e_dev / max(e_32, 1e-300) > worst[0]:
            worst = (e_dev / max(e_32, 1e-300), i)
        if not e_dev <= bar:
            bad.append((i, e_dev, e_32, bar))
    i = worst[1] if worst[1] is not None else 0
    e_dev, e_32 = np.abs(y[i] - y64[i]).max(), np.abs(y32[i] - y64[i]).max()
    bar, floor = _bar(e_32, y64[i])
    print('FCGEMM_FIG | %dto%d-MA rows | %s | worst row %d (2^%d) | e_dev %.3e | e_32 %.3e | ratio %.3f | floor %.3e | above_floor %d | max|ref| %.3e | bar %.3e'
          % (K, N, route, i, R.spread_exp(i), e_dev, e_32, e_dev / max(e_32, 1e-300), floor, e_dev > floor, np.abs(y64[i]).max(), bar))
    assert not y[5].any() and not bad, bad[:5]


# ------------------------------------------------------------------------------------------ 5. exact backward in a Fisher pass
@pytest.mark.parametrize('ops', ['M', 'MA'])
@pytest.mark.parametrize('shape', [s for s in SHAPES if SHAPES[s][2]], ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if SHAPES[s][2]])
def test_exact_backward_in_a_fisher_pass(sess, shape, ops):
    """Integer weights (|w| <= 15) in fc_t and the head: the cotangent at fc_t's output is (W_head[0] - W_head[1]), masked by the
    layer's own ReLU, and the backward Gemm's result an integer below 2^24: what = 1 of fc0 must equal the fp64 statement (masked by
    fc0's output as read from the device) exactly - on fp16 pairs under the static bound, on bf16 triples, in every tile form.
    320 -> 256 is the 64-unit backward tile by dispatch."""
    K, N = shape
    ld, in_shape = below_fc(K, N, ops)
    rs = np.random.RandomState(50 + K + N)
    W = rs.randint(-15, 16, size=(N, K)).astype(np.float32)
    b = rs.randint(-15, 16, size=N).astype(np.float32)
    Wh, bh = _small_head(N, 51 + N)
    pars = _fc_pars(ld, in_shape, 52, fct=(W, b), head=(Wh, bh))
    pars['fc0'][0] = pars['fc0'][0] * np.float32(8.)      # activations of a few units: fc_t's integer weights do not drown its bias
    M = 129
    t = _dev(sess, np.random.RandomState(53).randn(M, 64))
    counts = {}
    for route in ('default', 'no_fc_f16', 'square', 'bn64', 'no_fcgemm'):
        g = _assert_regime(sess, N, K, M, route, (True, N // 32))
        if route == 'default':
            assert g[1] == (128 if K % 128 == 0 else 64)
        m = _make(sess, ld, in_shape, pars, M, route)
        counts[route] = _f16_launches(sess, lambda: m.fisher_device(t, M, None, 1e-3, want=('p1', 'g0', 'g1')))
        act = _copy(sess, m, 0, 0, M, (M, K))
        y = _copy(sess, m, 1, 0, M, (M, N))
        dy = _copy(sess, m, 1, 1, M, (M, N))
        dlow = _copy(sess, m, 0, 1, M, (M, K))
        wd = _copy(sess, m, 1, 10, 1, (4,), np.int32) if (SHAPES[shape][0] and route != 'no_fcgemm') else None
        m.close()
        d = (Wh[0] - Wh[1]).astype(np.float64)
        want_dy = np.tile(d, (M, 1)) * ((y > 0) if 'A' in ops else 1.)
        _assert_equal(dy, want_dy, '%dto%d %s, route %s: the cotangent at fc_t' % (K, N, ops, route))
        assert 0.2 < (act > 0).mean() < 0.8 and np.count_nonzero(dy) > dy.size // 8
        if route == 'default':      # the conditions of exactness for what the device read (the masks are its own)
            R.assert_exact(dy, W.T.copy(), None, 'pairs', a_exp=R.bound_exp(np.abs(d).max() * (1 + 1e-6)))
            R.assert_exact(dy, W.T.copy(), None, 'triples')
        _assert_equal(dlow, R.din64(dy, W, act), '%dto%d %s, route %s: the cotangent of fc0' % (K, N, ops, route))
        # the static bounds: the head's max |W0 - W1| covers the cotangent at fc_t; times fc_t's column L1 norm (what = 10) the one below
        col_l1 = np.abs(W).sum(axis=0).max()
        assert np.abs(dy).max() <= np.abs(d).max() and np.abs(R.din64(dy, W)).max() <= col_l1 * np.abs(d).max()
        if wd is not None:
            l1 = float(wd[2:].view(np.float64)[0])
            assert col_l1 <= l1 <= col_l1 * (1 + 1e-5), (l1, col_l1)
            assert np.abs(R.din64(dy, W)).max() <= l1 * np.abs(dy).max()
            assert wd[0] == R.matrix_exp(W) and (route == 'no_fc_f16' or wd[1] == R.matrix_exp(W)), (route, wd, R.matrix_exp(W))
    print('FCGEMM_REGIME | %dto%d-%s | igemm_f16x2 launches of a Fisher pass per route: %r' % (K, N, ops, counts))
    assert counts['default'] == counts['no_fc_f16'] + 1 and counts['square'] == counts['bn64'] == counts['default']


# ------------------------------------------------------------------------------------------ 6. whole models
NW = 16
_WHOLE = {}


def whole(c):
    """Model, chosen patches, labels, a vector and both oracles' gradients for c classes: computed once, shared, never modified."""
    if c in _WHOLE:
        return _WHOLE[c]
    import torch
    ld = OrderedDict([('conv', ['conv', [16, [3, 3]], 'MA']), ('pool', ['pool', [2, 2]]), ('fc1', ['fc', [320], 'MA']), ('fc2', ['fc', [256], 'MA']),
                      ('head', ['fc', [c]])])
    in_shape = (8, 8, 1)
    seed = 600 + c
    pars = netspec.he_init(ld, in_shape, seed=seed, bias_std=0.05)
    assert pars['fc1'][0].shape == (320, 256) and pars['fc2'][0].shape == (256, 320)
    om64 = OracleModel(ld, in_shape, pars, dtype=torch.float64)
    om32 = OracleModel(ld, in_shape, pars)
    x, chosen = convt_ref.first_stable_patches(om64, in_shape, seed + 1000, NW, 4 * NW, fragile_units)
    assert len(chosen) == NW, 'too few patches without a fragile decision: pick another seed'
    print('c = %d: patches %r of stream %d, smallest key %.3e' % (c, chosen, seed + 1000, min(smallest_key(om64, x[[i]]) for i in range(NW))))
    rs = np.random.RandomState(seed + 2000)
    labels = rs.randint(0, 2, size=NW).astype(np.int32)
    names = list(pars.keys())
    v = [rs.randn(*np.asarray(a).shape).astype(np.float32) for nme in names for a in pars[nme]]
    g64 = [[[np.asarray(a, np.float64) for a in om64.grad_log_post(j, x[[i]])] for j in range(c)] for i in range(NW)]
    g32 = [[[np.asarray(a) for a in om32.grad_log_post(j, x[[i]])] for j in range(c)] for i in range(NW)]
    d = dict(name='c%d' % c, seed=seed, ld=ld, sk=(), in_shape=in_shape, n=NW, pars=pars, x=x, labels=labels, v=v, names=names, om64=om64, om32=om32,
             g64=g64, g32=g32, p64=om64.forward(x)['posteriors'].astype(np.float64), arrays=[nme + s for nme in names for s in ('/W', '/b')])
    _WHOLE[c] = d
    return d


def test_whole_model_no_fragile_decision():
    """On the CPU: the chosen patches are the first 16 of the stream without a fragile ReLU or pool decision in fp64."""
    from nnal_amd import ref64
    assert EPS == ref64.DEFAULT_EPS
    for c in (2, 5):
        d = whole(c)
        assert all(fragile_units(d['om64'], d['x'][[i]]) == 0 for i in range(NW))


def test_whole_model_param_grads_vs_fp64(sess):
    """tests/test_gpu_grads_fp64.test_param_grads_vs_fp64 on this model (its bar, grad_bar): every W and b array, modes 0 and 1,
    rows and sum; 16 patches as one pass and as 10 + 6."""
    d = whole(2)
    g64, g32, lab = d['g64'], d['g32'], d['labels']
    rows64, rows32, sum64, sum32 = mode1_refs(d)
    t = _dev(sess, d['x'])
    bad = []
    for route, mb in (('default', NW), ('default', 10), ('no_fcgemm', NW)):
        m = _make(sess, d['ld'], d['in_shape'], d['pars'], mb, route)
        got = {'mode 0 class 0': [], 'mode 0 class 1': [], 'mode 1 rows': []}
        total = np.zeros(m.num_params)
        for a, e in _passes(NW, mb):
            for cls in (0, 1):
                g, post, _ = m.param_grads_device(t[a:e], e - a, 0, cls=cls, want_post=True)
                got['mode 0 class %d' % cls] += [m.unflatten(r) for r in g.cpu().numpy()]
                assert np.abs(post.cpu().numpy().astype(np.float64) - d['p64'][:, a:e]).max() <= 2e-6
            g = m.param_grads_device(t[a:e], e - a, 1, labels=lab[a:e], loss_scale=1. / NW)[0]
            got['mode 1 rows'] += [m.unflatten(r) for r in g.cpu().numpy()]
            total += m.param_grads_device(t[a:e], e - a, 1, labels=lab[a:e], loss_scale=1. / NW, per_sample=False)[0].cpu().numpy().astype(np.float64)
        variants = [('mode 0 class %d' % j, got['mode 0 class %d' % j], [g64[i][j] for i in range(NW)], [g32[i][j] for i in range(NW)]) for j in (0, 1)]
        variants.append(('mode 1 rows', got['mode 1 rows'], rows64, rows32))
        variants.append(('mode 1 sum', [m.unflatten(total.astype(np.float32))], [sum64], [sum32]))
        m.close()
        for what, gd, r64, r32 in variants:
            for k, arr in enumerate(d['arrays']):
                dv, a64, a32 = np.stack([r[k] for r in gd]), np.stack([r[k] for r in r64]), np.stack([r[k] for r in r32])
                e_dev, e_32 = np.abs(dv - a64).max(), np.abs(a32 - a64).max()
                bar = grad_bar(e_32, a64)
                print('FCGEMM_WHOLE | %s mb %d | %s | %s | e_dev %.3e | e_32 %.3e | ratio %.3f | bar %.3e' % (route, mb, what, arr, e_dev, e_32, e_dev / max(e_32, 1e-300), bar))
                if not e_dev <= bar:
                    bad.append((route, mb, what, arr, e_dev, e_32, bar))
    assert not bad, bad


def _sq(arrs):
    return np.array([np.sum(np.asarray(a, dtype=np.float64) ** 2) for a in arrs])


def test_whole_model_other_entry_points_vs_fp64(sess):
    """alq_forward, alq_grad_sqnorms, alq_diag_fisher and alq_hess_vecp under the bars tests/test_gpu_grads_fp64.py holds NET-C to:
    posteriors 2e-6; 1e-4 r + 1e-12 row total; 2e-3 ref + 1e-6 max ref; test_gpu_hvp.bars, and the product also under
    the fp64 bar hvp_cases.bars64."""
    d = whole(2)
    g64, lab = d['g64'], d['labels']
    p1 = d['p64'][1]
    m = _make(sess, d['ld'], d['in_shape'], d['pars'], NW)
    t = _dev(sess, d['x'])
    post = m.forward_device(t, NW)[0].cpu().numpy()
    print('forward: max |post - p64| %.3e' % np.abs(post - d['p64']).max())
    assert np.abs(post - d['p64']).max() <= 2e-6
    ref = {j: np.stack([_sq(g64[i][j]) for i in range(NW)]) for j in (0, 1)}
    for cls in (0, 1, -1):
        got = m.grad_sqnorms_device(t, NW, cls=cls).cpu().numpy()
        r = ref[cls] if cls >= 0 else ref[0] / (p1[:, None] ** 2)
        err = np.abs(got - r)
        print('sqnorms class %d: max err / r %.3e (bar 1e-4)' % (cls, np.max(err / (r + 1e-300))))
        assert np.all(err <= 1e-4 * r + 1e-12 * r.sum(axis=1, keepdims=True)), cls
    dref = [sum(g64[i][lab[i]][k] ** 2 for i in range(NW)) / NW for k in range(len(d['arrays']))]
    for arr, a, r in zip(d['arrays'], m.diagonal_fisher(d['x'], lab), dref):
        assert a.shape == r.shape and a.dtype == np.float64, arr
        err = np.abs(a - r)
        print('diag fisher %s: max err / max ref = %.3e' % (arr, err.max() / r.max()))
        assert np.all(err <= 2e-3 * r + 1e-6 * r.max()), arr
    hv64, hv32 = (oracle_hv(om, d['x'], lab, d['v'], d['names'], 1. / NW) for om in (d['om64'], d['om32']))
    hv = m.hess_vecp(d['x'], lab, d['v'])
    # the product is evaluated in fp64: also under the fp64 bar of tests/hvp_cases.py, on patches with its decision margin
    # (tests/test_hvp_cases_host.py proves the bar's three conditions for this model)
    tight = hvp_cases.whole_tight(d)
    assert tight['bad'] == [], tight['bad']
    hv_tight = hv if tight['chosen'] is None else m.hess_vecp(tight['x'], lab, d['v'])
    m.close()
    for arr, a, a64, a32, b in zip(d['arrays'], hv, hv64, hv32, bars(hv64, hv32)):
        e = np.abs(a - a64).max()
        print('Hv %s: e_dev %.3e  e_32 %.3e  bar %.3e' % (arr, e, np.abs(a32 - a64).max(), b))
        assert a.dtype == np.float64 and a.shape == a64.shape and e <= b, (arr, e, b)
    hvp_cases.hold64('Hv (patches %r)' % (tight['chosen'] or 'of the other checks'), hv_tight, tight['y'], d['arrays'])


def test_whole_model_fisher_pass_vs_fp64(sess):
    """p1, g0, g1 and A of the Fisher pass against factored_ref in fp64, the bars of test_gpu_parity.test_netc_other_shapes_vs_fp64,
    on every sample and every route."""
    d = whole(2)
    p64, S64, sizes = factored_ref.factored_unit_scores(d['om64'], d['x'].astype(np.float64))
    g64, h64, A64 = factored_ref.fisher_from_unit(p64[1], S64, sizes, 1e-3)
    t = _dev(sess, d['x'])
    for route, (_, knob, _, _, _, _) in ROUTES.items():
        m = _make(sess, d['ld'], d['in_shape'], d['pars'], 10, route)
        with _knob(sess, knob):
            rs = [m.fisher_device(t[a:e], e - a, None, 1e-3, want=('p1', 'g0', 'g1', 'A')) for a, e in _passes(NW, 10)]
            r = {k: np.concatenate([q[k].cpu().numpy() for q in rs]) for k in ('p1', 'g0', 'g1', 'A')}
        m.close()
        e_p = np.abs(r['p1'] - p64[1]).max()
        print('%s | Fisher pass: max |p1 - p64| %.3e' % (route, e_p))
        assert e_p <= 5e-6, (route, e_p)
        for key, ref in (('g0', g64), ('g1', h64)):
            scale = np.abs(ref).max(axis=0, keepdims=True)
            err = np.abs(r[key] - ref)
            print('%s | %s: max err / per-layer max %.3e (bar 5e-4)' % (route, key, np.max(err / (scale + 1e-300))))
            assert (err <= 5e-4 * scale + 1e-9).all(), (route, key, err.max())
        np.testing.assert_allclose(r['A'], A64, rtol=2e-3, atol=1e-3 * np.abs(A64 - 1e-3 * np.eye(A64.shape[1])).max())


def test_whole_model_class_layer_sums_vs_fp64(sess):
    """alq_class_layer_sums on the five-class model: every class of every sample against alpath.shrink_gradient of the fp64
    gradients, the bar of test_gpu_lsum: per layer e(fused) <= 2 e(rows) + 6e-8 mean |entry|."""
    c = 5
    d = whole(c)
    g64 = d['g64']
    m = _make(sess, d['ld'], d['in_shape'], d['pars'], NW)
    L = m.L
    t = _dev(sess, d['x'])
    s64 = np.array([[alpath.shrink_gradient(g64[i][j]) for j in range(c)] for i in range(NW)])
    mean_abs = np.array([[[(np.abs(gr[2 * q]).sum() + np.abs(gr[2 * q + 1]).sum()) / (gr[2 * q].size + gr[2 * q + 1].size)
                           for q in range(L)] for gr in g64[i]] for i in range(NW)]).mean(axis=(0, 1))
    g_rows = m.shrunk_class_gradients(d['x'])[0].cpu().numpy()
    g_fused = m.class_layer_sums_device(t, NW, np.tile(np.arange(c), (NW, 1))).cpu().numpy()
    m.close()
    assert g_fused.shape == g_rows.shape == s64.shape == (NW, c, L)
    e_fused, e_rows = np.abs(g_fused - s64).max(axis=(0, 1)), np.abs(g_rows - s64).max(axis=(0, 1))
    for q in range(L):
        print('layer sums %s: e(fused) %.3e  e(rows) %.3e  floor %.3e' % (d['names'][q], e_fused[q], e_rows[q], 6e-8 * mean_abs[q]))
    assert np.all(e_fused <= 2 * e_rows + 6e-8 * mean_abs), (e_fused, e_rows)


def test_device_weight_packing_same_bits(sess):
    """alq_model_set_weights_device against alq_model_set_weights at these widths (320: the 64-unit tiles of wpack.hip's layout):
    the same bits out of the forward pass - and of the Fisher pass and the parameter gradients."""
    d = whole(2)
    t = _dev(sess, d['x'])
    outs = []
    for dw in (False, True):
        m = _make(sess, d['ld'], d['in_shape'], d['pars'], NW, extra_env={} if dw else {'ALQ_HOST_REPACK': '1'}, device_weights=dw)
        assert m._host_repack == (not dw)
        if dw:
            assert m._dev_pack == [False, True, True, False]
        o = OrderedDict()
        o['post'] = m.forward_device(t, NW)[0].cpu().numpy()
        o['fc1'] = _copy(sess, m, 2, 0, NW, (NW, 320))
        o['fc2'] = _copy(sess, m, 3, 0, NW, (NW, 256))
        r = m.fisher_device(t, NW, None, 1e-3, want=('p1', 'g0', 'g1', 'A'))
        for k in ('p1', 'g0', 'g1', 'A'):
            o[k] = r[k].cpu().numpy()
        o['grads'] = m.param_grads_device(t, NW, 1, labels=d['labels'], loss_scale=1. / NW)[0].cpu().numpy()
        m.close()
        outs.append(o)
    for k in outs[0]:
        assert np.isfinite(outs[0][k]).all() and np.abs(outs[0][k]).max() > 0, k
        np.testing.assert_array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8), err_msg=k)
