"""NET-C's fused layer launches at 32^3, each alone against tests/netc_ref.py (GPU box).

The Fisher pass of the benchmark's NET-C spends its time in launches that exist at this one geometry only.  The rest of the suite
holds them to the two-slot engine (2e-6 of a tensor's maximum), to each other (bit identity of the sweep forms) and to fp64 through
whole-model scores whose bar hides a wrong voxel.  Here every launch's stored inputs are read from the device and taken as given,
and every stored output is held to an exact or fp64 statement of the launch's own operation.

The table (netc_ref.LAUNCHES, read from csrc/passes.hip; layers 0 enc1, 1 pool1, 2 enc2, 3 pool2, 4 bott, 5 up1, 6 dec1, 7 up2,
8 dec2, 9 fc).  Forward: direct.hip runs layers 0 and 1 (its own file; input only here: out, sign field and arg-max bytes);
    f3d_fwd       f3d.hip     pool1 out -> enc2 out, sign field, channel sums; pool2 out, arg-max bytes, channel sums
    bott_fwd      igemm4.hip  pool2 out -> bott out, sign field, channel sums (bf16 triples; no maxima are asked of it: no launch
                              above it takes a measured scale)
    t3d_fwd_up1   t3d.hip     bott out -> up1 out, channel sums (bf16 triples)
    d3d_fwd       d3d.hip     [enc2 | up1] under the derived bounds of both -> dec1 out, sign field, channel sums
    t3d_fwd_up2   t3d.hip     dec1 out -> up2 out, channel sums, the measured per-patch maxima (bf16 triples)
c3d_fwd (layer 8) writes the head's sign bytes and partials only: tests/test_gpu_fc_small.py; input only here.  Backward:
    c3d_bwd7      c3d.hip     head sign bytes x wv, enc1's sign field -> up2's cotangent (channels 8 .. 15) and its sums; channels
                              0 .. 7 are masked and summed into enc1's PARTIAL dsum, which is not in memory after the pass
    t3d_bwd_up2   t3d.hip     up2's cotangent, dec1's sign field -> dec1's masked cotangent, dsum
    d3d_bwd       d3d.hip     dec1's cotangent -> enc2's half of the concat cotangent (unmasked, partial: pool2's share is not in
                              it yet), up1's cotangent, up1's dsum
    t3d8_bwd_up1  t3d8b.hip   up1's cotangent, bott's sign field -> bott's masked cotangent, dsum
    bott_bwd      igemm4.hip  bott's cotangent -> pool2's cotangent
    e3d_bwd       e3d.hip     enc2's partial cotangent, pool2's cotangent, both arg-max fields, the sign fields of enc2 and pool1
                              (and, for the reference of the completed sum, the head's sign bytes and enc1's sign field) ->
                              enc2's dsum, enc1's completed dsum; nothing else
alq_model_debug_copy returns whatever a buffer holds, so every test first asserts from alq_model_engine_info that the launches ran
(netc_ref.ENGINE_INFO: 7, 8, 9, 10, 11, 12, 13, 17 and 19 = 2); the c3d family is read on the fresh model (run index 1 / 2 = 0),
then after the pass (1), the plan indices 13 / 19 / 20 separately, and the overflow count 5 stays 0.

Check A, exact.  netc_ref.integer_model: x in {0, 1} (patch 0 all zero, patch 1 all one), weights in {-1, 0, 1} thinned per layer
(bott 3 / 256, up1 4 / 256, dec1 6 / 256 - enc2's static cotangent bound, 3.3e7 at 1 / 16, is then 3.65e6 head units < 2^22), a head
in [-2, 2] 2^-6.  Every launch meets the three exactness conditions (tests/test_netc_ref_host.py asserts them on the CPU; here
again before the device is asked), e3d.hip included: NOT_EXACT is empty.  Every tensor of the table must EQUAL the fp64 composition
from x, on every patch: activations, sign and arg-max bytes, channel sums, per-patch maxima, cotangents, dsum, and S of the layers
the table covers.

Check B, float.  he_init weights with bias_std = 0.05; alq_synth_patches, then patch 1 all zero, patch 2 times 2^20, patch 3 times
2^-20, patch 4 non-zero on the one-voxel shell of the volume only.  Runs: N = 9 under max_batch = 9 (SW_XCD_DEAL: one XCD owns two
patches), N = 1 (seven idle workgroups), N = 5 under max_batch = 4 (two passes, the second of one patch), and N = 9 with the grids of
e3d.hip and c3d_bwd7 capped at 2 workgroups (alq_debug_set(9 / 10, 2), restored in a finally: streams cross patch boundaries).  Every
float output is held to the DERIVED bar of netc_ref's docstring - u_x at the scale the launch used (what = 15 / 16 / 18), u_w at
f16_pair_exp of the weights, the dropped lo x lo product, 2^-24 (M - 1) sum |x w|, one rounding - nothing in it is measured or
tuned; channel sums by test_gpu_pool._assert_sums against the launch's own stored tensor (e3d.hip's two sums, whose terms are not
stored: netc_ref.e3d_extra); sign and arg-max bytes, pooled values and per-patch maxima exactly against the launch's own stored
tensor.  NETC_FIG prints err, bar, err / bar and the fp32 yardstick's error e_32 per launch and output before anything is asserted.

Batch invariance: all scales are per patch or static, so the nine patches one at a time give the same bytes in every tensor.

FORMS_UNREACHABLE names what no test here reaches.

Worst err / bar of check B per launch, MI355X, 2026-10-21 (NETC_WORST; DESIGN.md carries the same table): f3d_fwd 0.056, bott_fwd 0.054,
t3d_fwd_up1 0.021, d3d_fwd 0.018, t3d_fwd_up2 0.042, c3d_bwd7 0.068, t3d_bwd_up2 0.038, d3d_bwd 0.029, t3d8_bwd_up1 0.017,
bott_bwd 0.014, e3d_bwd 0.135 (enc2's dsum: sixteen fp32 additions; enc1's dsum 0.030).  No launch missed a check: no kernel changed.

Runtime of the file on an MI355X, 2026-10-21: 23.2 s for its 51 tests (RUNTIME below; tests/test_gpu_convt.py: 6.7 s in the same
session).  Nearly all of it is the fp64 references on the CPU - six contractions per launch and run - the slowest call 3.8 s (e3d_bwd on
nine patches: the bars of two contractions at 32^3).
"""
import ctypes as C
import time
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import netc_ref as R  # noqa: E402
from tests import pool_ref, side_ref  # noqa: E402
from tests.netc_ref import BOTT, DEC1, ENC1, ENC2, FC, POOL1, POOL2, UP1, UP2  # noqa: E402
from tests.test_gpu_convt import _copy, _dev, _make, _passes  # noqa: E402
from tests.test_gpu_pool import _assert_same_bits, _assert_sums  # noqa: E402

_T0 = time.time()
# launch -> why no integer model makes it exact (such a launch is held to check B alone; at most e3d_bwd may stand here)
NOT_EXACT = OrderedDict()
# what no test of this file reaches, and why
FORMS_UNREACHABLE = OrderedDict([
    ('the forward-only (light) forms of f3d.hip, d3d.hip and c3d.hip',
     'they store no sign field and no channel sums, and alq_model_debug_copy reads the buffers of a Fisher pass (what = 11 .. 14 are '
     'refused after a forward-only call); tests/test_gpu_parity.py compares their posteriors'),
    ('ALQ_E3D_ROWS, ALQ_C3D_BWD_ROWS, ALQ_C3D_BWD_WAVES',
     'the other arms of e3d.hip and c3d.hip are held bit for bit to the default arms tested here (tests/test_gpu_e3d_plane_sweep.py, '
     'tests/test_gpu_parity.py)'),
    ('multi-patch streams of f3d.hip, d3d.hip, t3d.hip and t3d8b.hip',
     'their grids have no cap: a workgroup gets a second patch only beyond one patch per workgroup slot; '
     'test_shipped_batch_2047_is_bit_identical_to_small_batches covers those'),
    ('a lost THIRD piece of a bf16 triple (bott_fwd, t3d_fwd)',
     '2^-17 per element: inside the accumulation term of any derived bar (tests/test_netc_ref_host.py); check A would need integers '
     'above 2^16, which the accumulator bound of the layers above does not leave room for'),
])
DIMS = {l: (R.SIZE[l],) * 3 + (R.CH[l],) for l in R.SIZE}
WORST = {}      # launch -> worst err / bar of this session (printed by test_zz_runtime_and_worst)
# The file's 51 tests on an MI355X, 2026-10-21: 23.2 s (pytest's own figure); tests/test_gpu_convt.py in the same session: 6.7 s
RUNTIME = 23.2


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _info(sess, m, k):
    return int(sess.lib.alq_model_engine_info(m._m, k))


def _assert_fresh(sess, m):
    assert _info(sess, m, 1) == 0 and _info(sess, m, 2) == 0 and _info(sess, m, 5) == 0, 'a fresh model reports a c3d launch'


def _assert_ran(sess, m, n, grid=None):
    """Every launch of the table ran in the last Fisher pass."""
    got = OrderedDict((k, _info(sess, m, k)) for k in R.ENGINE_INFO)
    assert got == R.ENGINE_INFO, got
    assert _info(sess, m, 6) == 1, 'no launch on derived bounds: not the default route'
    assert _info(sess, m, 1) == 1 and _info(sess, m, 2) == 1, 'c3d.hip did not run'      # the run indices ...
    assert _info(sess, m, 13) == 7 and _info(sess, m, 19) == 2      # ... and the plan indices, separately
    assert _info(sess, m, 20) == (grid if grid else min(n, 256)), _info(sess, m, 20)
    assert _info(sess, m, 5) == 0, 'the flip lists overflowed'
    assert _info(sess, m, 16) > 0, 'direct.hip did not run the first conv + pool'


def _bytes(a, n):
    return np.ascontiguousarray(a).view(np.uint8).reshape(n, -1)


def _unpack(b, shape):
    assert (b < 16).all(), 'a sign byte has a bit above its nibble'
    return (((b[:, :, None] >> np.arange(4, dtype=np.uint8)) & 1) > 0).reshape(shape)


def _read(sess, m, n):
    """Every tensor of the table as the last Fisher pass left it, and the scales S it ran under."""
    T = OrderedDict()
    for layer in range(8):
        T[(layer, 'out')] = _copy(sess, m, layer, 0, n, (n,) + DIMS[layer])
    for layer in (UP2, DEC1, ENC2, UP1, BOTT, POOL2):
        T[(layer, 'dout')] = _copy(sess, m, layer, 1, n, (n,) + DIMS[layer])
    for layer in (ENC2, POOL2, BOTT, UP1, DEC1, UP2):
        T[(layer, 'osum')] = _copy(sess, m, layer, 11, n, (n,) + DIMS[layer][:3])
    for layer in (ENC1, ENC2, BOTT, UP1, DEC1, UP2):
        T[(layer, 'dsum')] = _copy(sess, m, layer, 3, n, (n,) + DIMS[layer][:3])
    for layer in (ENC1, POOL1, ENC2, BOTT, DEC1):      # (the split concat: every tensor is dense, cs = C - the element count says so)
        vox, Cn = R.SIZE[layer] ** 3, R.CH[layer]
        T[(layer, 'sign')] = _unpack(_bytes(_copy(sess, m, layer, 12, n, (n, vox * Cn // 16)), n), (n,) + DIMS[layer])
    for layer in (POOL1, POOL2):
        vox, Cn = R.SIZE[layer] ** 3, R.CH[layer]
        T[(layer, 'argmax')] = _bytes(_copy(sess, m, layer, 13, n, (n, vox * Cn // 4)), n).reshape((n,) + DIMS[layer])
    T[(FC, 'headsign')] = _unpack(_bytes(_copy(sess, m, FC, 14, n, (n, 32 ** 3 * 8 // 16)), n), (n, 32, 32, 32, 8))
    for layer in (ENC1, UP2):
        T[(layer, 'amax')] = _copy(sess, m, layer, 16, n, (n,))
    T['S'] = _copy(sess, m, 0, 4, n, (n, m.L))
    S = dict(amax0=T[(ENC1, 'amax')].astype(np.float64), derived=_copy(sess, m, 0, 15, n, (10, n)).astype(np.float64),
             static=_copy(sess, m, 0, 18, n, (10,)).astype(np.float64))
    return T, S


def _fisher(sess, m, t, n, grid=None):
    m.fisher_device(t, n, None, 1e-3, want=('p1',))
    _assert_ran(sess, m, n, grid)
    return _read(sess, m, n)


def _cat_passes(parts):
    return OrderedDict((k, np.concatenate([p[k] for p in parts])) for k in parts[0])


# ------------------------------------------------------------------------------------------ A. exact
@pytest.fixture(scope='module')
def exact(sess):
    x, P, want, _ = R.integer_model()
    ld, sk = R.net()
    n = len(x)
    m = _make(sess, ld, R.IN_SHAPE, sk, P, n)
    try:
        _assert_fresh(sess, m)
        T, S = _fisher(sess, m, _dev(sess, x), n)
    finally:
        m.close()
    return x, P, want, T, S


def _equal(tag, key, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, key, got.shape, want.shape)
    bad = np.argwhere(got.astype(np.float64) != want.astype(np.float64))
    print('NETC_EXACT | %s | %s | %d of %d values differ' % (tag, key, len(bad), got.size))
    assert bad.size == 0, '%s, %r: %d of %d values differ, first at %r: %r != %r' % (tag, key, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                                   want[tuple(bad[0])])


def test_exact_inputs_scales_and_S(exact):
    """What direct.hip and c3d_fwd hand to the table, the bounds the launches took their scales from, and S of the layers covered."""
    x, P, want, T, S = exact
    for k in ((ENC1, 'out'), (ENC1, 'sign'), (POOL1, 'out'), (POOL1, 'argmax'), (POOL1, 'sign'), (FC, 'headsign')):
        _equal('inputs', k, T[k], want[k])
    _equal('inputs', (ENC1, 'amax'), T[(ENC1, 'amax')], np.abs(want[(ENC1, 'out')]).reshape(len(x), -1).max(1))
    static, derived = R.bwd_bounds(P), R.derived_bounds(P, S['amax0'])
    for layer in range(1, 10):
        assert abs(S['static'][layer] / static[layer] - 1) <= 2.0 ** -20, (layer, S['static'][layer], static[layer])
    live = derived > 0
    assert np.all(np.abs(S['derived'][live] / derived[live] - 1) <= 2.0 ** -20) and not S['derived'][~live].any()
    ld, sk = R.net()
    geoms = side_ref.layers_of(ld, sk, R.IN_SHAPE)
    xs = x.reshape(len(x), 32, 32, 32).astype(np.float64)
    for layer in (ENC1, ENC2, BOTT, UP1, DEC1, UP2):
        g = next(g for g in geoms if g['layer'] == layer)
        asum = xs if layer == 0 else want[(g['src'], 'osum')] if (g['src'], 'osum') in want else want[(g['src'], 'out')].sum(-1)
        S64 = side_ref.layer_S64(g, want[(layer, 'dsum')], asum, None if g['src2'] is None else want[(g['src2'], 'osum')])
        assert np.abs(S64).max() < 2.0 ** 24 * R.HEAD_SCALE
        _equal('S', R.NAMES[layer], T['S'][:, g['pidx']], S64)


@pytest.mark.parametrize('l', [l for l in R.LAUNCHES if l.name not in NOT_EXACT], ids=[n for n in R.BY_NAME if n not in NOT_EXACT])
def test_launch_equals_the_integers_of_its_definition(exact, l):
    x, P, want, T, S = exact
    ints, sb, acc = R.exactness(l, want, P)
    assert ints and sb < 1. and acc < 1., (l.name, ints, sb, acc)
    for k in l.outputs:
        _equal(l.name, k, T[k], want[k])
        assert np.asarray(want[k])[1:].any(), (l.name, k)
        assert not np.asarray(T[k])[0].any() or k[1] == 'argmax', (l.name, k, 'the all-zero patch')


def test_tables():
    assert set(NOT_EXACT) <= {'e3d_bwd'} and len(FORMS_UNREACHABLE) == 4
    read = {(ENC1, 'out'), (ENC1, 'sign'), (POOL1, 'out'), (POOL1, 'argmax'), (POOL1, 'sign'), (FC, 'headsign'), (ENC1, 'amax')}
    for l in R.LAUNCHES:
        read |= set(l.outputs)
    assert len(read) == 7 + sum(len(l.outputs) for l in R.LAUNCHES)


# ------------------------------------------------------------------------------------------ B. float
N9 = 9
RUNS = OrderedDict([('n9', (9, 9, None)), ('n1', (1, 1, None)), ('n5_mb4', (5, 4, None)), ('n9_cap2', (9, 9, 2))])      # n, max_batch, grid cap
_FLOAT = {}


def _patches(sess, n):
    """alq_synth_patches; 1: all zero, 2: times 2^20, 3: times 2^-20, 4: non-zero on the one-voxel shell of the volume only."""
    from nnal_amd._lib import check
    torch = sess.torch
    x = torch.empty((n, 32 ** 3), dtype=torch.float32, device=sess.device)
    check(sess.lib.alq_synth_patches(sess.ctx, 1004, 0, n, 32 ** 3, C.c_void_p(x.data_ptr())))
    torch.cuda.synchronize()
    if n >= 5:
        x[1] = 0
        x[2] *= 2.0 ** 20
        x[3] *= 2.0 ** -20
        shell = torch.ones((32, 32, 32), dtype=torch.float32, device=sess.device)
        shell[1:-1, 1:-1, 1:-1] = 0
        x[4] *= shell.reshape(-1)
    return x


def _float_run(sess, run):
    """(T, S, P, models' patches) of a run of RUNS, computed once."""
    if run in _FLOAT:
        return _FLOAT[run]
    from tests.test_gpu_parity import _netc32_models
    n, mb, cap = RUNS[run]
    ld, sk, in_shape, P, (m,) = _netc32_models(sess, [{}], mb, seed=14, bias_std=0.05)
    assert in_shape == R.IN_SHAPE and list(ld) == R.NAMES
    x = _patches(sess, N9)[:n] if n > 1 else _patches(sess, N9)[5:6]
    try:
        _assert_fresh(sess, m)
        if cap:
            assert sess.lib.alq_debug_set(9, cap) == 0 and sess.lib.alq_debug_set(10, cap) == 0
        parts = [_fisher(sess, m, x[a:e], e - a, cap) for a, e in _passes(n, mb)]
        alone = None
        if run == 'n9':      # the same patches one at a time, on the same model
            alone = _cat_passes([_fisher(sess, m, x[i:i + 1], 1)[0] for i in range(n)])
    finally:
        if cap:
            sess.lib.alq_debug_set(9, 0)
            sess.lib.alq_debug_set(10, 0)
        m.close()
    T = _cat_passes([p[0] for p in parts])
    S = dict(amax0=np.concatenate([p[1]['amax0'] for p in parts]), derived=np.concatenate([p[1]['derived'] for p in parts], axis=1), static=parts[0][1]['static'])
    for p in parts[1:]:
        assert np.array_equal(p[1]['static'], S['static'])
    _FLOAT[run] = (T, S, P, alone)
    return _FLOAT[run]


def _figure(bad, run, l, key, dev, ref, bar, e32):
    """Prints err, bar, err / bar at the worst element and the error e_32 of the same operation in fp32 torch beside them, then records a miss."""
    err = np.abs(np.asarray(dev, np.float64) - ref)
    ratio = err / np.maximum(bar, 1e-300) * (err > 0)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print('NETC_FIG | %s | %s | %s | err %.3e | bar %.3e | err / bar %.4f | e_32 %.3e (there; its worst e_32 / bar %.4f)'
          % (run, l.name, key, err[i], bar[i], ratio[i], e32[i], np.max(e32 / np.maximum(bar, 1e-300) * (e32 > 0))))
    WORST[l.name] = max(WORST.get(l.name, 0.), float(ratio[i]))
    if not np.all(err <= bar):
        bad.append((run, l.name, key, float(err[i]), float(bar[i]), tuple(int(v) for v in i)))


def _check_float(run, l, T, S, P):
    """Every stored output of launch l in T against the reference of its stored inputs in T."""
    bad = []
    n = len(T[(ENC1, 'out')])
    ref = R.reference(l, T, P)
    y = R.lin(l.kind, l.core(T, P), R.weights(l, P))
    y32 = R.lin(l.kind, l.core(T, P), R.weights(l, P), dtype=np.float32)
    ref32 = l.finish(y32.astype(np.float64), T, P, None)
    by = R.bars(l, T, P, S, y=y)
    assert np.all(np.isfinite(by)) and by.min() >= 0
    ob = R.output_bars(l, by, T)
    if l.name == 'e3d_bwd':
        ob[(ENC2, 'dsum')], ob[(ENC1, 'dsum')] = R.e3d_extra(T, P, S)
    for key in l.outputs:
        layer, what = key
        dev, tag = T[key], '%s | %s | %r' % (run, l.name, key)
        if key in ob:
            _figure(bad, run, l, key, dev, ref[key], ob[key], np.abs(np.asarray(ref32[key], np.float64) - ref[key]))
            assert np.count_nonzero(dev) > 0, tag
        elif what == 'sign':      # exactly act > 0 of the launch's own stored tensor
            assert np.array_equal(dev, T[(layer, 'out')] > 0), (tag, int(np.count_nonzero(dev != (T[(layer, 'out')] > 0))))
        elif what == 'argmax':      # the first maximum in window order of the launch's own enc2 output; the pooled value is that maximum
            pooled, arg = pool_ref.pool_fwd(T[(ENC2, 'out')], R.W2)
            assert np.array_equal(dev, arg), (tag, int(np.count_nonzero(dev != arg)))
            _assert_same_bits(T[(POOL2, 'out')], pooled, tag + ' pooled values')
        elif what in ('osum', 'dsum'):
            _assert_sums(dev, T[(layer, 'out' if what == 'osum' else 'dout')], 'NETC_SUM | ' + tag)
        elif what == 'amax':
            own = np.abs(T[(layer, 'out')]).reshape(n, -1).max(1)
            assert np.array_equal(dev.view(np.uint32), own.view(np.uint32)), (tag, dev, own)
        else:
            assert key == (POOL2, 'out'), key      # (held with the arg-max bytes)
    assert not bad, bad


def _launches_of(run):
    return [l for l in R.LAUNCHES if RUNS[run][2] is None or l.name in ('e3d_bwd', 'c3d_bwd7')]


@pytest.mark.parametrize('run,l', [(r, l) for r in RUNS for l in _launches_of(r)], ids=['%s-%s' % (r, l.name) for r in RUNS for l in _launches_of(r)])
def test_launch_within_the_derived_bar_of_fp64(sess, run, l):
    T, S, P, _ = _float_run(sess, run)
    if l is R.LAUNCHES[0]:      # the scales the launches ran under are the host twins', once per run
        static = R.bwd_bounds(P)
        assert np.all(np.abs(S['static'][1:] / static[1:] - 1) <= 2.0 ** -20), (S['static'], static)
        derived = R.derived_bounds(P, S['amax0'])
        assert np.all(np.abs(S['derived'] / derived - 1) <= 2.0 ** -20)
        assert np.array_equal(S['derived'][POOL1], S['amax0'])
    _check_float(run, l, T, S, P)


def test_batch_invariance(sess):
    """The nine patches one at a time: the same bytes in every tensor of the table."""
    T, S, P, alone = _float_run(sess, 'n9')
    assert set(alone) == set(T)
    for k in T:
        a, b = np.ascontiguousarray(T[k]), np.ascontiguousarray(alone[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        same = np.array_equal(a.view(np.uint8), b.view(np.uint8))
        print('NETC_BATCH | %r | %s' % (k, 'same bytes' if same else 'DIFFERS'))
        assert same, (k, int(np.count_nonzero(a != b)))


def test_grid_cap_changes_no_byte(sess):
    """Capped at 2 workgroups, e3d.hip and c3d_bwd7 walk streams that cross patch boundaries: the same bytes as uncapped."""
    T, _, _, _ = _float_run(sess, 'n9')
    Tc, _, _, _ = _float_run(sess, 'n9_cap2')
    for k in ((UP2, 'dout'), (UP2, 'dsum'), (ENC2, 'dsum'), (ENC1, 'dsum')):
        assert np.array_equal(T[k].view(np.uint32), Tc[k].view(np.uint32)), k


def test_zz_runtime_and_worst():
    for name, r in sorted(WORST.items()):
        print('NETC_WORST | %s | worst err / bar %.4f' % (name, r))
    print('NETC_RUNTIME | %.1f s since the file was imported (with the CPU references)' % (time.time() - _T0))
