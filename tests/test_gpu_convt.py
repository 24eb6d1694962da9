"""conv_transpose beyond NET-C's 3x3x3 stride 2: every route of the layer's device code against fp64 references (GPU box).

The layer's device code is general - igemm4_build_plan's kinds 1 (backward-data), 2 (every class from one staged block, with and
without the pair form), 3 (one parity class) and 4 (classes as tiles); convt_class_desc / convt_bwd_desc in front of igemm.hip,
igemm2.hip, igemm3.hip and direct.hip; set_convt and its device twin; boxdot_convT_kernel; the conv_transpose geometry of lsum.hip;
the conv_transpose branches of wgrad_kernel and hvp.hip - and the rest of the suite runs it at k = 3, s = 2 only.  Here: the
geometries of tests/convt_ref.py (k = 2 .. 5, s = 1 .. 3, another k per dimension, the 2-D schema; every volume ragged), channel
pairs on and off the two-slot engine, both op orders, under every engine switch.

Models (tests/convt_ref.py), built through device.DeviceModel, internals read with alq_model_debug_copy:
  first-layer   conv_transpose -> conv(4, 1x1) -> fc(2): the layer reads the caller's x, so x, W and b are small integers and
                the output must EQUAL the loops of the definition in fp64 (check 1), after a forward pass and after a Fisher pass;
  below-conv    conv(Ci, 3^3, 'MA') -> conv_transpose -> conv(4, 1x1) -> fc(2): the layer's input activation and its own cotangent
                are read from the device after alq_param_grads and taken as given; its output (check 2), the cotangent of the conv
                below (check 3: (a > 0) sum_t dy[s q + t - lo] W[t]) and its rows of the parameter gradients (check 4) follow from
                them in fp64.  With 'MA' the cotangent read is already masked: it must be zero wherever the output is;
  whole models  below-conv models and two U-Net levels (the conv_transpose as a producer of a concat, k = 2 and k = 4)
                against OracleModel(dtype=float64): alq_param_grads, alq_grad_sqnorms, alq_class_layer_sums, alq_diag_fisher,
                alq_hess_vecp under the bars of tests/test_gpu_grads_fp64.py (check 5), the Fisher pass under the bars of
                test_gpu_parity.test_netc_other_shapes_vs_fp64 (check 6), and the device weight packers bit for bit (check 7).
N = 5 patches under max_batch = 4 are two passes with a ragged last group; two cases take max_batch = 8 (several patches per tile).
Patches of the below-conv and whole models: the first N of a fixed stream whose fp64 evaluation has no fragile decision at
ref64.DEFAULT_EPS (asserted, smallest key printed); no sample is left out of any check.

Tolerances of checks 2 - 5: per compared array e_dev = max |dev - ref64| and e_32 = max |ref32 - ref64|, ref32 the same operation in
fp32 torch on the same inputs; the assertion is e_dev <= 4 R e_32 + 6e-8 mean |ref64 entry| with R = R_DEV_OVER_F32 below, and never
looser than 2e-4 max |ref64| + 1e-9 (tests/test_gpu_grads_fp64.py).  Every figure is printed before it is asserted.

Refused geometries: a conv_transpose that is not the first parameterised layer needs a backward-data GEMM, one descriptor of all
prod(k) taps, and igemm_build_plan takes 28 (IG_MAXTAPS): alq_model_create refuses 4x4x4 (64) and 5x5x5 (125) below a conv with
ALQ_EUNSUPPORTED, "igemm: 64 taps unsupported".  Those models stay in every table and the refusal and its text are their check
(_refusal); as first layers the same kernels run and are held to check 1, and 4x4 / 5x5 in 2-D (16 / 25 taps) and 2x3x4 (24) run
everywhere - two taps per class with lo = 1 are therefore checked backward along y and x, never along all three dimensions at once.

Routes: the engine switches are set around model creation (they are read there and when weights are packed), knobs 4 and 5 of
alq_debug_set around the calls.  test_routes_table reads igemm4_build_plan's own lines (ALQ_G4_VERBOSE) for every case and asserts
which forms the case list reaches (FORMS_REACHED).  Forms no case can reach: none - kinds 1, 2 with and without the pair form, 3 and
4, the natural and the conflict-free LDS order and tiles of several patches are all run by some case (kind 3 runs where neither
kind 2 nor kind 4 is built: 3 classes per dimension, or ALQ_NO_CLASS_TILES); FORMS_UNREACHABLE stays empty and is asserted so.
"""
import ctypes as C
import os
import re
from collections import OrderedDict, namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import alpath, netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests import convt_ref, factored_ref, hvp_cases  # noqa: E402
from tests.convt_ref import GEOMETRIES, geometry  # noqa: E402
from tests.test_gpu_grads_fp64 import smallest_key  # noqa: E402
from tests.test_gpu_hvp import EPS, bars, fragile_units, oracle_hv  # noqa: E402

# Largest e_dev / e_32 over the 3676 figures of checks 2 - 5 (every case, route, pass and variant) whose e_dev exceeds the floor
# 6e-8 mean |ref64| (below it the floor alone carries the assertion and e_32 may be 0), measured on an MI355X on 2026-10-20: 5.092 at
# k3s1-16to4-M, patches 0..3, the layer's output on the two-slot engine (kind 4 by default, kind 3 under ALQ_NO_CLASS_TILES: the same
# figure; e_dev 5.580e-06, e_32 1.096e-06, max |ref64| 8.69: 6.4e-07 relative).  Stride 1 is the longest contraction of the table - 27
# taps x 16 channels = 432 products per output, of a non-negative activation with weights of either sign - and every engine pays for
# its length there: 2.98 under ALQ_DISABLE_V4, 4.11 (patch 4) under ALQ_DISABLE_V4 + V3 + V2, the fp32 engines.  The next cases are
# 2d_k3s2-8to40-MA (3.89, the cotangent below, 360 products) and, among the whole models, 2d_k4s2-16to4 (3.39, mix/b); the layer's
# own dW and db rows stay at or below 1.42.  NET-C's figure (tests/test_gpu_grads_fp64.py) is 3.004.  DESIGN.md has the table.
R_DEV_OVER_F32 = 5.092
R_FACTOR = 4.0
N = 5

Case = namedtuple('Case', 'tag Ci Co ops mb ig')
# on the two-slot engine: (8, 8) reaches the pair form when s[2] = 2; NT = 1 and 2.  Off it: Ci < 8, Ci % 8, Co % 4, NT > 2
IG_PAIRS = [(8, 8), (16, 4), (8, 16), (8, 32)]
OFF_PAIRS = [(4, 8), (12, 8), (8, 6), (8, 40)]


def _cases():
    out = []
    for i, tag in enumerate(GEOMETRIES):
        for ig, (Ci, Co) in ((True, IG_PAIRS[i % 4]), (False, OFF_PAIRS[i % 4])):
            for ops in ('M', 'MA'):
                out.append(Case(tag, Ci, Co, ops, 4, ig))
    # several patches per tile (PT > 1 needs the batch to hold them)
    out += [Case('k3s2_ragged', 8, 8, 'M', 8, True), Case('k4s2', 8, 16, 'MA', 8, True)]
    return out


CASES = _cases()
CASE_IDS = ['%s-%dto%d-%s-mb%d' % c[:5] for c in CASES]

# name -> (environment around model creation, alq_debug_set knob around the calls)
ROUTES = OrderedDict([
    ('default', ({}, None)),
    ('no_v4', ({'ALQ_DISABLE_V4': '1'}, None)),
    ('no_v4_v3', ({'ALQ_DISABLE_V4': '1', 'ALQ_DISABLE_V3': '1'}, None)),
    ('no_v4_v3_v2', ({'ALQ_DISABLE_V4': '1', 'ALQ_DISABLE_V3': '1', 'ALQ_DISABLE_V2': '1'}, None)),
    ('no_class_tiles', ({'ALQ_NO_CLASS_TILES': '1'}, None)),
    ('no_f16x2', ({'ALQ_NO_F16X2': '1'}, None)),
    ('knob4', ({}, 4)),
    ('knob5', ({}, 5)),
])


# ------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


class _env(object):
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
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


def _make(sess, ld, in_shape, sk, pars, mb, route='default', extra_env=None, device_weights=False, routes=None):
    """`routes`: another table of the form of ROUTES (tests/test_gpu_conv.py has its own)."""
    from nnal_amd import device
    env = dict((routes or ROUTES)[route][0])
    env.update(extra_env or {})
    with _env(env):
        m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=mb)
        assert m.max_batch == mb
        if device_weights:
            torch = sess.torch
            m.set_weights_device(OrderedDict((nme, (sess.to_device(np.ascontiguousarray(W, dtype=np.float32), torch.float32),
                                                    sess.to_device(np.ascontiguousarray(b, dtype=np.float32), torch.float32)))
                                             for nme, (W, b) in pars.items()))
        else:
            m.set_weights(pars)
    return m


def _copy(sess, m, layer, what, n, shape):
    """alq_model_debug_copy of the last pass as an array of `shape` (its size must come back)."""
    from nnal_amd._lib import check
    torch = sess.torch
    expect = int(np.prod(shape))
    e = C.c_int64()
    buf = torch.zeros((expect + 64,), dtype=torch.float32, device=sess.device)
    check(m.lib.alq_model_debug_copy(m._m, int(layer), int(what), int(n), C.c_void_p(buf.data_ptr()), C.byref(e)))
    torch.cuda.synchronize()
    assert e.value == expect, (layer, what, e.value, expect)
    return buf[:expect].cpu().numpy().reshape(shape)


def _dev(sess, x):
    return sess.to_device(np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1), sess.torch.float32)


def _passes(n, mb):
    return [(a, min(n, a + mb)) for a in range(0, n, mb)]


def _bar(e32, a64):
    a64 = np.asarray(a64)
    floor = 6e-8 * np.abs(a64).mean()
    return min(R_FACTOR * R_DEV_OVER_F32 * e32 + floor, 2e-4 * np.abs(a64).max() + 1e-9), floor


def _figure(bad, tag, what, dev, r64, r32):
    """Prints e_dev, e_32 and their ratio, then records a miss of the bar of the module docstring in `bad`."""
    dev, r64, r32 = np.asarray(dev), np.asarray(r64, np.float64), np.asarray(r32)
    assert dev.shape == r64.shape == r32.shape and dev.dtype == np.float32 and r32.dtype == np.float32, (tag, what, dev.shape, r64.shape)
    e_dev, e_32 = np.abs(dev - r64).max(), np.abs(r32 - r64).max()
    bar, floor = _bar(e_32, r64)
    print('CONVT_FIG | %s | %s | e_dev %.3e | e_32 %.3e | ratio %.3f | floor %.3e | above_floor %d | max|ref| %.3e | bar %.3e'
          % (tag, what, e_dev, e_32, e_dev / max(e_32, 1e-300), floor, e_dev > floor, np.abs(r64).max(), bar))
    if not e_dev <= bar:
        bad.append((tag, what, e_dev, e_32, bar))


def _w3(W, k3):
    """A TF conv_transpose filter [k.., Co, Ci] of a 2-D or 3-D layer as [kz, ky, kx, Co, Ci]."""
    return np.asarray(W).reshape(tuple(k3) + tuple(W.shape[-2:]))


MAX_TAPS = 28      # IG_MAXTAPS (csrc/alq_internal.h): the taps of one GEMM descriptor


def _refusal(k, first_layer=False):
    """The text of alq_model_create's refusal of a conv_transpose of kernel k, or None.  Its backward-data GEMM is one descriptor
    of all prod(k) taps (the forward classes have at most ceil(k / s)^3 each), and igemm_build_plan takes 28 at the most: 4x4x4
    and 5x5x5 are refused unless the layer is the first parameterised one, which has no backward-data launch."""
    taps = int(np.prod(k))
    return None if first_layer or taps <= MAX_TAPS else 'libalq error -4: igemm: %d taps unsupported' % taps


def _assert_refused(sess, ld, in_shape, sk, pars, text):
    from nnal_amd._lib import AlqError
    with pytest.raises(AlqError) as ei:
        _make(sess, ld, in_shape, sk, pars, 4)
    print('refused: %s' % ei.value)
    assert str(ei.value) == text


def _model_of(c, kind):
    """(layer dict, skips, input shape) of a case's first-layer or below-conv model."""
    g = GEOMETRIES[c.tag]
    nd = len(g['k'])
    sp = tuple(g['size'][3 - nd:])
    if kind == 'first':
        ld, sk = convt_ref.first_layer(c.Co, g['k'], g['s'], c.ops)
        return ld, sk, sp + (c.Ci,)
    ld, sk = convt_ref.below_conv(c.Ci, c.Co, g['k'], g['s'], c.ops)
    return ld, sk, sp + (1,)


# ------------------------------------------------------------------------------------------ 0. which forms the cases reach
_LINE = re.compile(r'\[igemm4\] kind (\d)( flipped)? Ci (\d+) Co (\d+) M (\d+)x(\d+)x(\d+): tile (\d+) x \((\d+),(\d+),(\d+)\) .* xw (\d+) ud .*'
                   r'NTW \d( pair)?, LDS \d+ B \(W \d+, (\d) pieces\)')


def _plan_lines(err):
    """igemm4_build_plan's lines of conv_transpose plans (kinds 1 - 4; the bf16x3 plans, not their two-piece fp16 twins)."""
    out = []
    for ln in err.split('\n'):
        if '[igemm4]' not in ln:
            continue
        mt = _LINE.search(ln)
        assert mt, ln
        kind, pieces = int(mt.group(1)), int(mt.group(14))
        if kind >= 1 and pieces == 3:
            out.append(dict(kind=kind, Ci=int(mt.group(3)), Co=int(mt.group(4)), PT=int(mt.group(8)), xw=int(mt.group(12)),
                            pair=mt.group(13) is not None, line=ln.strip()))
    return out


def _forms_run(lines):
    """The forms a model's conv_transpose launches take on the default knobs, from its plan lines: the forward launch is the
    all-classes plan (kind 2 or 4) where one was built, else the per-class plans (kind 3, built for every class either way);
    the backward-data launch is kind 1."""
    fwd_all = [p for p in lines if p['kind'] in (2, 4)]
    run = fwd_all if fwd_all else [p for p in lines if p['kind'] == 3]
    run = run + [p for p in lines if p['kind'] == 1]
    return {(p['kind'], p['pair'], p['xw'] > 0, p['PT'] > 1) for p in run}


# what the table must show: (label, predicate on (kind, pair, xw > 0, PT > 1))
FORMS_REACHED = [
    ('kind 1', lambda f: f[0] == 1),
    ('kind 2 with pair', lambda f: f[0] == 2 and f[1]),
    ('kind 2 without pair', lambda f: f[0] == 2 and not f[1]),
    ('kind 3', lambda f: f[0] == 3),
    ('kind 4', lambda f: f[0] == 4),
    ('natural order (xw = 0)', lambda f: not f[2]),
    ('conflict-free order (xw > 0)', lambda f: f[2]),
    ('several patches per tile', lambda f: f[3]),
]
FORMS_UNREACHABLE = []      # labels of FORMS_REACHED no case reaches, each with its reason in the module docstring


def test_routes_table(sess, capfd):
    """Every first-layer and below-conv model of the case list that alq_model_create accepts and the U-Net level at k = 2, created
    under ALQ_G4_VERBOSE on the default switches, without the classes-as-tiles form and without the two-slot engine."""
    reached, table = set(), []
    models = [(cid, c.ig, c.mb) + _model_of(c, kind) for c, cid in zip(CASES, CASE_IDS) for kind in ('first', 'below')
              if kind == 'first' or _refusal(GEOMETRIES[c.tag]['k']) is None]
    models += [('unet_k2', True, 4) + convt_ref.unet_level([2] * 3, [2] * 3) + ((4, 6, 6, 1),)]
    for cid, ig, mb, ld, sk, in_shape in models:
        pars = netspec.he_init(ld, in_shape, seed=11, skips=sk, bias_std=0.05)
        for route in ('default', 'no_class_tiles', 'no_v4'):
            capfd.readouterr()
            _make(sess, ld, in_shape, sk, pars, mb, route, {'ALQ_G4_VERBOSE': '1'}).close()
            lines = _plan_lines(capfd.readouterr().err)
            forms = _forms_run(lines)
            table.append('%s | %s | %s' % (cid, route, ' ; '.join(sorted('kind %d%s xw%s PT%s' % (f[0], ' pair' if f[1] else '', '>0' if f[2] else '=0',
                                                                                                   '>1' if f[3] else '=1') for f in forms)) or '-'))
            if route == 'no_v4':      # no conv_transpose plan at all
                assert lines == [], (cid, route, [p['line'] for p in lines])
            if not ig:      # the forward launches are off the two-slot engine (the backward GEMM swaps the channels: it may be on it)
                assert all(p['kind'] == 1 for p in lines), (cid, route, [p['line'] for p in lines])
            if route == 'no_class_tiles':
                assert not any(f[0] == 4 for f in forms), (cid, forms)
            reached |= forms
    print('\n'.join('CONVT_ROUTE | ' + t for t in table))      # shown with the captured output of a failure
    for label, pred in FORMS_REACHED:
        hit = any(pred(f) for f in reached)
        assert hit != (label in FORMS_UNREACHABLE), (label, 'reached' if hit else 'not reached', sorted(reached))


# ------------------------------------------------------------------------------------------ 1. exact forward, first-layer models
@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_exact_forward_on_integer_inputs(sess, c):
    size, k3, s3, out, lo, nd = geometry(c.tag)
    ld, sk, in_shape = _model_of(c, 'first')
    x, W, b = convt_ref.exact_inputs(N, size, c.Ci, c.Co, k3, seed=300 + CASES.index(c))
    pars = netspec.he_init(ld, in_shape, seed=12, bias_std=0.05)
    pars['up'] = [W.reshape(pars['up'][0].shape), b]
    want = convt_ref.forward_naive64(x, W, b, s3)
    if 'A' in c.ops:
        want = np.maximum(want, 0.)
    assert want.shape == (N,) + out + (c.Co,) and np.all(want * 2 == np.round(want * 2)) and np.abs(want).max() < 2 ** 22
    assert not x[0].any() and np.count_nonzero(x[1].any(axis=-1)) == int(np.prod([min(v, 2) for v in size]))
    t = _dev(sess, x)
    for route, (_, knob) in ROUTES.items():
        m = _make(sess, ld, in_shape, sk, pars, c.mb, route)
        with _knob(sess, knob):
            for a, e in _passes(N, c.mb):
                n = e - a
                for what in ('forward', 'Fisher'):
                    if what == 'forward':
                        m.forward_device(t[a:e], n)
                    else:
                        m.fisher_device(t[a:e], n, None, 1e-3, want=('p1', 'g0', 'g1'))
                    got = _copy(sess, m, 0, 0, n, (n,) + out + (c.Co,)).astype(np.float64)
                    bad = np.argwhere(got != want[a:e])
                    assert bad.size == 0, ('%s, route %s, %s pass, patches %d..%d: %d of %d outputs differ, first at %r: %r != %r'
                                           % (c, route, what, a, e - 1, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                              want[a:e][tuple(bad[0])]))
        m.close()


# ------------------------------------------------------------------------------------------ 2 - 4. below-conv models
def _variants(labels):
    ls = 1. / N
    return OrderedDict([
        ('mode 0 class 0', dict(mode=0, cls=0)), ('mode 0 class 1', dict(mode=0, cls=1)),
        ('mode 1 rows', dict(mode=1, labels=labels, loss_scale=ls)), ('mode 1 sum', dict(mode=1, labels=labels, loss_scale=ls, per_sample=False)),
    ])


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_forward_backward_and_gradients_below_a_conv(sess, c):
    import torch
    from nnal_amd import ref64
    assert EPS == ref64.DEFAULT_EPS
    size, k3, s3, out, lo, nd = geometry(c.tag)
    ld, sk, in_shape = _model_of(c, 'below')
    seed = 400 + CASES.index(c)
    pars = netspec.he_init(ld, in_shape, seed=seed, bias_std=0.05)
    om64 = OracleModel(ld, in_shape, pars, dtype=torch.float64)
    x, chosen = convt_ref.first_stable_patches(om64, in_shape, seed + 1000, N, 4 * N, fragile_units)
    assert len(chosen) == N, 'too few patches without a fragile decision: pick another seed'
    print('%s: patches %r of stream %d, smallest key %.3e' % (c, chosen, seed + 1000, min(smallest_key(om64, x[[i]]) for i in range(N))))
    if _refusal(k3):      # a refused geometry stays in the table: the refusal and its message are the check
        return _assert_refused(sess, ld, in_shape, sk, pars, _refusal(k3))
    W, b = _w3(pars['up'][0], k3), np.asarray(pars['up'][1]).reshape(-1)
    relu = 'A' in c.ops
    labels = (np.arange(N) % 2).astype(np.int32)
    t = _dev(sess, x)
    bad = []
    for route, (_, knob) in ROUTES.items():
        m = _make(sess, ld, in_shape, sk, pars, c.mb, route)
        with _knob(sess, knob):
            for a, e in _passes(N, c.mb):
                n = e - a
                allv = _variants(labels[a:e])
                for vname in (list(allv) if route == 'default' else ['mode 0 class 1']):
                    kw = allv[vname]
                    rows = m.param_grads_device(t[a:e], n, **kw)[0].cpu().numpy()
                    tag = '%s | %s | %s | patches %d..%d' % (CASE_IDS[CASES.index(c)], route, vname, a, e - 1)
                    act = _copy(sess, m, 0, 0, n, (n,) + size + (c.Ci,))
                    y = _copy(sess, m, 1, 0, n, (n,) + out + (c.Co,))
                    dy = _copy(sess, m, 1, 1, n, (n,) + out + (c.Co,))
                    dlow = _copy(sess, m, 0, 1, n, (n,) + size + (c.Ci,))
                    assert np.count_nonzero(act) and np.count_nonzero(dy) and (act >= 0).all(), tag
                    # 2. forward on the device's own input activation
                    y64, y32 = (convt_ref.forward_torch(act, W, b, s3, dt) for dt in (torch.float64, torch.float32))
                    if relu:
                        y64, y32 = np.maximum(y64, 0), np.maximum(y32, 0)
                        assert not dy[y == 0].any(), (tag, 'the cotangent of an ReLU layer is not masked by its own output')
                    _figure(bad, tag, 'output', y, y64, y32)
                    # 3. backward-data: the cotangent of the conv below, after its ReLU mask
                    _figure(bad, tag, 'cotangent below', dlow, convt_ref.bwd_data64(dy, W, s3, lo, size, act=act),
                            convt_ref.bwd_data_torch(dy, W, s3, act, torch.float32))
                    # 4. the layer's rows of the parameter gradients
                    dW64, db64 = convt_ref.wgrad64(act, dy, k3, s3, lo)
                    dW32, db32 = convt_ref.wgrad_torch(act, dy, W, s3, torch.float32)
                    if rows.ndim == 1:
                        rows, dW64, db64, dW32, db32 = rows[None], dW64.sum(0, keepdims=True), db64.sum(0, keepdims=True), \
                            dW32.sum(0, keepdims=True), db32.sum(0, keepdims=True)
                    gW = np.stack([_w3(m.unflatten(r)[2], k3) for r in rows])
                    gb = np.stack([m.unflatten(r)[3].reshape(-1) for r in rows])
                    _figure(bad, tag, 'dW', gW, dW64, dW32)
                    _figure(bad, tag, 'db', gb, db64, db32)
        m.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 5 - 7. whole models
# name -> (geometry tag or None for a U-Net level, Ci, Co, k of the U-Net level)
WHOLE = OrderedDict(
    [('%s-%dto%d' % (tag, Ci, Co), (tag, Ci, Co, None)) for tag, pairs in (('k2s2', ((8, 8), (4, 8))), ('k4s2', ((8, 16), (8, 6))),
                                                                          ('k234s2', ((8, 16), (8, 6))), ('2d_k4s2', ((16, 4), (12, 8))))
     for Ci, Co in pairs] + [('unet_k2', (None, 16, 8, 2)), ('unet_k4', (None, 16, 8, 4))])
PACKING = [w for w in WHOLE if w.split('-')[0] in ('k2s2', 'k4s2', 'k234s2')]
_WHOLE = {}


def whole(name):
    """Model, chosen patches, labels, a vector and both oracles' gradients: computed once, shared, never modified."""
    if name in _WHOLE:
        return _WHOLE[name]
    tag, Ci, Co, ku = WHOLE[name]
    if tag is None:
        (ld, sk), in_shape = convt_ref.unet_level([ku] * 3, [2] * 3), (4, 6, 6, 1)
    else:
        ld, sk, in_shape = _model_of(Case(tag, Ci, Co, 'MA', 4, True), 'below')
    refused = _refusal([ku] * 3 if tag is None else GEOMETRIES[tag]['k'])
    _WHOLE[name] = whole_record(name, ld, sk, in_shape, 500 + list(WHOLE).index(name), refused)
    return _WHOLE[name]


def whole_record(name, ld, sk, in_shape, seed, refused):
    """What the whole-model checks share for one model: weights, both oracles, N patches without a fragile decision, labels, a
    vector and both oracles' gradients."""
    import torch
    pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    om64 = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
    om32 = OracleModel(ld, in_shape, pars, skips=sk)
    x, chosen = convt_ref.first_stable_patches(om64, in_shape, seed + 1000, N, 6 * N, fragile_units)
    assert len(chosen) == N, 'too few patches without a fragile decision: pick another seed'
    print('%s: patches %r of stream %d, smallest key %.3e' % (name, chosen, seed + 1000, min(smallest_key(om64, x[[i]]) for i in range(N))))
    rs = np.random.RandomState(seed + 2000)
    labels = rs.randint(0, 2, size=N).astype(np.int32)
    names = list(pars.keys())
    v = [rs.randn(*np.asarray(a).shape).astype(np.float32) for nme in names for a in pars[nme]]
    g64 = [[[np.asarray(a, np.float64) for a in om64.grad_log_post(j, x[[i]])] for j in (0, 1)] for i in range(N)]
    g32 = [[[np.asarray(a) for a in om32.grad_log_post(j, x[[i]])] for j in (0, 1)] for i in range(N)]
    return dict(refused=refused, name=name, seed=seed, ld=ld, sk=sk, in_shape=in_shape, n=N, pars=pars, x=x, labels=labels, v=v, names=names, om64=om64, om32=om32,
                g64=g64, g32=g32, p64=om64.forward(x)['posteriors'].astype(np.float64), arrays=[nme + s for nme in names for s in ('/W', '/b')])


def _refused(sess, d):
    """True after asserting the refusal where alq_model_create refuses the model (_refusal)."""
    if d['refused']:
        _assert_refused(sess, d['ld'], d['in_shape'], d['sk'], d['pars'], d['refused'])
    return d['refused'] is not None


def _mk(sess, d, route='default', **kw):
    return _make(sess, d['ld'], d['in_shape'], d['sk'], d['pars'], 4, route, **kw)


@pytest.mark.parametrize('name', list(WHOLE))
def test_whole_model_param_grads_vs_fp64(sess, name):
    """tests/test_gpu_grads_fp64.test_param_grads_vs_fp64 on these models: every W and b array, modes 0 and 1, rows and sum."""
    d = whole(name)
    if _refused(sess, d):
        return
    check_param_grads(sess, d, _mk, ('default', 'no_v4_v3'))


def check_param_grads(sess, d, mk, routes):
    """The body of test_whole_model_param_grads_vs_fp64 on a model record of the form whole() builds (N patches, passes of 4);
    mk(sess, d, route) creates the device model."""
    from tests.test_gpu_grads_fp64 import mode1_refs
    name = d['name']
    g64, g32, lab = d['g64'], d['g32'], d['labels']
    rows64, rows32, sum64, sum32 = mode1_refs(d)
    t = _dev(sess, d['x'])
    bad = []
    for route in routes:
        m = mk(sess, d, route)
        got = {'mode 0 class 0': [], 'mode 0 class 1': [], 'mode 1 rows': []}
        total = np.zeros(m.num_params)
        for a, e in _passes(N, 4):
            for cls in (0, 1):
                g, post, _ = m.param_grads_device(t[a:e], e - a, 0, cls=cls, want_post=True)
                got['mode 0 class %d' % cls] += [m.unflatten(r) for r in g.cpu().numpy()]
                assert np.abs(post.cpu().numpy().astype(np.float64) - d['p64'][:, a:e]).max() <= 2e-6
            g = m.param_grads_device(t[a:e], e - a, 1, labels=lab[a:e], loss_scale=1. / N)[0]
            got['mode 1 rows'] += [m.unflatten(r) for r in g.cpu().numpy()]
            total += m.param_grads_device(t[a:e], e - a, 1, labels=lab[a:e], loss_scale=1. / N, per_sample=False)[0].cpu().numpy().astype(np.float64)
        variants = [('mode 0 class %d' % j, got['mode 0 class %d' % j], [g64[i][j] for i in range(N)], [g32[i][j] for i in range(N)]) for j in (0, 1)]
        variants.append(('mode 1 rows', got['mode 1 rows'], rows64, rows32))
        # the two passes' sums are added in fp64 here, so each pass's fp32 sum is held to the same bar as one sum would be
        variants.append(('mode 1 sum', [m.unflatten(total.astype(np.float32))], [sum64], [sum32]))
        m.close()
        for what, gd, r64, r32 in variants:
            for k, arr in enumerate(d['arrays']):
                _figure(bad, '%s | %s | %s' % (name, route, what), arr, np.stack([r[k] for r in gd]), np.stack([r[k] for r in r64]),
                        np.stack([r[k] for r in r32]))
    assert not bad, bad


def _sq(arrs):
    return np.array([np.sum(np.asarray(a, dtype=np.float64) ** 2) for a in arrs])


@pytest.mark.parametrize('name', list(WHOLE))
def test_whole_model_other_entry_points_vs_fp64(sess, name):
    """alq_grad_sqnorms, alq_class_layer_sums, alq_diag_fisher and alq_hess_vecp under the bars tests/test_gpu_grads_fp64.py holds
    NET-C to: 1e-4 r + 1e-12 row total; per layer 2 e(rows) + 6e-8 mean |entry|; 2e-3 ref + 1e-6 max ref; test_gpu_hvp.bars, and the product also under
    the fp64 bar hvp_cases.bars64."""
    d = whole(name)
    if _refused(sess, d):
        return
    check_other_entry_points(sess, d, _mk)


def check_other_entry_points(sess, d, mk):
    """The body of test_whole_model_other_entry_points_vs_fp64 on a model record of the form whole() builds."""
    name = d['name']
    g64, lab = d['g64'], d['labels']
    p1 = d['p64'][1]
    m = mk(sess, d)
    t = _dev(sess, d['x'])
    L = m.L
    ref = {j: np.stack([_sq(g64[i][j]) for i in range(N)]) for j in (0, 1)}
    for cls in (0, 1, -1):
        got = m.grad_sqnorms_device(t, N, cls=cls).cpu().numpy()
        r = ref[cls] if cls >= 0 else ref[0] / (p1[:, None] ** 2)
        err = np.abs(got - r)
        print('%s sqnorms class %d: max err / r %.3e (bar 1e-4)' % (name, cls, np.max(err / (r + 1e-300))))
        assert np.all(err <= 1e-4 * r + 1e-12 * r.sum(axis=1, keepdims=True)), (name, cls)
    s64 = np.array([[alpath.shrink_gradient(g64[i][j]) for j in (0, 1)] for i in range(N)])
    mean_abs = np.array([[[(np.abs(gr[2 * q]).sum() + np.abs(gr[2 * q + 1]).sum()) / (gr[2 * q].size + gr[2 * q + 1].size)
                           for q in range(L)] for gr in (g64[i][0], g64[i][1])] for i in range(N)]).mean(axis=(0, 1))
    g_rows = m.shrunk_class_gradients(d['x'])[0].cpu().numpy()
    g_fused = m.class_layer_sums_device(t, N, np.tile(np.arange(2), (N, 1))).cpu().numpy()
    assert g_fused.shape == g_rows.shape == s64.shape == (N, 2, L)
    e_fused, e_rows = np.abs(g_fused - s64).max(axis=(0, 1)), np.abs(g_rows - s64).max(axis=(0, 1))
    for q in range(L):
        print('%s layer sums %s: e(fused) %.3e  e(rows) %.3e  floor %.3e' % (name, d['names'][q], e_fused[q], e_rows[q], 6e-8 * mean_abs[q]))
    assert np.all(e_fused <= 2 * e_rows + 6e-8 * mean_abs), (name, e_fused, e_rows)
    dref = [sum(g64[i][lab[i]][k] ** 2 for i in range(N)) / N for k in range(len(d['arrays']))]
    for arr, a, r in zip(d['arrays'], m.diagonal_fisher(d['x'], lab), dref):
        assert a.shape == r.shape and a.dtype == np.float64, arr
        err = np.abs(a - r)
        print('%s diag fisher %s: max err / max ref = %.3e' % (name, arr, err.max() / r.max()))
        assert np.all(err <= 2e-3 * r + 1e-6 * r.max()), (name, arr)
    hv64, hv32 = (oracle_hv(om, d['x'], lab, d['v'], d['names'], 1. / N) for om in (d['om64'], d['om32']))
    hv = m.hess_vecp(d['x'], lab, d['v'])
    # the product is evaluated in fp64: also under the fp64 bar of tests/hvp_cases.py, on patches with its decision margin
    # (tests/test_hvp_cases_host.py proves the bar's three conditions for every whole model that reaches this line)
    tight = hvp_cases.whole_tight(d)
    assert tight['bad'] == [], (name, tight['bad'])
    hv_tight = hv if tight['chosen'] is None else m.hess_vecp(tight['x'], lab, d['v'])
    m.close()
    for arr, a, a64, a32, b in zip(d['arrays'], hv, hv64, hv32, bars(hv64, hv32)):
        e = np.abs(a - a64).max()
        print('%s Hv %s: e_dev %.3e  e_32 %.3e  bar %.3e' % (name, arr, e, np.abs(a32 - a64).max(), b))
        assert a.dtype == np.float64 and a.shape == a64.shape and e <= b, (name, arr, e, b)
    hvp_cases.hold64('%s Hv (patches %r)' % (name, tight['chosen'] or 'of the other checks'), hv_tight, tight['y'], d['arrays'])


@pytest.mark.parametrize('name', list(WHOLE))
def test_whole_model_fisher_pass_vs_fp64(sess, name):
    """p1, g0, g1 and A of the Fisher pass (boxdot_convT_kernel, the conv_transpose geometry of lsum.hip, the fused epilogues)
    against factored_ref in fp64, the bars of test_gpu_parity.test_netc_other_shapes_vs_fp64, on every sample."""
    d = whole(name)
    if _refused(sess, d):
        return
    check_fisher_pass(sess, d, _mk, ROUTES)


def check_fisher_pass(sess, d, mk, routes):
    """The body of test_whole_model_fisher_pass_vs_fp64 on a model record of the form whole() builds, on every route of the table
    `routes` (of the form of ROUTES)."""
    name = d['name']
    p64, S64, sizes = factored_ref.factored_unit_scores(d['om64'], d['x'].astype(np.float64))
    g64, h64, A64 = factored_ref.fisher_from_unit(p64[1], S64, sizes, 1e-3)
    t = _dev(sess, d['x'])
    for route, (_, knob) in routes.items():
        m = mk(sess, d, route)
        with _knob(sess, knob):
            rs = [m.fisher_device(t[a:e], e - a, None, 1e-3, want=('p1', 'g0', 'g1', 'A')) for a, e in _passes(N, 4)]
            r = {k: np.concatenate([q[k].cpu().numpy() for q in rs]) for k in ('p1', 'g0', 'g1', 'A')}
        m.close()
        e_p = np.abs(r['p1'] - p64[1]).max()
        print('%s | %s | Fisher pass: max |p1 - p64| %.3e' % (name, route, e_p))
        assert e_p <= 5e-6, (name, route, e_p)
        for key, ref in (('g0', g64), ('g1', h64)):
            scale = np.abs(ref).max(axis=0, keepdims=True)
            err = np.abs(r[key] - ref)
            print('%s | %s | %s: max err / per-layer max %.3e (bar 5e-4)' % (name, route, key, np.max(err / (scale + 1e-300))))
            assert (err <= 5e-4 * scale + 1e-9).all(), (name, route, key, err.max())
        np.testing.assert_allclose(r['A'], A64, rtol=2e-3, atol=1e-3 * np.abs(A64 - 1e-3 * np.eye(A64.shape[1])).max())


@pytest.mark.parametrize('name', PACKING)
def test_device_weight_packing_same_bits(sess, name):
    """alq_model_set_weights_device against alq_model_set_weights (tests/test_gpu_weights_device.py): the same bits out of the
    forward pass, the Fisher pass and the parameter gradients."""
    d = whole(name)
    if _refused(sess, d):
        return
    check_packing(sess, d, _mk)


def check_packing(sess, d, mk):
    """The body of test_device_weight_packing_same_bits on a model record of the form whole() builds."""
    name = d['name']
    t = _dev(sess, d['x'])
    outs = []
    for dw in (False, True):
        m = mk(sess, d, extra_env={} if dw else {'ALQ_HOST_REPACK': '1'}, device_weights=dw)
        assert m._host_repack == (not dw)
        o = OrderedDict()
        for a, e in _passes(N, 4):
            o['post%d' % a] = m.forward_device(t[a:e], e - a)[0].cpu().numpy()
            r = m.fisher_device(t[a:e], e - a, None, 1e-3, want=('p1', 'g0', 'g1', 'A'))
            for k in ('p1', 'g0', 'g1', 'A'):
                o['%s%d' % (k, a)] = r[k].cpu().numpy()
            o['grads%d' % a] = m.param_grads_device(t[a:e], e - a, 1, labels=d['labels'][a:e], loss_scale=1. / N)[0].cpu().numpy()
        m.close()
        outs.append(o)
    for k in outs[0]:
        assert np.isfinite(outs[0][k]).all() and np.abs(outs[0][k]).max() > 0, k
        np.testing.assert_array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8), err_msg='%s: %s' % (name, k))
