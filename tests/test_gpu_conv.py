"""The plain stride-1 conv beyond 3x3x3 and 5x5: every route of the layer's device code against fp64 references (GPU box).

The conv carries almost all of the FLOPs and sits in front of the largest dispatch tree - same_pads / conv_fwd_desc / conv_bwd_desc
(an even window pads asymmetrically and the backward taps flip to lo - t), igemm_build_plan (smallc, CB = 32, NTW / NB, the tile
search, 28 taps), igemm2 / igemm3 / direct_build_plan and their refusals, igemm4_build_plan kind 0 and its flipped twin (pair form,
halo classes, PT), plan_conv (the wide-2-D rule, the fp16-pair twins, the output-channel split), alloc_activations (split against
interleaved concat), set_weights and the device packers, wgrad_kernel, gnorm.hip, the conv geometry of lsum.hip, the conv branches
of hvp.hip - and the rest of the suite runs it at 3x3x3 / 3x3, 5x5 and 1x1 on near-cubic volumes, always at odd k, through whole-
model scores only.  This file is the counterpart of tests/test_gpu_convt.py (whose helpers it imports) for ALQ_CONV: the
geometries of tests/conv_ref.py (even and mixed windows, in-plane / through-plane / row windows, 1, 24, 25 and 28 taps, several
tiles per patch; every volume ragged), channel pairs on and off the two-slot engine and wide ones, both op orders, every switch.

Models (tests/conv_ref.py), built through device.DeviceModel, internals read with alq_model_debug_copy:
  first-layer   conv -> conv(4, 1x1) 'MA' -> fc(2): the layer reads the caller's x, so x, W and b are small integers and the output
                must EQUAL the loops of the definition in fp64 (check 1), after a forward pass and after a Fisher pass;
  below-conv    conv(Ci, 3^nd, 'MA') -> conv -> conv(4, 1x1) 'MA' -> fc(2): the layer's input activation and its own cotangent are
                read from the device after alq_param_grads and taken as given; its output (check 2), the cotangent of the conv below
                (check 3: (a > 0) sum_t dy[q + lo - t] W[t]^T, zero wherever the activation is) and its dW / db rows (check 4) follow
                in fp64.  After a Fisher pass on the default route the channel-sum fields (alq_model_debug_copy what = 2, 3, 11) are
                held to the sums of the tensors copied beside them, each where the pass stores it (_check_sums) (tests/test_gpu_pool._assert_sums);
  whole models  below-conv models, the two concat models of tests/test_gpu_parity.py with 2x2x2 and 1x3x3 consumers on ragged
                volumes and a wide model against OracleModel(dtype=float64), under the checks and bars of tests/test_gpu_convt.py
                (imported: check_param_grads, check_other_entry_points, check_fisher_pass, check_packing).
N = 5 patches under max_batch = 4 are two passes with a ragged last group; two cases take max_batch = 8.

Tolerances of checks 2 - 4: test_gpu_convt._bar unchanged - e_dev <= R_FACTOR R_DEV_OVER_F32 e_32 + 6e-8 mean |ref64|, never looser
than 2e-4 max |ref64| + 1e-9, e_32 the error of fp32 torch on the same inputs.  Every figure is printed before it is asserted.

Refused geometries (conv_ref.REFUSED; _refused_text): a conv's forward GEMM is one descriptor of all prod(k) taps, so 4x4x4, 3x3x4
and 6x6 are refused with "igemm: N taps unsupported" even as the first layer (a conv_transpose is not: asserted), a stride other
than 1 with "layer i: strided conv", 3x3x3 on 44 channels with the single-chunk limit's text; 37 and 36 channels run.

Routes: the switches are set around model creation, knobs 4 and 5 around the calls; the wide pairs take WIDE_ROUTES, four of the
eleven (the file's runtime is held to about twice tests/test_gpu_convt.py's: 6.8 s there, 17.3 s here on all routes).  test_routes_table reads igemm4_build_plan's own
lines (ALQ_G4_VERBOSE) and the profiler's launch counts.  The profiler files a two-slot launch under the class of the igemm3 launch
it replaces (igemm3_fwd / igemm3_bwd, or igemm_f16x2 on fp16 pairs), so which of the two engines ran is not in the counts: the
wide-2-D rule is observed through knob 5 instead (test_wide_2d_rule: taking the two-slot engine away at call time changes no bit of
the output where the rule has already done so, and changes some where it has not).  FORMS_UNREACHABLE lists what no case reaches.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests import conv_ref, test_gpu_convt as tc  # noqa: E402
from tests.conv_ref import GEOMETRIES, REFUSED, geometry  # noqa: E402
from tests.convt_ref import first_stable_patches  # noqa: E402
from tests.test_gpu_convt import _copy, _dev, _figure, _knob, _make, _passes  # noqa: E402
from tests.test_gpu_grads_fp64 import smallest_key  # noqa: E402
from tests.test_gpu_hvp import EPS, fragile_units  # noqa: E402
from tests.test_gpu_pool import _assert_sums  # noqa: E402

N = tc.N

Case = namedtuple('Case', 'tag Ci Co ops mb kind')      # kind: 'ig' on the two-slot engine, 'off' off it, 'wide', 'first' (first-layer only)
IG_PAIRS = [(8, 8), (16, 4), (8, 16), (8, 32), (32, 8)]
OFF_PAIRS = [(4, 8), (12, 8), (8, 6), (8, 40)]      # smallc twice, Co % 4, NT = 3
# output-channel split in slices of 32, 16 and 48; 72: no slice width divides it and NB = 5, the general kernel
WIDE_PAIRS = [(8, 64), (8, 80), (8, 144), (8, 72)]
CO_SPLIT_W = {64: 32, 80: 16, 144: 48, 72: None}


def _cases():
    out = []
    for i, tag in enumerate(GEOMETRIES):
        for kind, (Ci, Co) in (('ig', IG_PAIRS[i % 5]), ('off', OFF_PAIRS[i % 4]), ('wide', WIDE_PAIRS[i % 4])):
            for ops in ('M', 'MA'):
                out.append(Case(tag, Ci, Co, ops, 4, kind))
    out += [Case('k1', 32, 8, 'M', 4, 'ig'), Case('k1', 32, 8, 'MA', 4, 'ig')]      # one tap, Ci % 32 == 0: CB = 32
    out += [Case('k3_tiles', 8, 144, 'MA', 4, 'wide')]      # the largest tensor of the file
    # the single-chunk limit of a smallc layer: K = 999 (KC = 1000) and 972
    out += [Case(tag, Ci, 8, ops, 4, 'off') for (tag, Ci), ops in zip(conv_ref.SMALLC_LIMIT, ('M', 'MA'))]
    # several patches per tile (PT > 1 needs the batch to hold them)
    out += [Case('k3_ragged', 8, 8, 'M', 8, 'ig'), Case('k2', 8, 16, 'MA', 8, 'ig')]
    # direct.hip's own conv (Ci <= 4, Co in 8 .. 32, tiles of 256 rows) and Ci = 5, just outside it: the caller's x has Ci channels
    firsts = [(1, 8), (3, 24), (4, 8), (1, 24), (3, 8), (4, 24), (5, 8), (5, 24)]
    for j, (Ci, Co) in enumerate(firsts):
        out.append(Case(('k3_ragged', 'k2', 'k4_2d', 'k3_tiles')[j % 4], Ci, Co, ('M', 'MA')[j % 2], 4, 'first'))
    return out


CASES = _cases()
CASE_IDS = ['%s-%dto%d-%s-mb%d' % c[:5] for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)
BELOW = [c for c in CASES if c.kind != 'first']

# name -> (environment around model creation, alq_debug_set knob around the calls): test_gpu_convt.ROUTES without no_class_tiles
# (no meaning for a conv), then the switches plan_conv and the two-slot engine's dispatch read
ROUTES = OrderedDict([(r, v) for r, v in tc.ROUTES.items() if r != 'no_class_tiles'] + [
    ('no_co_split', ({'ALQ_NO_CO_SPLIT': '1'}, None)),
    ('no_wide2d_rule', ({'ALQ_NO_WIDE2D_RULE': '1'}, None)),
    ('no_v3_f16', ({'ALQ_NO_V3_F16': '1'}, None)),
    ('no_fixed', ({'ALQ_NO_FIXED': '1'}, None)),
])
assert list(ROUTES)[:7] == ['default', 'no_v4', 'no_v4_v3', 'no_v4_v3_v2', 'no_f16x2', 'knob4', 'knob5']
# The wide pairs cost the most (the tiled 2-D map at 144 channels is the largest tensor) and differ from the others in plan_conv's
# output-channel split alone: they take both arms of it with and without the two-slot engine and the general kernels
WIDE_ROUTES = OrderedDict((r, ROUTES[r]) for r in ('default', 'no_v4', 'no_v4_v3_v2', 'no_co_split'))
CONCAT_ROUTES = OrderedDict(list(ROUTES.items()) + [('no_split', ({'ALQ_NO_SPLIT': '1'}, None))])


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _mk_model(sess, ld, in_shape, sk, pars, mb, route='default', **kw):
    return _make(sess, ld, in_shape, sk, pars, mb, route, routes=CONCAT_ROUTES, **kw)


def _routes(c):
    return WIDE_ROUTES if c.kind == 'wide' else ROUTES


def _model_of(c, kind):
    """(layer dict, skips, input shape) of a case's first-layer or below-conv model."""
    g = GEOMETRIES[c.tag]
    nd = len(g['k'])
    sp = tuple(g['size'][3 - nd:])
    if kind == 'first':
        ld, sk = conv_ref.first_layer(c.Co, g['k'], c.ops)
        return ld, sk, sp + (c.Ci,)
    ld, sk = conv_ref.below_conv(c.Ci, c.Co, g['k'], c.ops)
    return ld, sk, sp + (1,)


# ------------------------------------------------------------------------------------------ refused geometries
def _refused_text(tag, layer):
    t = REFUSED[tag]['text']
    return 'libalq error -4: ' + (t % layer if '%d' in t else t)


@pytest.mark.parametrize('tag', list(REFUSED))
def test_refused_geometries(sess, tag):
    """alq_model_create's refusal and its text, as the first layer and below a conv."""
    g = REFUSED[tag]
    nd = len(g['k'])
    sp = tuple(g['size'][3 - nd:])
    for layer, (ld, sk), in_shape in ((0, conv_ref.first_layer(8, g['k'], 'MA', g['s']), sp + (g['Ci'],)),
                                      (1, conv_ref.below_conv(g['Ci'], 8, g['k'], 'MA', g['s']), sp + (1,))):
        pars = netspec.he_init(ld, in_shape, seed=5, bias_std=0.05)
        tc._assert_refused(sess, ld, in_shape, sk, pars, _refused_text(tag, layer))
    # unlike a conv_transpose, whose forward classes hold ceil(k / s)^3 taps each: 4x4x4 is no refusal there as the first layer
    if tag == 'k4':
        assert tc._refusal([4, 4, 4], first_layer=True) is None and tc._refusal([4, 4, 4]) == _refused_text(tag, 1)


# ------------------------------------------------------------------------------------------ 0. which forms the cases reach
def _plan_lines(err):
    """igemm4_build_plan's lines of conv plans (kind 0, forward and flipped; the bf16x3 plans, not their two-piece fp16 twins)."""
    out = []
    for ln in err.split('\n'):
        if '[igemm4]' not in ln:
            continue
        mt = tc._LINE.search(ln)
        assert mt, ln
        if int(mt.group(1)) == 0 and int(mt.group(14)) == 3:
            out.append(dict(flipped=mt.group(2) is not None, Ci=int(mt.group(3)), Co=int(mt.group(4)), PT=int(mt.group(8)), xw=int(mt.group(12)),
                            pair=mt.group(13) is not None, line=ln.strip()))
    return out


_FWD_CLASSES = ('igemm_fwd', 'igemm3_fwd', 'direct_conv', 'igemm_f16x2')


def _counts(sess, m, t, n):
    """Launch counts per profiler class of one forward pass, one alq_param_grads call (forward + general backward) and one Fisher
    pass."""
    out = OrderedDict()
    for what, call in (('fwd', lambda: m.forward_device(t, n)), ('grads', lambda: m.param_grads_device(t, n, 0, cls=1)),
                       ('fisher', lambda: m.fisher_device(t, n, None, 1e-3, want=('p1', 'g0', 'g1')))):
        sess.prof_reset()
        call()
        out[what] = {k: v['launches'] for k, v in sess.prof_read().items() if v['launches']}
    return out


# what the table must show: label -> predicate on a record (case, model kind, route, plan lines of the conv under test, counts)
def _cv(r, flipped):
    """Plan lines of the conv under test: forward Ci -> Co, flipped Co -> Ci."""
    c = r['c']
    ci, co = (c.Co, c.Ci) if flipped else (c.Ci, c.Co)
    return [p for p in r['lines'] if p['flipped'] == flipped and p['Ci'] == ci and p['Co'] == co]


def _mix(r):
    """Plan lines of the 1x1 conv behind the conv under test (Co -> 4 channels)."""
    return [p for p in r['lines'] if not p['flipped'] and p['Ci'] == r['c'].Co and p['Co'] == 4]


def _n(r, cls):
    return r['counts']['grads'].get(cls, 0)


FORMS_REACHED = OrderedDict([
    ('kind 0 forward', lambda r: bool(_cv(r, False))),
    ('kind 0 flipped (backward-data)', lambda r: r['kind'] == 'below' and bool(_cv(r, True))),
    ('forward with the pair form', lambda r: any(p['pair'] for p in _cv(r, False))),
    ('forward without the pair form', lambda r: any(not p['pair'] for p in _cv(r, False))),
    ('flipped with the pair form', lambda r: r['kind'] == 'below' and any(p['pair'] for p in _cv(r, True))),
    ('several patches per tile', lambda r: any(p['PT'] > 1 for p in _cv(r, False) + _cv(r, True))),
    ('one patch per tile', lambda r: any(p['PT'] == 1 for p in _cv(r, False) + _cv(r, True))),
    ('natural order (xw = 0)', lambda r: any(p['xw'] == 0 for p in _cv(r, False) + _cv(r, True))),
    ('conflict-free order (xw > 0)', lambda r: any(p['xw'] > 0 for p in _cv(r, False) + _cv(r, True))),
    # a first-layer model with Ci <= 4: mix reads >= 8 channels, so a direct_conv launch is the conv's own
    ('direct_conv class', lambda r: r['kind'] == 'first' and r['c'].Ci <= 4 and r['counts']['fwd'].get('direct_conv', 0) > 0),
    # Launches of a first-layer model's forward pass are the conv's and mix's (fc(2) is the fc_small class), of a below-conv model's
    # backward pass the conv's and mix's (low is the first parameterised layer; mix hands 4 channels down: smallc, the general kernel)
    # (a wide pair's slices have two-slot plans of their own: not meant)
    ('igemm3_fwd without a two-slot plan, default switches', lambda r: r['route'] == 'default' and r['kind'] == 'first' and r['c'].kind == 'off' and
     not _cv(r, False) and _n(r, 'igemm_fwd') == 0 and _n(r, 'direct_conv') == 0 and _n(r, 'igemm3_fwd') >= 1),
    ('igemm3_bwd without a two-slot plan, default switches', lambda r: r['route'] == 'default' and r['kind'] == 'below' and not _cv(r, True) and
     _n(r, 'igemm_bwd') == 1 and _n(r, 'igemm3_bwd') >= 1),
    ('igemm_fwd class on the default switches', lambda r: r['route'] == 'default' and r['kind'] == 'first' and not _cv(r, False) and
     _n(r, 'igemm_fwd') == (1 if _mix(r) else 2)),
    ('igemm_bwd class on the default switches', lambda r: r['route'] == 'default' and r['kind'] == 'below' and not _cv(r, True) and
     _n(r, 'igemm_bwd') == 2),
    ('fp16x2 class', lambda r: r['counts']['fwd'].get('igemm_f16x2', 0) + r['counts']['fisher'].get('igemm_f16x2', 0) > 0),
])
FORMS_UNREACHABLE = []      # labels of FORMS_REACHED no case reaches, each with its reason in the module docstring


def _fwd_launches(counts):
    return sum(counts['fwd'].get(k, 0) for k in _FWD_CLASSES)


def test_routes_table(sess, capfd):
    """Every first-layer and below-conv model of the case list, created under ALQ_G4_VERBOSE on the default switches, without the
    two-slot engine and without igemm3 (wide pairs: also under ALQ_NO_CO_SPLIT); one forward pass, one alq_param_grads call and one
    Fisher pass under the profiler."""
    records, table, problems = [], [], []
    sess.prof_enable(True)
    try:
        for c, cid in zip(CASES, CASE_IDS):
            for kind in (('first',) if c.kind == 'first' else ('first', 'below')):
                ld, sk, in_shape = _model_of(c, kind)
                pars = netspec.he_init(ld, in_shape, seed=11, skips=sk, bias_std=0.05)
                n = min(N, c.mb)
                t = _dev(sess, np.random.RandomState(17).randn(n, *in_shape).astype(np.float32))
                split = {}
                for route in ('default', 'no_v4', 'no_v4_v3') + (('no_co_split',) if c.kind == 'wide' else ()):
                    capfd.readouterr()
                    m = _mk_model(sess, ld, in_shape, sk, pars, c.mb, route, extra_env={'ALQ_G4_VERBOSE': '1'})
                    lines = _plan_lines(capfd.readouterr().err)
                    counts = _counts(sess, m, t, n)
                    m.close()
                    r = dict(c=c, kind=kind, route=route, lines=lines, counts=counts)
                    records.append(r)
                    table.append('%s | %s | %s | %s | %s' % (cid, kind, route, ' ; '.join(
                        '%s%d->%d%s xw%s PT%d' % ('flipped ' if p['flipped'] else '', p['Ci'], p['Co'], ' pair' if p['pair'] else '',
                                                  '>0' if p['xw'] else '=0', p['PT']) for p in lines) or '-',
                        ' '.join('%s{%s}' % (w, ','.join('%s:%d' % kv for kv in sorted(cn.items()))) for w, cn in counts.items())))
                    if route != 'default' and route != 'no_co_split' and lines:      # ALQ_DISABLE_V4: no two-slot plan at all
                        problems.append((cid, kind, route, [p['line'] for p in lines]))
                    if (c.kind == 'ig') != bool(_cv(r, False)) and route == 'default':
                        # 'ig' pairs have a two-slot forward plan; the others' forward launch is off that engine
                        problems.append((cid, kind, route, 'forward plan', [p['line'] for p in lines]))
                    split[route] = _fwd_launches(counts)
                if c.kind == 'wide' and kind == 'first':
                    # the output-channel split: cout / w forward launches where ALQ_NO_CO_SPLIT makes one
                    w = CO_SPLIT_W[c.Co]
                    extra = c.Co // w - 1 if w else 0
                    # without the two-slot engine the slices need igemm3, and igemm2_build_plan takes 27 taps: no split at 28
                    extra3 = extra if int(np.prod(GEOMETRIES[c.tag]['k'])) <= 27 else 0
                    if not (split['default'] - split['no_co_split'] == extra and split['no_v4'] - split['no_co_split'] == extra3):
                        problems.append((cid, 'output-channel split', extra, extra3, split))
    finally:
        sess.prof_enable(False)
        print('\n'.join('CONV_ROUTE | ' + t for t in table))      # shown with the captured output of a failure
    for label, pred in FORMS_REACHED.items():
        hit = [r for r in records if pred(r)]
        print('CONV_FORM | %s | %d records, first: %s' % (label, len(hit), ('%s %s %s' % (hit[0]['c'], hit[0]['kind'], hit[0]['route'])) if hit else '-'))
    assert not problems, problems
    for label, pred in FORMS_REACHED.items():
        hit = any(pred(r) for r in records)
        assert hit != (label in FORMS_UNREACHABLE), (label, 'reached' if hit else 'not reached')


@pytest.mark.parametrize('tag,fires', [('k5_2d', True), ('k155_3d', False)])
def test_wide_2d_rule(sess, tag, fires):
    """plan_conv's rule for 2-D windows of 25 taps or more (igemm3 instead of the two-slot engine) fires at ID == 1 only, and
    ALQ_NO_WIDE2D_RULE is its other arm: where the forward launch is igemm3's already, knob 5 (no two-slot engine at call time)
    changes no bit of the layer's output; where it is the two-slot engine's, the two engines sum in another order and some bits
    differ.  8 -> 16 channels at 25 taps: both engines have a plan.  Every output is also held to fp64 (the cap of the bar)."""
    import torch
    c = Case(tag, 8, 16, 'M', 4, 'ig')
    size, k3, lo, nd = geometry(tag)
    ld, sk, in_shape = _model_of(c, 'first')
    pars = netspec.he_init(ld, in_shape, seed=21, bias_std=0.05)
    x = np.random.RandomState(22).randn(4, *in_shape).astype(np.float32)
    t = _dev(sess, x)
    y64 = conv_ref.forward_torch(x.reshape((4,) + size + (8,)), conv_ref._w5(pars['cv'][0]), pars['cv'][1], torch.float64)
    same = {}
    for route in ('default', 'no_wide2d_rule'):
        m = _mk_model(sess, ld, in_shape, sk, pars, 4, route)
        outs = []
        for knob in (None, 5):
            with _knob(sess, knob):
                m.param_grads_device(t, 4, 0, cls=1)
                outs.append(_copy(sess, m, 0, 0, 4, (4,) + size + (16,)))
        m.close()
        for o in outs:
            assert np.abs(o - y64).max() <= 2e-4 * np.abs(y64).max()
        same[route] = bool(np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)))
        print('%s | %s | output with and without the two-slot engine: %s' % (tag, route, 'same bits' if same[route] else 'bits differ'))
    assert same == {'default': fires, 'no_wide2d_rule': False}, (tag, same)


# ------------------------------------------------------------------------------------------ 1. exact forward, first-layer models
@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_exact_forward_on_integer_inputs(sess, c):
    size, k3, lo, nd = geometry(c.tag)
    ld, sk, in_shape = _model_of(c, 'first')
    x, W, b = conv_ref.exact_inputs(N, size, c.Ci, c.Co, k3, seed=300 + CASES.index(c))
    pars = netspec.he_init(ld, in_shape, seed=12, bias_std=0.05)
    pars['cv'] = [W.reshape(pars['cv'][0].shape), b]
    want = conv_ref.forward_naive64(x, W, b)
    if 'A' in c.ops:
        want = np.maximum(want, 0.)
    # integers (half-integers through b) far below 2^24: at most 28 taps x 64 channels of products <= 16 per output
    assert int(np.prod(k3)) * c.Ci <= 28 * 64 and max(np.abs(x).max(), np.abs(W).max(), np.abs(b).max()) <= 4
    assert want.shape == (N,) + size + (c.Co,) and np.all(want * 2 == np.round(want * 2)) and np.abs(want).max() < 2 ** 22
    assert not x[0].any() and np.count_nonzero(x[1].any(axis=-1)) == int(np.prod([min(v, 2) for v in size]))
    t = _dev(sess, x)
    for route, (_, knob) in _routes(c).items():
        m = _mk_model(sess, ld, in_shape, sk, pars, c.mb, route)
        with _knob(sess, knob):
            for a, e in _passes(N, c.mb):
                n = e - a
                for what in ('forward', 'Fisher'):
                    if what == 'forward':
                        m.forward_device(t[a:e], n)
                    else:
                        m.fisher_device(t[a:e], n, None, 1e-3, want=('p1', 'g0', 'g1'))
                    got = _copy(sess, m, 0, 0, n, (n,) + size + (c.Co,)).astype(np.float64)
                    bad = np.argwhere(got != want[a:e])
                    assert bad.size == 0, ('%s, route %s, %s pass, patches %d..%d: %d of %d outputs differ, first at %r: %r != %r'
                                           % (c, route, what, a, e - 1, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                              want[a:e][tuple(bad[0])]))
        m.close()


# ------------------------------------------------------------------------------------------ 2 - 4. below-conv models
def _check_sums(sess, m, n, size, c, tag):
    """After a Fisher pass: the channel-sum fields around the conv under test (layer 1) against the sums of the tensors copied
    beside them.  What is stored where (passes.hip): a spatial layer behind another reads its input's sums from the producer's
    output field (what = 11 of layer 0: the fused epilogue of low's forward launch) and what = 2 is filled for fc layers and the
    network input only - here the fc head's, one sum per patch; the conv's backward launch masks and sums the cotangent it hands
    down in its epilogue (what = 3 of layer 0) and the layer above does the same for the conv's own (what = 3 of layer 1); the
    conv's forward epilogue sums its output (what = 11 of layer 1).  No layer here is a first conv under a pool or the conv under a
    fused fc head, so every tensor is stored beside its sums (tests/test_gpu_pool.py's rule)."""
    act = _copy(sess, m, 0, 0, n, (n,) + size + (c.Ci,))
    dlow = _copy(sess, m, 0, 1, n, (n,) + size + (c.Ci,))
    y = _copy(sess, m, 1, 0, n, (n,) + size + (c.Co,))
    dy = _copy(sess, m, 1, 1, n, (n,) + size + (c.Co,))
    z = _copy(sess, m, 2, 0, n, (n,) + size + (4,))
    assert np.count_nonzero(act) and np.count_nonzero(y) and np.count_nonzero(dy) and np.count_nonzero(dlow) and np.count_nonzero(z), tag
    _assert_sums(_copy(sess, m, 0, 11, n, (n,) + size), act, tag + ': sums of the input activation')
    _assert_sums(_copy(sess, m, 0, 3, n, (n,) + size), dlow, tag + ': sums of the cotangent handed down')
    _assert_sums(_copy(sess, m, 1, 3, n, (n,) + size), dy, tag + ': sums of the masked cotangent')
    _assert_sums(_copy(sess, m, 1, 11, n, (n,) + size), y, tag + ': sums of the output')
    _assert_sums(_copy(sess, m, 3, 2, n, (n, 1, 1, 1)), z.reshape(n, 1, 1, 1, -1), tag + ": sums of the fc head's input")


@pytest.mark.parametrize('c', BELOW, ids=[CASE_IDS[CASES.index(c)] for c in BELOW])
def test_forward_backward_and_gradients_below_a_conv(sess, c):
    import torch
    from nnal_amd import ref64
    assert EPS == ref64.DEFAULT_EPS
    size, k3, lo, nd = geometry(c.tag)
    ld, sk, in_shape = _model_of(c, 'below')
    cid = CASE_IDS[CASES.index(c)]
    seed = 400 + CASES.index(c)
    pars = netspec.he_init(ld, in_shape, seed=seed, bias_std=0.05)
    om64 = OracleModel(ld, in_shape, pars, dtype=torch.float64)
    x, chosen = first_stable_patches(om64, in_shape, seed + 1000, N, 4 * N, fragile_units)
    assert len(chosen) == N, 'too few patches without a fragile decision: pick another seed'
    print('%s: patches %r of stream %d, smallest key %.3e' % (c, chosen, seed + 1000, min(smallest_key(om64, x[[i]]) for i in range(N))))
    W, b = conv_ref._w5(pars['cv'][0]), np.asarray(pars['cv'][1]).reshape(-1)
    relu = 'A' in c.ops
    labels = (np.arange(N) % 2).astype(np.int32)
    t = _dev(sess, x)
    bad = []
    for route, (_, knob) in _routes(c).items():
        m = _mk_model(sess, ld, in_shape, sk, pars, c.mb, route)
        with _knob(sess, knob):
            for a, e in _passes(N, c.mb):
                n = e - a
                allv = tc._variants(labels[a:e])
                for vname in (list(allv) if route == 'default' else ['mode 0 class 1']):
                    kw = allv[vname]
                    rows = m.param_grads_device(t[a:e], n, **kw)[0].cpu().numpy()
                    tag = '%s | %s | %s | patches %d..%d' % (cid, route, vname, a, e - 1)
                    act = _copy(sess, m, 0, 0, n, (n,) + size + (c.Ci,))
                    y = _copy(sess, m, 1, 0, n, (n,) + size + (c.Co,))
                    dy = _copy(sess, m, 1, 1, n, (n,) + size + (c.Co,))
                    dlow = _copy(sess, m, 0, 1, n, (n,) + size + (c.Ci,))
                    assert np.count_nonzero(act) and np.count_nonzero(dy) and (act >= 0).all(), tag
                    # 2. forward on the device's own input activation
                    y64, y32 = (conv_ref.forward_torch(act, W, b, dt) for dt in (torch.float64, torch.float32))
                    if relu:
                        y64, y32 = np.maximum(y64, 0), np.maximum(y32, 0)
                        assert not dy[y == 0].any(), (tag, 'the cotangent of an ReLU layer is not masked by its own output')
                    _figure(bad, tag, 'output', y, y64, y32)
                    # 3. backward-data: the cotangent of the conv below, after its ReLU mask - zero wherever the activation is
                    assert not dlow[act == 0].any(), (tag, 'the cotangent below is not masked by the activation')
                    _figure(bad, tag, 'cotangent below', dlow, conv_ref.bwd_data64(dy, W, lo, act=act),
                            conv_ref.bwd_data_torch(dy, W, act, torch.float32))
                    # 4. the layer's rows of the parameter gradients
                    dW64, db64 = conv_ref.wgrad64(act, dy, k3, lo)
                    dW32, db32 = conv_ref.wgrad_torch(act, dy, W, torch.float32)
                    if rows.ndim == 1:
                        rows, dW64, db64, dW32, db32 = rows[None], dW64.sum(0, keepdims=True), db64.sum(0, keepdims=True), \
                            dW32.sum(0, keepdims=True), db32.sum(0, keepdims=True)
                    gW = np.stack([conv_ref._w5(m.unflatten(r)[2]) for r in rows])
                    gb = np.stack([m.unflatten(r)[3].reshape(-1) for r in rows])
                    _figure(bad, tag, 'dW', gW, dW64, dW32)
                    _figure(bad, tag, 'db', gb, db64, db32)
                if route == 'default':      # the fused-epilogue sums of a Fisher pass
                    m.fisher_device(t[a:e], n, None, 1e-3, want=('p1', 'g0', 'g1'))
                    _check_sums(sess, m, n, size, c, '%s | Fisher pass | patches %d..%d' % (cid, a, e - 1))
        m.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------ whole models
# name -> (layers, skips, input shape); the concat models take CONCAT_ROUTES
def _whole_models():
    out = OrderedDict()
    for tag, Ci, Co in (('k2', 8, 8), ('k234', 8, 16), ('k147', 12, 8), ('k5_2d', 8, 32)):
        out['%s-%dto%d' % (tag, Ci, Co)] = _model_of(Case(tag, Ci, Co, 'MA', 4, 'ig'), 'below')
    out['skipcat_k2'] = conv_ref.skip_concat([2, 2, 2]) + ((4, 5, 6, 1),)
    out['skipcat_k133'] = conv_ref.skip_concat([1, 3, 3]) + ((3, 5, 6, 1),)
    out['accum_k2'] = conv_ref.accumulating([2, 2, 2]) + ((4, 5, 6, 1),)
    out['accum_k133'] = conv_ref.accumulating([1, 3, 3]) + ((3, 5, 6, 1),)
    out['wide-k3_oddw-8to64'] = _model_of(Case('k3_oddw', 8, 64, 'MA', 4, 'wide'), 'below')
    return out


WHOLE = _whole_models()
_WHOLE = {}


def whole(name):
    """test_gpu_convt.whole_record of a model of WHOLE: computed once, shared, never modified."""
    if name not in _WHOLE:
        ld, sk, in_shape = WHOLE[name]
        _WHOLE[name] = tc.whole_record(name, ld, sk, in_shape, 700 + list(WHOLE).index(name), None)
    return _WHOLE[name]


def _mk(sess, d, route='default', **kw):
    return _mk_model(sess, d['ld'], d['in_shape'], d['sk'], d['pars'], 4, route, **kw)


def _routes_of(name):
    return CONCAT_ROUTES if d_is_concat(name) else ROUTES


def d_is_concat(name):
    return bool(WHOLE[name][1])


@pytest.mark.parametrize('name', list(WHOLE))
def test_whole_model_param_grads_vs_fp64(sess, name):
    tc.check_param_grads(sess, whole(name), _mk, ('default', 'no_v4_v3') + (('no_split',) if d_is_concat(name) else ()))


@pytest.mark.parametrize('name', list(WHOLE))
def test_whole_model_other_entry_points_vs_fp64(sess, name):
    tc.check_other_entry_points(sess, whole(name), _mk)


@pytest.mark.parametrize('name', list(WHOLE))
def test_whole_model_fisher_pass_vs_fp64(sess, name):
    tc.check_fisher_pass(sess, whole(name), _mk, _routes_of(name))


@pytest.mark.parametrize('name', list(WHOLE))
def test_device_weight_packing_same_bits(sess, name):
    tc.check_packing(sess, whole(name), _mk)

