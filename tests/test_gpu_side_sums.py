"""The Fisher pass's box-filter dot products and its finalisation, kernel by kernel against tests/side_ref.py (GPU box).

A Fisher pass reduces two channel-sum fields per parameterised layer to one number per patch, the unit-cotangent layer sum S[n, t]
(k_boxdot_conv / k_boxdot_convT of csrc/kernels.hip: seven kernel forms chosen by geometry alone), and fisher_finalize_kernel /
reduce_Asum_kernel turn S and the posteriors into g0, g1, A, trace and Asum.  The rest of the suite sees these kernels through
whole-model scores whose bars hide a wrong voxel; here every form is held to a reference of its own.

Models (tests/side_ref.py: CASES, model_of): conv(8, 3^nd) -> layer under test -> conv(4, 1x1) -> fc(2), and the skip-concat model of
tests/conv_ref.py whose consumer reads two producers (asum2), with the split and with the interleaved concat (ALQ_NO_SPLIT, the only
switch set here).  Each case names the smallest volume that reaches its form; tests/test_side_ref_host.py holds the table to
side_ref.expected_form.  EVERY parameterised layer of every model is checked, not only the one the case is named after - the low
conv, the 1x1 conv and the fc head bring further volumes and windows - and each check names the form side_ref expects the layer
to take.  After one Fisher pass the fields are read with alq_model_debug_copy: dsum (what = 3), the input sums (what = 2 of an fc
layer, what = 11 of the producers, the caller's x for the one-channel first layer) and S (what = 4).  N = 5 patches under
max_batch = 4: two passes, the second of one patch.

Check A, exact.  Integer models (side_ref.integer_model: x in {0, 1}, weights in {-1, 0, 1}, zero conv biases, a head in [-2, 2];
every activation, cotangent, channel sum and box sum an integer whose absolute accumulation stays below 2^24 - asserted on the CPU).
The copied fields must EQUAL the oracle's fp64 fields (a failure there belongs to a layer engine, not to this file), then S must
EQUAL the integer of side_ref on every layer of every patch, the all-zero patch included.  tests/test_side_ref_host.py shows that
one border tap left out changes that integer for some exact case of every form.  NOT_EXACT lists the cases a route cannot make
exact (none).

Check B, float.  he_init weights with bias_std = 0.05 and normal x; the fields read from the device are taken as given and
S64 = side_ref's sum over them in fp64.  The bar is derived, not measured:

    |S_dev - S64| <= 2^-24 [(M - 1) abs_terms + |S64|] x 1.01

A box is a sum of at most M fp32 terms (side_ref.additions: the taps, twice as many with a second source - the rounding of
asum + asum2 counts as one addition per tap -; for a conv_transpose also the prod(s) terms of the own-sum and the one rounding of
asum + asum2), so in any order its error is at most (M - 1) 2^-24 times the sum of the absolute terms to first order; the factor
dsum, the + 1, the product and the sum over voxels are fp64 (2^-53: nothing beside 2^-24).  abs_terms is the same reduction over
absolute values.  What = 4 returns S as a float: 2^-24 |S64|.  1.01 covers the second-order terms (M 2^-24 < 1e-5) and the fp64
work.  The volumes are at most 16^3-scale so that one dropped tap (about 1 / voxels of abs_terms) exceeds the bar.  Every figure
is printed (SIDE_FIG) before it is asserted.

Finalisation.  One tiny integer model (4x4x4 input; its head's integers times 2^-8, so that the logits are exact AND the posteriors
moderate) at N in {1, 63, 64, 65, 129} under max_batch = N: Apart spans one, two and three blocks.  S must equal the oracle's; g0,
g1, A, trace and Asum are held to side_ref.finalize64 of the device's own S and posteriors.  The Fisher pass returns p1 only; p0 is
taken from a forward pass over the same patches where its p1 equals the Fisher pass's bit for bit (the logits are exact, so it
does): then g0 and g1 must EQUAL the reference.  Otherwise p0 = float32(1 - p1) and g is held to 2 ulp of fp32.  A, trace and Asum
are formed from the kernel's own g0, g1 and held to 1e-14 x the sum of their absolute terms (fp64 products whose contraction
into fused multiply-adds and whose summation order are the kernel's).  The same model once more with a p1_in vector on both sides
of both saturation thresholds, and a model of 15 tiny fc layers and the head: L = 16, L L = 256 = reduce_Asum_kernel's block, every
entry of Asum checked (L = 17 is refused: tests/test_model_plan_host.py).

FORMS_UNREACHABLE names what no case reaches.
"""
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import side_ref  # noqa: E402
from tests.side_ref import CASES, CASE_IDS, FORMS, N  # noqa: E402
from tests.test_gpu_convt import _copy, _dev, _make, _passes  # noqa: E402

MB = 4
DIAG = 1e-3
# case tag -> why a route cannot make it exact (such a case is held to check B only).  At most a quarter of the cases, and no
# form with all of its cases here (test_tables).
NOT_EXACT = OrderedDict()
# what no case reaches, and why
FORMS_UNREACHABLE = OrderedDict([
    ('boxdot_conv_lds_kernel on a column window with W % 4 == 0 (the al16 fallback of k_boxdot_conv)',
     'taken only when dsum, asum or asum2 is not 16-byte aligned; the model allocates every field itself and torch hands out '
     'aligned x - a test must not offset x to force it'),
    ('the scalar loads of boxdot_convT_out_kernel (al == false)',
     'the same: only for a field that is not 16-byte aligned; every per-patch stride is a multiple of 4 floats (ivox % 4 == 0)'),
])


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _fields(sess, m, geoms, x, n):
    """Per parameterised layer (dsum, asum, asum2) of the last Fisher pass as [n, D, H, W] arrays, and S [n, L]."""
    out = []
    for g in geoms:
        dsum = _copy(sess, m, g['layer'], 3, n, (n,) + g['dgrid'])
        if g['type'] == 'fc':
            out.append((dsum, _copy(sess, m, g['layer'], 2, n, (n, 1, 1, 1)), None))
            continue
        assert g['layer'] > 0 or x.shape[-1] == 1
        asum = x.reshape((n,) + g['grid']) if g['layer'] == 0 else _copy(sess, m, g['src'], 11, n, (n,) + g['grid'])
        asum2 = None if g['src2'] is None else _copy(sess, m, g['src2'], 11, n, (n,) + g['grid'])
        out.append((dsum, asum, asum2))
    return out, _copy(sess, m, 0, 4, n, (n, len(geoms)))


def _run(sess, c, rec):
    """One Fisher pass per group of MB patches; yields (first patch, end, fields, S) of each."""
    ld, sk, in_shape, x, pars, _, geoms = rec
    t = _dev(sess, x)
    m = _make(sess, ld, in_shape, sk, pars, MB, extra_env=c.env)
    assert m.L == len(geoms)
    try:
        for a, e in _passes(N, MB):
            m.fisher_device(t[a:e], e - a, None, DIAG, want=('p1',))
            yield (a, e) + _fields(sess, m, geoms, x[a:e], e - a)
    finally:
        m.close()


def test_tables():
    assert set(NOT_EXACT) <= set(CASE_IDS) and 4 * len(NOT_EXACT) <= len(CASES)
    for f in FORMS:
        assert any(c.form == f and c.tag not in NOT_EXACT for c in CASES), f
    assert len(FORMS_UNREACHABLE) == 2
    for tag in side_ref.ODD_WIDTH:
        assert tag not in NOT_EXACT


# ------------------------------------------------------------------------------------------ A. exact
@pytest.mark.parametrize('c', [c for c in CASES if c.tag not in NOT_EXACT], ids=[t for t in CASE_IDS if t not in NOT_EXACT])
def test_S_equals_the_integer_of_the_definition(sess, c):
    rec = side_ref.integer_case(c)
    o, geoms = rec[5], rec[6]
    passes = 0
    for a, e, fields, S in _run(sess, c, rec):
        for g, got, want in zip(geoms, fields, o['fields']):
            for what, gv, wv in zip(('dsum', 'asum', 'asum2'), got, want):
                assert (gv is None) == (wv is None)
                if gv is not None:
                    bad = np.argwhere(gv.astype(np.float64) != wv[a:e])
                    assert bad.size == 0, ('%s, layer %s, patches %d..%d: the engine-made field %s differs from the fp64 oracle in %d places, '
                                           'first at %r: %r != %r' % (c.tag, g['name'], a, e - 1, what, len(bad), tuple(bad[0]),
                                                                      gv[tuple(bad[0])], wv[a:e][tuple(bad[0])]))
        for g, (dsum, asum, asum2) in zip(geoms, fields):
            want = side_ref.layer_S64(g, dsum, asum, asum2)
            np.testing.assert_array_equal(want, o['S'][a:e, g['pidx']])
            assert np.all(want == np.round(want)) and np.abs(want).max() < side_ref.EXACT_BOUND
            got = S[:, g['pidx']].astype(np.float64)
            print('SIDE_EXACT | %s | %s | %s, %d slab(s) | patches %d..%d | S %r' % (c.tag, g['name'], g['form'], g['nslab'], a, e - 1, got.tolist()))
            assert np.array_equal(got, want), ('%s, layer %s (%s, %d slabs), patches %d..%d: S %r != %r'
                                               % (c.tag, g['name'], g['form'], g['nslab'], a, e - 1, got.tolist(), want.tolist()))
        if a == 0:
            assert not S[0].any()      # the all-zero patch
        passes += 1
    assert passes == 2


# ------------------------------------------------------------------------------------------ B. float
@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_S_within_the_fp32_bar_of_fp64(sess, c):
    rec = side_ref.float_case(c)
    geoms = rec[6]
    bad = []
    for a, e, fields, S in _run(sess, c, rec):
        for g, (dsum, asum, asum2) in zip(geoms, fields):
            assert g['type'] == 'fc' or (np.count_nonzero(dsum) and np.count_nonzero(asum)), (c.tag, g['name'])      # (the head's two cotangents cancel)
            S64 = side_ref.layer_S64(g, dsum, asum, asum2)
            M = side_ref.additions(g, asum2 is not None)
            bar = 2. ** -24 * ((M - 1) * side_ref.layer_abs(g, dsum, asum, asum2) + np.abs(S64)) * 1.01
            err = np.abs(S[:, g['pidx']].astype(np.float64) - S64)
            ratio = float(np.max(err / np.maximum(bar, 1e-300)))
            print('SIDE_FIG | %s | %s | %s | M %d | patches %d..%d | err %.3e | bar %.3e | err / bar %.3f'
                  % (c.tag, g['name'], g['form'], M, a, e - 1, err.max(), bar[np.argmax(err / np.maximum(bar, 1e-300))], ratio))
            if not np.all(err <= bar):
                bad.append((c.tag, g['name'], g['form'], a, err.tolist(), bar.tolist()))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ finalisation
def _posteriors(sess, m, t, n, p1):
    """(p0 as fp32, whether it is the kernel's own): from a forward pass where its p1 equals the Fisher pass's bit for bit."""
    post = m.forward_device(t, n)[0].cpu().numpy()
    if np.array_equal(post[1].view(np.uint32), p1.view(np.uint32)):
        return post[0], True
    return (1. - p1.astype(np.float64)).astype(np.float32), False


def _check_finalisation(tag, r, S, p0, own_p0, sizes, exact_S, p1_branch=None):
    p1 = r['p1']
    ref = side_ref.finalize64(S, p0, p1, sizes, DIAG, p1_branch)
    for key in ('g0', 'g1'):
        err = np.abs(r[key] - ref[key])
        if exact_S and (key == 'g0' or own_p0):
            print('FIN | %s | %s: max |dev - ref| %.3e (must be 0)' % (tag, key, err.max()))
            assert np.array_equal(r[key], ref[key]), (tag, key, err.max())
        else:
            bar = 2 * 2. ** -23 * np.abs(ref[key])
            print('FIN | %s | %s: max err / (2 ulp of fp32) %.3f' % (tag, key, np.max(err / np.maximum(bar, 1e-300))))
            assert (err <= bar).all(), (tag, key, err.max())
    own = side_ref.finalize64(S, p0, p1, sizes, DIAG, p1_branch, g=(r['g0'], r['g1']))
    for key in ('A', 'trace', 'Asum'):
        err, bar = np.abs(r[key] - own[key]), 1e-14 * own[key + '_abs']
        print('FIN | %s | %s: max err / (1e-14 sum |terms|) %.3f' % (tag, key, np.max(err / np.maximum(bar, 1e-300))))
        assert r[key].shape == own[key].shape and bar.max() > 0 and (err <= bar).all(), (tag, key, err.max())
    return ref


def _fisher(sess, m, t, n, p1_in=None):
    r = m.fisher_device(t, n, p1_in, DIAG, want=('p1', 'g0', 'g1', 'A', 'trace', 'Asum'))
    return {k: r[k].cpu().numpy() for k in ('p1', 'g0', 'g1', 'A', 'trace', 'Asum')}


@pytest.mark.parametrize('n', side_ref.FIN_N)
def test_finalize_and_Asum(sess, n):
    ld, sk, in_shape, x, pars, o = side_ref.fin_case(n)
    t = _dev(sess, x)
    m = _make(sess, ld, in_shape, sk, pars, n)
    r = _fisher(sess, m, t, n)
    S = _copy(sess, m, 0, 4, n, (n, m.L)).astype(np.float64)
    p0, own_p0 = _posteriors(sess, m, t, n, r['p1'])
    m.close()
    np.testing.assert_array_equal(S, o['S'][:n])
    assert np.abs(r['p1'].astype(np.float64) - o['p'][1][:n]).max() <= 1e-6
    print('FIN | N %d: %d block(s) of Apart, p0 from the forward pass: %s' % (n, -(-n // 64), own_p0))
    _check_finalisation('N %d' % n, r, S, p0, own_p0, o['sizes'], True)


def test_finalize_saturation_branches_and_p1_in(sess):
    pb = np.array(side_ref.P1_BRANCH, np.float32)
    n = len(pb)
    ld, sk, in_shape, x, pars, o = side_ref.fin_case(n)
    t = _dev(sess, x)
    m = _make(sess, ld, in_shape, sk, pars, n)
    r = _fisher(sess, m, t, n, sess.to_device(pb, sess.torch.float32))
    S = _copy(sess, m, 0, 4, n, (n, m.L)).astype(np.float64)
    p0, own_p0 = _posteriors(sess, m, t, n, r['p1'])
    m.close()
    np.testing.assert_array_equal(S, o['S'][:n])
    ref = _check_finalisation('p1_in', r, S, p0, own_p0, o['sizes'], True, p1_branch=pb)
    assert ref['low'].tolist() == [True, True, True, False, False, False, False] and ref['high'].tolist()[-2:] == [True, True]
    assert not r['g1'][ref['low']].any() and not r['g0'][ref['high']].any()
    live = S[:, :-1].any(axis=1)      # (patch 0 is all zero)
    assert r['g0'][~ref['high'] & live].any(axis=1).all() and r['g1'][~ref['low'] & live].any(axis=1).all()


def test_Asum_of_sixteen_layers(sess):
    """L = 16: Asum has exactly the 256 entries of reduce_Asum_kernel's block; 65 patches are two blocks of Apart.  Float weights:
    what = 4 returns S rounded to fp32, so g is held to 2 ulp of fp32; A, trace and Asum follow from the kernel's own g."""
    ld, sk, in_shape, x, pars = side_ref.l16_case()
    n = len(x)
    t = _dev(sess, x)
    m = _make(sess, ld, in_shape, sk, pars, n)
    assert m.L == 16
    r = _fisher(sess, m, t, n)
    S = _copy(sess, m, 0, 4, n, (n, 16)).astype(np.float64)
    p0, own_p0 = _posteriors(sess, m, t, n, r['p1'])
    m.close()
    assert np.count_nonzero(S[:, :15].any(axis=0)) == 15 and not S[:, 15].any()
    sizes = [np.asarray(W).size + np.asarray(b).size for W, b in pars.values()]
    print('FIN | L16: p0 from the forward pass: %s' % own_p0)
    _check_finalisation('L16', r, S, p0, own_p0, sizes, False)
    assert r['Asum'].shape == (16, 16) and np.count_nonzero(r['Asum'][:15, :15]) == 225
