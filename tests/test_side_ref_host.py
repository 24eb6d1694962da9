"""tests/side_ref.py against the fp64 oracle, and its case tables against its own restatement of the dispatch (CPU only).

The references of tests/test_gpu_side_sums.py are themselves checked here: the box-filter dot products written from the definition
must reproduce the per-layer sums of tests.factored_ref on the oracle's fp64 activations and cotangents (conv, conv_transpose, fc
and a concat consumer with a second producer; float and integer models), finalize64 must reproduce factored_ref.fisher_from_unit,
every case must reach the kernel form it claims, every integer model must be exact, and leaving one border tap out of the
reference must change the integer some exact case of every form is held to."""
import numpy as np
import pytest

from tests import factored_ref, side_ref
from tests.side_ref import CASES, CASE_IDS, FORMS


def _check_layers(rec, o, tag):
    ld, sk, in_shape, x, pars, _, geoms = rec
    assert o['S'].shape == (len(x), len(geoms))
    for g, (dsum, asum, asum2) in zip(geoms, o['fields']):
        S = side_ref.layer_S64(g, dsum, asum, asum2)
        tol = 1e-13 * side_ref.layer_abs(g, dsum, asum, asum2) + 1e-300
        err = np.abs(S - o['S'][:, g['pidx']])
        assert (err <= tol).all(), (tag, g['name'], err.max(), tol.min())
        assert (g['src2'] is not None) == (asum2 is not None)


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_boxdot_reproduces_factored_ref_on_float_models(c):
    rec = side_ref.float_case(c)
    ld, sk, in_shape, x, pars = rec[:5]
    o = side_ref.oracle_fields(ld, sk, in_shape, pars, x)
    assert np.abs(o['S'][:, :-1]).min() > 0
    _check_layers(rec, o, c.tag)


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_integer_models_are_exact_and_reproduce_factored_ref(c):
    """The builder's own assertion, restated: integers everywhere, every absolute accumulation below the bounds, mixed signs in
    the head conv, patch 0 all zero (S = 0 on it) and patch 1 all one."""
    rec = side_ref.integer_case(c)
    ld, sk, in_shape, x, pars, o, geoms = rec
    o2, worst, share = side_ref.exactness(ld, sk, in_shape, pars, x)
    print('%s: densities %r, largest bound / limit %.3f, positive share of the head conv %.2f' % (c.tag, o['dens'], worst, share))
    assert worst < 1. and 0.2 <= share <= 0.8
    assert not x[0].any() and x[1].all() and set(np.unique(x)) == {0., 1.}
    assert not o['S'][0].any() and np.abs(o['S'][:, :-1]).max(0).all()
    for name, (W, b) in pars.items():
        assert np.all(W == np.round(W)) and np.abs(W).max() <= (2 if name == list(pars)[-1] else 1)
        assert not np.any(b) or name == list(pars)[-1]
    _check_layers(rec, o, c.tag)
    np.testing.assert_array_equal(o2['S'], o['S'])


def test_concat_consumers_have_two_producers():
    for c in CASES:
        geoms = side_ref.layers_of(*side_ref.model_of(c))
        two = [g['name'] for g in geoms if g['src2'] is not None]
        assert two == (['c3'] if c.kind == 'concat' else []), (c.tag, two)
    assert {c.kind for c in CASES} == {'conv', 'convT', 'concat'}


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_case_reaches_the_form_it_claims(c):
    g = side_ref.under_test(c)
    assert (g['form'], g['nslab'], g['planes']) == (c.form, c.nslab, c.planes), (c.tag, g['form'], g['nslab'], g['planes'])


def test_every_form_is_reached_and_the_table_is_as_the_dispatch_says():
    assert {c.form for c in CASES} == set(FORMS)
    ef = side_ref.expected_form
    # the thresholds of the dispatch, one step to either side
    assert ef('conv', (8, 8, 8), [3, 3, 3])[0] == 'col<3,3,3>' and ef('conv', (7, 8, 9), [3, 3, 3])[0] == 'plain'       # 512 and 504 voxels
    assert ef('conv', (1, 112, 112), [1, 5, 5]) == ('plain', 13, None) and ef('conv', (1, 104, 104), [1, 5, 5])[0] == 'col<1,5,5>'
    assert ef('conv', (4, 4, 512), [3, 3, 3]) == ('col<3,3,3>', 4, 1) and side_ref._tile_bytes(2, 4, 512, [3, 3, 3]) > side_ref.LDS_LIMIT
    assert ef('conv', (12, 20, 20), [3, 3, 3]) == ('col<3,3,3>', 2, 10)
    assert ef('conv', (8, 9, 9), [3, 3, 3])[0] == 'lds' and ef('conv', (8, 8, 8), [1, 3, 3])[0] == 'col<1,3,3>'
    assert ef('conv_transpose', (6, 6, 6), [3, 3, 3], [2, 2, 2]) == ('convT_out<3,2>', 1, 12)
    assert ef('conv_transpose', (8, 10, 10), [3, 3, 3], [2, 2, 2]) == ('convT_out<3,2>', 2, 10)
    # an odd input width leaves output rows of 2 mod 4 points: the output-side form walks them in groups of four
    for size in ((4, 4, 3), (2, 2, 5)):
        assert ef('conv_transpose', size, [3, 3, 3], [2, 2, 2])[0] == 'convT_plain' and np.prod(size) % 4 == 0
    assert ef('conv_transpose', (1, 4, 5), [1, 3, 3], [1, 2, 2])[0] == 'convT_plain' and ef('conv_transpose', (1, 4, 6), [1, 3, 3], [1, 2, 2])[0] == 'convT_out<3,2>'
    assert ef('conv_transpose', (3, 5, 6), [3, 3, 3], [2, 2, 2])[0] == 'convT_plain'      # 90 voxels: not a multiple of 4
    assert ef('conv_transpose', (4, 4, 4), [2, 2, 2], [2, 2, 2])[0] == 'convT_plain'
    assert ef('fc', (1, 1, 1), [1, 1, 1]) == ('plain', 1, None)
    assert sorted(side_ref.ODD_WIDTH) == ['tplain-oddw-2x2x5', 'tplain-oddw-4x4x3', 'tplain-oddw-4x5-2d']


def _corner_drops(g):
    """(voxel, tap) pairs: the 8 corners of the reduction grid, each with the tap that reaches furthest into the volume."""
    out = []
    for c in np.ndindex(2, 2, 2):
        x = tuple((n - 1) if v else 0 for v, n in zip(c, g['grid']))
        if g['type'] == 'conv_transpose':
            t = tuple(0 if v else k - 1 for v, k in zip(c, g['k3']))
            p = tuple(s * q + tt - l for s, q, tt, l in zip(g['s3'], x, t, g['lo']))
            ok = all(0 <= v < n for v, n in zip(p, g['dgrid']))
        else:
            t = tuple(0 if v else k - 1 for v, k in zip(c, g['k3']))
            ok = all(0 <= q + tt - l < n for q, tt, l, n in zip(x, t, g['lo'], g['grid']))
        if ok:
            out.append((x, t))
    return out


def test_one_dropped_border_tap_changes_an_exact_case_of_every_form():
    """What makes check A of tests/test_gpu_side_sums.py a test of single taps: with a tap of a corner voxel left out of the
    reference, the integer S of the layer under test changes on some patch, for some exact case of every form."""
    hit = {f: [] for f in FORMS}
    for c in CASES:
        ld, sk, in_shape, x, pars, o, geoms = side_ref.integer_case(c)
        g = side_ref.under_test(c)
        dsum, asum, asum2 = o['fields'][g['pidx']]
        S = side_ref.layer_S64(g, dsum, asum, asum2)
        for drop in _corner_drops(g):
            S2 = side_ref.layer_S64(g, dsum, asum, asum2, drop=drop)
            if np.any(S2 != S):
                assert np.all(S2 == np.round(S2)) and np.abs(S2 - S).max() >= 1.
                hit[c.form].append((c.tag, drop))
    for f in FORMS:
        print('%s: %d (case, corner tap) pairs change S' % (f, len(hit[f])))
        assert hit[f], f


def test_finalize64_reproduces_fisher_from_unit():
    rs = np.random.RandomState(5)
    N, L = 40, 6
    S = rs.randn(N, L) * 100.
    sizes = rs.randint(10, 5000, size=L)
    p1 = rs.uniform(0.02, 0.98, size=N).astype(np.float32)
    p0 = (1. - p1.astype(np.float64)).astype(np.float32)
    g0, g1, A = factored_ref.fisher_from_unit(p1.astype(np.float64), S, sizes, 1e-3)
    f = side_ref.finalize64(S, p0, p1, sizes, 1e-3)
    # the rounding of p1 s to fp32 (2^-24 relative), of p0 = 1 - p1 to fp32 (2^-25 absolute on p0 >= 0.02) and their products
    np.testing.assert_allclose(f['g0'], g0, rtol=2 ** -23, atol=0)
    np.testing.assert_allclose(f['g1'], g1, rtol=2 ** -21, atol=0)
    assert (np.abs(f['A'] - A) <= 2 ** -19 * f['A_abs']).all()
    np.testing.assert_allclose(f['trace'], A[:, np.arange(L), np.arange(L)].sum(1), rtol=2 ** -19)
    np.testing.assert_allclose(f['Asum'], f['A'].sum(0), rtol=0, atol=0)
    assert not f['low'].any() and not f['high'].any()


def test_finalize64_saturation_branches():
    """p < 1e-6 on the fp32 value as a double: p = 0 and g1 = 0; p > 1 - 1e-6: p = 1 and g0 = 0; p1_branch decides, p1f scales."""
    pb = np.array(side_ref.P1_BRANCH, np.float32)
    N, L = len(pb), 3
    S = np.arange(1, N * L + 1, dtype=np.float64).reshape(N, L)
    p1 = np.full(N, 0.25, np.float32)
    f = side_ref.finalize64(S, 1 - p1, p1, [2., 4., 8.], 0.5, p1_branch=pb)
    low = pb.astype(np.float64) < 1e-6
    high = pb.astype(np.float64) > 1. - 1e-6
    assert low.tolist() == [True, True, True, False, False, False, False]      # float32(1e-6) lies below 1e-6
    assert high[-2:].all() and not high[:4].any()
    assert not f['g1'][low].any() and f['g1'][~low].all() and not f['g0'][high].any() and f['g0'][~high].all()
    for n in range(N):
        p = 0. if low[n] else 1. if high[n] else float(pb[n])
        A = (1 - p) * np.outer(f['g0'][n], f['g0'][n]) + p * np.outer(f['g1'][n], f['g1'][n]) + 0.5 * np.eye(L)
        np.testing.assert_allclose(f['A'][n], A, rtol=1e-15)
    plain = side_ref.finalize64(S, 1 - p1, p1, [2., 4., 8.], 0.5)
    np.testing.assert_array_equal(plain['g0'], 0.25 * S / np.array([2., 4., 8.]))
    np.testing.assert_array_equal(plain['g1'], -0.75 * S / np.array([2., 4., 8.]))


def test_finalisation_model_is_exact_with_moderate_posteriors():
    ld, sk, in_shape, x, pars, o = side_ref.fin_case(max(side_ref.FIN_N))
    _, worst, share = side_ref.exactness(ld, sk, in_shape, pars, x, side_ref.FIN_SCALE)
    assert worst < 1. and 0.2 <= share <= 0.8
    p1 = o['p'][1]
    print('finalisation model: p1 in [%.3g, %.3g], %d of %d within (0.05, 0.95)' % (p1.min(), p1.max(), ((p1 > .05) & (p1 < .95)).sum(), len(p1)))
    assert ((p1 > 0.05) & (p1 < 0.95)).mean() > 0.5
    S = o['S'] / side_ref.FIN_SCALE
    assert np.all(S == np.round(S)) and np.abs(S).max() < side_ref.EXACT_BOUND
