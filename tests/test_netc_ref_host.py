"""tests/netc_ref.py on the CPU: the table of NET-C's fused launches, the integer model of check A and its exactness conditions per
launch, the per-launch references composed against the fp64 oracle, the host twin of the static cotangent bounds, the derived bar of
check B against a NumPy emulation of the fp16-pair / bf16-triple split (inside the bar; far outside it without the lo piece), and
the evidence that the checks of tests/test_gpu_netc_launches.py can fail: every mutation of every reference changes the integers
check A expects and exceeds the bar of check B.  No device."""
import numpy as np
import pytest

from oracle import netspec
from tests import netc_ref as R
from tests import pool_ref, side_ref

LO_MARGIN = 4.0      # "a wide margin": the emulation without the lo piece must exceed the bar at least this many times
_CACHE = {}


def integer():
    if 'int' not in _CACHE:
        _CACHE['int'] = R.integer_model()
    return _CACHE['int']


def floating():
    """he_init weights with bias_std = 0.05, two normal patches (one times 2^-20: per-patch scales differ), every tensor in fp64."""
    if 'float' not in _CACHE:
        ld, sk = R.net()
        P = netspec.he_init(ld, R.IN_SHAPE, seed=14, skips=sk, bias_std=0.05)
        x = np.random.RandomState(15).randn(2, *R.IN_SHAPE).astype(np.float32)
        x[1] *= np.float32(2.0 ** -20)
        _CACHE['float'] = (x, P, R.compose(x, P))
    return _CACHE['float']


def test_table():
    made = {(R.ENC1, 'out'), (R.ENC1, 'sign'), (R.POOL1, 'out'), (R.POOL1, 'argmax'), (R.POOL1, 'sign'), (R.FC, 'headsign')}      # direct.hip, c3d_fwd: input only
    for l in R.LAUNCHES:
        assert set(l.inputs) <= made, (l.name, set(l.inputs) - made)
        assert not set(l.outputs) & made, l.name
        made |= set(l.outputs)
        assert l.info[0] in R.ENGINE_INFO or l.name.startswith('bott'), l.name
        assert set(l.muts) <= set(R.MUTATIONS) | {'kchan'}
    assert sorted(R.ENGINE_INFO) == [7, 8, 9, 10, 11, 12, 13, 17, 19] and R.ENGINE_INFO[19] == 2
    assert len({l.file for l in R.LAUNCHES}) == 7      # f3d, t3d, d3d, t3d8b, c3d, e3d, igemm4
    x, P, T, _ = integer()
    for l in R.LAUNCHES:      # the references return exactly what the table lists (and c3d_bwd7 the partial that e3d completes)
        got = set(R.reference(l, T, P))
        assert set(l.outputs) <= got and got - set(l.outputs) <= {(R.ENC1, 'dsum_part'), (R.UP1, 'amax')}, (l.name, got)


def test_integer_model_meets_every_exactness_condition():
    """Check A owes equality on every launch of the table - the fused enc2 backward included: thinning bott, up1 and dec1 brings
    its static bound (3.3e7 at density 1/16) under 2^22."""
    x, P, T, dens = integer()
    assert not x[0].any() and x[1].all() and set(np.unique(x)) == {0., 1.}
    print('NETC_INT | densities / 256: %r' % dict(dens))
    for l in R.LAUNCHES:
        ints, sb, acc = R.exactness(l, T, P)
        print('NETC_INT | %s | integers %s | scale bound / 2^22 %.3g | accumulator / 2^24 %.3g' % (l.name, ints, sb, acc))
        assert ints and sb < 1. and acc < 1., (l.name, ints, sb, acc)
    for k, v in T.items():      # nothing of the table is trivially zero, and the ties and zeros check A lives on are there
        assert np.asarray(v)[1:].any(), k
    e2 = T[(R.ENC2, 'out')]
    win = e2.reshape(len(e2), 8, 2, 8, 2, 8, 2, 16)
    ties = (win == win.max(axis=(2, 4, 6), keepdims=True)).sum(axis=(2, 4, 6)) > 1
    assert ties[2].mean() > 0.1 and (e2[2] == 0).mean() > 0.1


def test_composed_references_reproduce_the_fp64_oracle():
    """side_ref.oracle_fields (OracleModel in fp64, autograd) of the integer model: activations, masked cotangents, dsum and S."""
    x, P, T, _ = integer()
    ld, sk = R.net()
    o = side_ref.oracle_fields(ld, sk, R.IN_SHAPE, P, x)
    det = o['det']
    for layer in range(8):
        np.testing.assert_array_equal(T[(layer, 'out')], det['out'][layer], err_msg=str(layer))
    pidx = {R.ENC1: 0, R.ENC2: 1, R.BOTT: 2, R.UP1: 3, R.DEC1: 4, R.UP2: 5, R.DEC2: 6}
    for layer in (R.BOTT, R.UP1, R.DEC1, R.UP2):
        np.testing.assert_array_equal(T[(layer, 'dout')], det['delta'][pidx[layer]].reshape(T[(layer, 'dout')].shape), err_msg=str(layer))
    np.testing.assert_array_equal(R.e3d_delta2(T), det['delta'][1].reshape(R.e3d_delta2(T).shape))
    geoms = side_ref.layers_of(ld, sk, R.IN_SHAPE)
    for layer in (R.ENC1, R.ENC2, R.BOTT, R.UP1, R.DEC1, R.UP2):
        g = geoms[pidx[layer]]
        dsum, asum, asum2 = o['fields'][pidx[layer]]
        np.testing.assert_array_equal(T[(layer, 'dsum')], dsum, err_msg=str(layer))
        mine = (x.reshape(len(x), 32, 32, 32).astype(np.float64) if layer == 0 else T[(g['src'], 'osum')] if (g['src'], 'osum') in T else T[(g['src'], 'out')].sum(-1),
                None if g['src2'] is None else T[(g['src2'], 'osum')])
        np.testing.assert_array_equal(mine[0], asum)
        assert (mine[1] is None) == (asum2 is None) and (asum2 is None or np.array_equal(mine[1], asum2))
        np.testing.assert_array_equal(side_ref.layer_S64(g, T[(layer, 'dsum')], mine[0], mine[1]), o['S'][:, pidx[layer]])
    assert np.abs(o['S'][:, :6]).max(0).min() > 0


def test_static_bounds_twin():
    """bwd_bounds bounds the true cotangents of both models, and is the chain of passes.hip: 1 at the logits, max |W0 - W1| below the
    head, every layer's own slice norm."""
    for x, P, T in (integer()[:3], floating()):
        b = R.bwd_bounds(P)
        assert b[R.FC] == 1. and abs(b[R.DEC2] / np.abs(R.head_wv(P)).max() - 1) < 1e-5
        for layer in (R.UP2, R.DEC1, R.UP1, R.BOTT, R.POOL2):
            assert b[layer] >= np.abs(T[(layer, 'dout')]).max() > 0, layer
        assert b[R.ENC2] >= np.abs(R.e3d_delta2(T)).max()
        l1, p0, p1 = R.bwd_l1_parts(P['dec1'][0], False, 16)
        assert max(p0, p1) == l1 and abs(b[R.UP1] / (p1 * b[R.DEC1]) - 1) < 1e-5
        assert abs(b[R.ENC2] / (p0 * b[R.DEC1] + b[R.POOL2]) - 1) < 1e-5


def _differs(l, T, P, mut, bar_of=None):
    """The outputs of l that its reference under `mut` changes - for the float model: by more than the bar of that output."""
    ref, got = R.reference(l, T, P), R.reference(l, T, P, mut)
    changed = []
    for k in l.outputs:
        a, b = np.asarray(ref[k]), np.asarray(got[k])
        if a.dtype != np.float64:
            if not np.array_equal(a, b):
                changed.append(k)
        elif bar_of is None:
            if not np.array_equal(a, b):
                changed.append(k)
        elif k in bar_of and np.any(np.abs(a - b) > bar_of[k]):
            changed.append(k)
    return changed


def _all_bars(l, T, P):
    """The bar of every float output of l as the GPU test applies it: output_bars, the sum bound on the reference's own terms for
    the channel sums, e3d_extra."""
    if l.name == 'e3d_bwd':
        b2, b0 = R.e3d_extra(T, P)
        return {(R.ENC2, 'dsum'): b2, (R.ENC1, 'dsum'): b0}
    ref = R.reference(l, T, P)
    out = dict(R.output_bars(l, R.bars(l, T, P), T))
    for (layer, what) in l.outputs:
        terms = {'osum': 'out', 'dsum': 'dout'}.get(what)
        if terms:
            t = np.abs(ref[(layer, terms)])
            out[(layer, what)] = pool_ref.sum_bound(t.sum(-1), t.shape[-1])
    return out


@pytest.mark.parametrize('l', R.LAUNCHES, ids=list(R.BY_NAME))
def test_every_mutation_changes_what_check_A_expects(l):
    x, P, T, _ = integer()
    for mut in l.muts:
        changed = _differs(l, T, P, mut)
        print('NETC_MUT_A | %s | %s | changes %r' % (l.name, mut, changed))
        assert changed, (l.name, mut)


@pytest.mark.parametrize('l', R.LAUNCHES, ids=list(R.BY_NAME))
def test_every_mutation_exceeds_the_bar_of_check_B(l):
    x, P, T = floating()
    bar_of = _all_bars(l, T, P)
    assert all(np.all(np.isfinite(b)) and np.all(b >= 0) for b in bar_of.values())
    for mut in l.muts:
        changed = _differs(l, T, P, mut, bar_of)
        print('NETC_MUT_B | %s | %s | exceeds the bar of %r' % (l.name, mut, changed))
        assert changed, (l.name, mut)


@pytest.mark.parametrize('l', R.LAUNCHES, ids=list(R.BY_NAME))
def test_split_emulation_inside_the_bar_and_far_outside_without_lo(l):
    """y of the launch from np.float16 pairs (f16_pair_split) / bf16 triples of its fp32 inputs stays inside the bar; without the
    input's lo piece - of a triple: its two lower pieces, so that in both forms only the leading piece is left - it exceeds the bar
    LO_MARGIN times somewhere.  (A triple without its THIRD piece alone is 2^-17 off per element, which is what M 2^-24 of the bar
    allows the accumulation: no derived bar can see that piece, only check A could, with integers above 2^16.)"""
    x, P, T = floating()
    y = R.lin(l.kind, np.asarray(l.core(T, P), np.float32), R.weights(l, P).astype(np.float32))
    bar = R.bars(l, T, P, y=y)
    e_in = np.abs(R.emulate(l, T, P) - y)
    e_lo = np.abs(R.emulate(l, T, P, drop_lo=True) - y)
    r_in, r_lo = float(np.max(e_in / np.maximum(bar, 1e-300))), float(np.max(e_lo / np.maximum(bar, 1e-300)))
    print('NETC_EMU | %s | %s | err %.3e | bar %.3e | err / bar %.3f | without lo: err / bar %.1f' % (l.name, l.split, e_in.max(), bar.max(), r_in, r_lo))
    assert bar.min() >= 0 and r_in <= 1., (l.name, r_in)
    assert r_lo >= LO_MARGIN, (l.name, r_lo)
