"""tests/scale_ref.py on the CPU: rescale leaves the network the same function (the fp32 oracle's logits bit for bit, the fp64
oracle's exactly), l1_chain bounds every activation of the fp64 oracle, tight_input attains the first layer's bound."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import netspec
from oracle.model import OracleModel
from tests import factored_ref, scale_ref


def _netc8():
    ld, sk = netspec.net_c()
    in_shape = (8, 8, 8, 1)
    return 'netc8', ld, sk, in_shape, netspec.he_init(ld, in_shape, seed=91, skips=sk, bias_std=0.05)


def _netb():
    ld = netspec.net_b_small(width=64)
    in_shape = (12, 12, 2)
    return 'netb', ld, [], in_shape, netspec.he_init(ld, in_shape, seed=92, bias_std=0.05)


MODELS = OrderedDict((m[0], m) for m in (_netc8(), _netb()))
CASES = [(name, layer) for name, m in MODELS.items() for layer in ['input'] + list(m[4])]


def test_consumers_of_netc():
    ld, sk = netspec.net_c()
    names = list(ld)
    got = {layer: [(names[i], part) for i, part in scale_ref.consumers(ld, sk, layer)] for layer in ['input', 'enc1', 'enc2', 'bott', 'up1', 'dec1', 'up2', 'dec2']}
    assert got == {'input': [('enc1', 'main')], 'enc1': [('enc2', 'main'), ('dec2', 'skip')], 'enc2': [('bott', 'main'), ('dec1', 'skip')],
                   'bott': [('up1', 'main')], 'up1': [('dec1', 'main')], 'dec1': [('up2', 'main')], 'up2': [('dec2', 'main')],
                   'dec2': [('fc', 'main')]}


@pytest.mark.parametrize('name,layer', CASES, ids=['%s-%s' % c for c in CASES])
def test_rescale_is_the_same_function(name, layer):
    _, ld, sk, in_shape, pars = MODELS[name]
    x = np.random.RandomState(7).randn(3, *in_shape).astype(np.float32)
    for dtype in (torch.float32, torch.float64):
        base = OracleModel(ld, in_shape, pars, skips=sk, dtype=dtype).forward(x)['output']
        assert np.isfinite(base).all() and np.abs(base).max() > 0
        for k in (-12, 12):
            p2, kx = scale_ref.rescale(pars, ld, sk, layer, k)
            changed = [n for n in pars if not np.array_equal(p2[n][0], pars[n][0]) or not np.array_equal(p2[n][1], pars[n][1])]
            assert changed, (layer, k)
            got = OracleModel(ld, in_shape, p2, skips=sk, dtype=dtype).forward(np.ldexp(x, kx))['output']
            assert got.dtype == base.dtype
            # (the head has no consumer: its own logits carry the factor)
            np.testing.assert_array_equal(got, np.ldexp(base, k) if layer == list(ld)[-1] else base, err_msg='%s %s k=%d %s' % (name, layer, k, dtype))


def test_rescale_refuses_what_leaves_the_normal_range():
    _, ld, sk, in_shape, pars = MODELS['netc8']
    with pytest.raises(AssertionError):
        scale_ref.rescale(pars, ld, sk, 'bott', 140)
    with pytest.raises(AssertionError):
        scale_ref.rescale(pars, ld, sk, 'bott', -125)


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('from_input', (0, 1))
def test_l1_chain_bounds_the_fp64_activations(name, from_input):
    _, ld, sk, in_shape, pars = MODELS[name]
    x = (37.0 * np.random.RandomState(8).randn(4, *in_shape)).astype(np.float32)
    x[1] *= 2.0 ** -9
    det = {}
    factored_ref.factored_unit_scores(OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64), x, details=det)
    acts = np.stack([np.abs(o).max(0) if o.ndim == 2 else np.abs(o).reshape(4, -1).max(1) for o in det['out']])
    amax = np.abs(x).reshape(4, -1).max(1) if from_input else acts[0]
    bound = scale_ref.l1_chain(pars, ld, sk, amax, from_input)
    assert bound.shape == acts.shape
    assert (bound >= acts).all(), (bound / acts).min()
    if not from_input:
        np.testing.assert_array_equal(bound[0], acts[0])
    # monotone in the measured maximum, and positively homogeneous where every bias is zero
    order = np.argsort(amax)
    assert (np.diff(bound[:, order], axis=1) >= 0).all()
    p0 = OrderedDict((n, [W, np.zeros_like(b)]) for n, (W, b) in pars.items())
    np.testing.assert_array_equal(scale_ref.l1_chain(p0, ld, sk, np.ldexp(amax, 5), from_input), np.ldexp(scale_ref.l1_chain(p0, ld, sk, amax, from_input), 5))


def test_conv_norms_against_loops():
    rs = np.random.RandomState(9)
    W = rs.randn(2, 3, 4, 5).astype(np.float32)
    b = rs.randn(5).astype(np.float32)
    bwd, l1, bm = scale_ref.conv_norms(W, b, False)
    assert bwd == max(np.abs(W[:, :, ci, :].astype(np.float64)).sum() for ci in range(4))
    assert l1 == np.float32(max(np.abs(W[..., co].astype(np.float64)).sum() for co in range(5)) * (1 + 1e-6))
    assert bm == np.float32(np.abs(b.astype(np.float64)).max() * (1 + 1e-6))
    bt = rs.randn(4).astype(np.float32)
    bwd, l1, _ = scale_ref.conv_norms(W, bt, True)          # conv_transpose: [k.., co, ci]
    assert bwd == max(np.abs(W[..., ci].astype(np.float64)).sum() for ci in range(5))
    assert l1 == np.float32(max(np.abs(W[:, :, co, :].astype(np.float64)).sum() for co in range(4)) * (1 + 1e-6))


@pytest.mark.parametrize('name', list(MODELS))
@pytest.mark.parametrize('amax', (1.0, 2.0 ** -9, 37.0))
def test_tight_input_attains_the_first_bound(name, amax):
    _, ld, sk, in_shape, pars = MODELS[name]
    first = list(pars)[0]
    W, b = pars[first]
    x, voxel, co = scale_ref.tight_input(W, b, amax, in_shape)
    assert np.abs(x).max() == np.float32(amax)
    det = {}
    factored_ref.factored_unit_scores(OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64), x[None], details=det)
    pre = det['pre'][0][(0,) + voxel + (co,)]
    l1 = np.abs(W[..., co].astype(np.float64)).sum()
    want = float(np.float32(amax)) * l1 + abs(float(b[co]))
    assert abs(abs(pre) - want) <= 1e-12 * want and np.sign(pre) == (-1 if b[co] < 0 else 1)
    bound = scale_ref.l1_chain(pars, ld, sk, [amax], 1)[0, 0]
    assert bound >= abs(pre) and bound <= (abs(pre) + np.abs(b).max() - abs(float(b[co]))) * (1 + 3e-6)
