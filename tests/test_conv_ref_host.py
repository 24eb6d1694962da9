"""tests/conv_ref.py against fp64 autograd and against the loops of the definition (CPU): the references tests/test_gpu_conv.py
holds the conv kernels to are checked here without a device, so a restatement that agreed with the kernels only by sharing their
mistake fails in this file."""
import numpy as np
import pytest
import torch

from oracle import tfops
from tests import conv_ref

TAGS = list(conv_ref.GEOMETRIES)


def _draw(tag, Ci, Co, n=2, seed=0):
    size, k3, lo, nd = conv_ref.geometry(tag)
    if tag == 'k3_tiles':      # the loops of the definition over a corner of the tiled map: the same k and lo
        size = (1, 7, 9)
    rs = np.random.RandomState(seed + TAGS.index(tag))
    a = rs.randn(n, *size, Ci)
    a = np.maximum(a, 0.)      # a ReLU output: about half of it is zero
    W = rs.randn(*k3, Ci, Co)
    b = rs.randn(Co)
    dy = rs.randn(n, *size, Co)
    return size, k3, lo, nd, a, W, b, dy


@pytest.mark.parametrize('tag', TAGS)
def test_lo_of_the_table(tag):
    """same_pads at stride 1: lo = (k - 1) // 2 before, k - 1 - lo behind, whatever the size - the table's own column."""
    g = conv_ref.GEOMETRIES[tag]
    size, k3, lo, nd = conv_ref.geometry(tag)
    assert lo == g['lo'] == [(k - 1) // 2 for k in k3]
    assert nd == len(g['k']) and k3[:3 - nd] == [1] * (3 - nd) and (nd == 3 or size[0] == 1)
    for n, k, l in zip(size, k3, lo):
        assert tfops.same_pads(n, k, 1) == (n, l, k - 1 - l)
    assert int(np.prod(k3)) <= conv_ref.MAX_TAPS
    if tag not in ('k3_tiles',):      # ragged: never a cube
        assert len(set(size[3 - nd:])) > 1


def test_the_table_covers_what_it_says():
    taps = {t: int(np.prod(conv_ref.geometry(t)[1])) for t in TAGS}
    assert taps['k147'] == 28 == conv_ref.MAX_TAPS and taps['k5_2d'] == taps['k155_3d'] == 25 and taps['k234'] == 24 and taps['k1'] == 1
    assert conv_ref.geometry('k5_2d')[0][0] == 1 and conv_ref.geometry('k155_3d')[0][0] == 2
    assert conv_ref.geometry('k3_ragged')[0][2] % 2 == 0 and conv_ref.geometry('k3_oddw')[0][2] % 2 == 1
    even = [t for t in TAGS if any(k % 2 == 0 for k in conv_ref.geometry(t)[1])]
    assert even == ['k2', 'k4_2d', 'k234', 'k147']
    for tag, g in conv_ref.REFUSED.items():
        taps_r = int(np.prod(g['k']))
        if 'taps unsupported' in g['text']:
            assert taps_r > conv_ref.MAX_TAPS and g['text'] == 'igemm: %d taps unsupported' % taps_r
        if 'single-chunk' in g['text']:
            assert g['Ci'] % 8 and taps_r * g['Ci'] > conv_ref.MAXK_SMALL
    for tag, Ci in conv_ref.SMALLC_LIMIT:
        K = int(np.prod(conv_ref.geometry(tag)[1])) * Ci
        assert Ci % 8 and K <= conv_ref.MAXK_SMALL and K in (999, 972)


@pytest.mark.parametrize('tag', TAGS)
def test_conv_ref_from_the_definition_vs_autograd(tag):
    size, k3, lo, nd, a, W, b, dy = _draw(tag, 3, 5)
    x = torch.tensor(a, requires_grad=True)
    Wt = torch.tensor(W, requires_grad=True)
    bt = torch.tensor(b, requires_grad=True)
    y = tfops.conv_same(x, Wt, bt)
    gx, gW, gb = torch.autograd.grad((y * torch.tensor(dy)).sum(), [x, Wt, bt])
    kw = dict(rtol=1e-12, atol=1e-12)
    # forward: the loops, the slabs and torch
    naive = conv_ref.forward_naive64(a, W, b)
    np.testing.assert_allclose(naive, y.detach().numpy(), **kw)
    np.testing.assert_allclose(conv_ref.forward64(a, W, b, lo), naive, **kw)
    np.testing.assert_allclose(conv_ref.forward_torch(a, W, b, torch.float64), naive, **kw)
    # backward-data, with and without the mask of the layer below
    np.testing.assert_allclose(conv_ref.bwd_data64(dy, W, lo), gx.numpy(), **kw)
    np.testing.assert_allclose(conv_ref.bwd_data64(dy, W, lo, act=a), gx.numpy() * (a > 0), **kw)
    np.testing.assert_allclose(conv_ref.bwd_data_torch(dy, W, a, torch.float64), gx.numpy() * (a > 0), **kw)
    assert np.count_nonzero(a == 0) and np.count_nonzero(gx.numpy() * (a == 0))      # the mask removes something
    # per-sample weight gradients: their sum over the samples is autograd's
    dW, db = conv_ref.wgrad64(a, dy, k3, lo)
    tW, tb = conv_ref.wgrad_torch(a, dy, W, torch.float64)
    np.testing.assert_allclose(dW, tW, **kw)
    np.testing.assert_allclose(db, tb, **kw)
    np.testing.assert_allclose(dW.sum(0), gW.numpy(), **kw)
    np.testing.assert_allclose(db.sum(0), gb.numpy(), **kw)


@pytest.mark.parametrize('tag', ['k2', 'k4_2d', 'k234', 'k147'])
def test_a_wrong_lo_is_seen_at_even_windows(tag):
    """The slip the even windows are in the table for - the backward taps shifted as if the padding were symmetric the other
    way (lo' = k - 1 - lo) - changes bwd_data64 at every even k and at no odd one."""
    size, k3, lo, nd, a, W, b, dy = _draw(tag, 3, 5)
    other = [k - 1 - l for k, l in zip(k3, lo)]
    assert other != lo
    assert np.abs(conv_ref.bwd_data64(dy, W, other) - conv_ref.bwd_data64(dy, W, lo)).max() > 1e-3
    size, k3, lo, nd, a, W, b, dy = _draw('k3_oddw', 3, 5)
    assert [k - 1 - l for k, l in zip(k3, lo)] == lo


def test_exact_inputs_are_small_integers():
    x, W, b = conv_ref.exact_inputs(5, (2, 5, 8), 8, 6, [1, 4, 7], seed=1)
    assert x.shape == (5, 2, 5, 8, 8) and W.shape == (1, 4, 7, 8, 6) and b.shape == (6,)
    assert np.all(x == np.round(x)) and np.all(W == np.round(W)) and np.all(2 * b == np.round(2 * b))
    assert max(np.abs(x).max(), np.abs(W).max(), np.abs(b).max()) <= 4 and not x[0].any()
    y = conv_ref.forward_naive64(x, W, b)
    assert np.all(2 * y == np.round(2 * y)) and np.abs(y).max() < 2 ** 22


def test_models_of_the_table_evaluate_in_the_oracle():
    """Every model schema of conv_ref builds in the oracle at an even window, an asymmetric one and the 2-D schema."""
    from oracle import netspec
    from oracle.model import OracleModel
    for (ld, sk), in_shape in ((conv_ref.first_layer(8, [2, 2, 2], 'M'), (4, 3, 5, 3)), (conv_ref.below_conv(8, 6, [4, 4], 'MA'), (5, 7, 1)),
                               (conv_ref.below_conv(4, 8, [1, 4, 7], 'M'), (2, 5, 8, 1)), (conv_ref.skip_concat([2, 2, 2]), (4, 6, 5, 1)),
                               (conv_ref.accumulating([1, 3, 3]), (3, 6, 5, 1))):
        pars = netspec.he_init(ld, in_shape, seed=3, skips=sk, bias_std=0.05)
        om = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
        x = np.random.RandomState(4).randn(2, *in_shape).astype(np.float32)
        p = om.forward(x)['posteriors']
        assert p.shape == (2, 2) and np.isfinite(p).all()
        g = om.grad_log_post(1, x[[0]])
        assert len(g) == 2 * len(pars) and all(np.isfinite(np.asarray(a)).all() for a in g)
