"""tests/fc_small_ref.py against OracleModel(dtype=float64) and its own case tables (CPU): the statement tests/test_gpu_fc_small.py
holds the skinny fc kernels to is checked here without a device, and every integer-input case of that file is shown to meet the
condition under which bit equality is owed - every partial sum any summation order could form is below 2^24 in magnitude."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import netspec, tfops
from oracle.model import OracleModel
from tests import fc_small_ref as R


# ------------------------------------------------------------------------------------------ the statement against the oracle
MODELS = [('2d', OrderedDict([('cv', ['conv', [4, [3, 3]], 'MA']), ('fc', ['fc', [3]])]), (5, 7, 1)),
          ('3d', OrderedDict([('cv', ['conv', [6, [3, 3, 3]], 'MA']), ('fc', ['fc', [5]])]), (2, 3, 5, 1))]


@pytest.mark.parametrize('name,ld,in_shape', MODELS, ids=[m[0] for m in MODELS])
def test_statement_vs_oracle_fp64(name, ld, in_shape):
    pars = netspec.he_init(ld, in_shape, seed=7, bias_std=0.1)
    om = OracleModel(ld, in_shape, pars, feature_layer=0, dtype=torch.float64)
    n = 3
    x = np.random.RandomState(8).randn(n, *in_shape)
    res = om.forward(x)
    act = res['feature_layer']
    C = act.shape[-1]
    shape = tuple(in_shape[:-1]) + (C,)
    assert act.shape == (n,) + shape and np.count_nonzero(act == 0) and np.count_nonzero(act > 0)
    W, b = (np.asarray(a, np.float64) for a in pars['fc'])
    kw = dict(rtol=1e-12, atol=1e-13)
    z = R.logits64(act, W, b, shape)
    np.testing.assert_allclose(z, res['output'].T, **kw)
    p, pred = R.softmax64(z)
    np.testing.assert_allclose(p, res['posteriors'].T, **kw)
    assert np.array_equal(pred, res['prediction'])
    # the order is not the memory order (a restatement that ignored the transpose would pass nothing here)
    assert np.abs(act.reshape(n, -1) @ W.T + b.reshape(1, -1) - z).max() > 1e-3
    for i in range(n):
        for j in range(W.shape[0]):
            g = om.grad_log_post(j, x[[i]])
            delta = (np.eye(W.shape[0])[j] - p[i])[None]          # d log p_j / d logits
            dW, db = R.wgrad64(act[[i]], delta, shape)
            np.testing.assert_allclose(dW[0], g[2], **kw)
            np.testing.assert_allclose(db[0], g[3], **kw)
            # the masked input cotangent, summed over the voxels, is the conv's bias gradient; the channel sums add up to its total
            dm = R.din64(delta, W, shape, act=act[[i]])
            np.testing.assert_allclose(dm.reshape(-1, C).sum(0), g[1], **kw)
            np.testing.assert_allclose(R.chansum64(dm, C).sum(), g[1].sum(), **kw)
            plain = R.din64(delta, W, shape)
            assert np.array_equal(dm, plain * (act[[i]].reshape(1, -1) > 0)) and np.count_nonzero(plain * (act[[i]].reshape(1, -1) == 0))


def test_order_comes_from_flatten_tf():
    """mem_of_tf is flatten_tf's own permutation: of a 3-D activation with three different sizes, element (d, h, w, c) sits at
    ((c W + w) H + h) D + d of the reference's order - and w_mem undoes it."""
    D, H, Wd, C = 3, 4, 5, 2
    m = R.mem_of_tf((D, H, Wd, C))
    assert sorted(m) == list(range(D * H * Wd * C))
    for d, h, w, c in ((0, 0, 0, 0), (2, 3, 4, 1), (1, 2, 3, 0), (0, 3, 1, 1)):
        assert m[((c * Wd + w) * H + h) * D + d] == ((d * H + h) * Wd + w) * C + c
    x = torch.arange(2 * D * H * Wd * C, dtype=torch.float64).reshape(2, D, H, Wd, C)
    assert np.array_equal(tfops.flatten_tf(x).numpy()[:, 1], x[1].reshape(-1).numpy()[m])
    W = np.arange(3 * m.size, dtype=np.float64).reshape(3, -1)
    assert np.array_equal(R.w_mem(W, (D, H, Wd, C))[:, m], W)


def test_sign_bytes_and_bits_sums():
    act = np.array([[0., 1., -1., 2., 3., 0., 0., 0., -1., -2., -3., -4., 1., 1., 1., 1.]])
    assert R.sign_bytes(act).tolist() == [[0b1010, 0b0001, 0, 0b1111]]
    wv = np.arange(16, dtype=np.float64) + 1
    assert R.bits_dsum64(act, wv).tolist() == [[2 + 4 + 5, 13 + 14 + 15 + 16]]
    # ... which is the channel sum of the masked cotangent under the unit cotangent (+1, -1)
    W = np.stack([wv, np.zeros(16)])
    assert np.array_equal(R.chansum64(R.din64([[1., -1.]], W, (1, 1, 16), act=act), 8), R.bits_dsum64(act, wv))


def test_softmax64_edges():
    p, pred = R.softmax64([[1., 1., 1.], [0., 5., 5.], [100., -100., 0.], [-1e4, 1e4, 0.]])
    assert pred.tolist() == [0, 1, 0, 1] and np.isfinite(p).all()
    assert p[0].tolist() == [1 / 3] * 3 and p[3].tolist() == [0., 1., 0.] and p[2, 0] == 1. and 0 < p[2, 1] < 1e-80


# ------------------------------------------------------------------------------------------ the tables
def test_first_layer_table_covers_what_it_says():
    Fs = sorted({int(np.prod(c.in_shape)) for c in R.FIRST if c.in_shape[:2] == (1, 1)})
    assert Fs == [1, 3, 4, 1023, 1024, 8188, 8192, 8193, 8196, 16388, 24577]
    assert sorted({c.c for c in R.FIRST}) == list(range(1, 9)) and R.WIDE.c == 9
    assert {R.slices(F) for F in Fs} == {1, 2, 3, 4} and R.slices(8192) == 1 and R.slices(8193) == 2 and R.slices(24577) == 4
    assert 8193 - R.FC_SLICE == 1 and 8196 - R.FC_SLICE == 4 and 16388 - 2 * R.FC_SLICE == 4
    assert {F % 4 == 0 for F in Fs} == {True, False}
    assert (3, 4, 5, 2) in [c.in_shape for c in R.FIRST] and (5, 7, 3) in [c.in_shape for c in R.FIRST]


@pytest.mark.parametrize('c', R.FIRST + [R.WIDE], ids=[c.tag for c in R.FIRST + [R.WIDE]])
def test_first_layer_integer_cases_are_exact(c):
    n = max(R.BATCHES)
    x, W, b = R.exact_fc_inputs(n, c.in_shape, c.c, seed=100 + len(c.tag))
    F = int(np.prod(c.in_shape))
    assert x.shape == (n,) + c.in_shape and W.shape == (c.c, F) and not x[0].any() and np.count_nonzero(x[1]) == min(F, 2)
    bound = R.assert_exact(x, W, b, c.in_shape)
    z = R.logits64(x, W, b, c.in_shape)
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and np.array_equal(z[0], b.astype(np.float64))
    if F >= 1023:      # a permuted or dropped column of W changes a logit; no two rows agree
        assert len({tuple(r) for r in W}) == c.c and bound > 1000
        Wp = W.copy()
        Wp[:, [0, F - 1]] = Wp[:, [F - 1, 0]]
        assert not np.array_equal(R.logits64(x, Wp, b, c.in_shape), z)


def test_hidden_chain_integer_case_is_exact():
    x, W, b, W2, b2 = R.hidden_inputs(max(R.BATCHES), seed=5)
    shape = (1, 1, R.HIDDEN_F)
    R.assert_exact(x, W, b, shape)
    h = R.logits64(x, W, b, shape, relu=True)
    assert np.count_nonzero(h == 0) and np.count_nonzero(h > 0)      # the finish kernel's ReLU has something to do
    R.assert_exact(h, W2, b2, (1, 1, 8))


def test_below_conv_table_covers_what_it_says():
    forms = {c.form for c in R.BELOW}
    assert forms == {'G0', 'G1', 'G2', 'G4', 'G8', 'scalar'}
    for c in R.BELOW:
        F, sp = R.below_F(c)
        assert len(set(c.size)) > 1 or len(c.size) == 2, c      # ragged
        assert F % 1024, c                                      # never the bits head
        if c.form == 'scalar':
            assert F % 4 and c.C == 6
        elif c.form == 'G0':
            assert F % 4 == 0 and (c.C % 4 or c.C // 4 not in (1, 2, 4, 8) or c.pool)
        else:
            assert F % 4 == 0 and c.C == 4 * int(c.form[1:]) and not c.pool
    assert sorted({c.c for c in R.BELOW}) == [2, 3, 5, 8] and {c.C for c in R.BELOW} >= {4, 8, 16, 32, 12, 20, 6}
    assert any(c.ops == 'M' for c in R.BELOW) and any(c.pool for c in R.BELOW)
    assert any((4 * R.below_F(c)[0] // 4) % 64 for c in R.BELOW)      # N F / 4 of a full pass of 4 patches off a whole wave


def test_bits_tables():
    for tag, size in R.BITS_GEOMS.items():
        assert (int(np.prod(size)) * 8) % 1024 == 0
    assert int(np.prod(R.BITS_GEOMS['4x4x8'])) * 8 == 1024 == int(np.prod(R.BITS_GEOMS['8x16'])) * 8
    F = int(np.prod(R.BITS_GEOMS['8x12x12'])) * 8
    assert F == 9216 and -(-(F // 32) // 256) == 2 and (F // 32) % 256      # two workgroups of fc_small_dsum_bits_kernel, ragged second
    assert [-(-n // R.FC_BITS_PG) for n in R.BITS_N] == [1, 1, 1, 2]
    assert (5 * 5 * 5 * 8) % 1024 and [t[0] for t in R.NO_BITS] == ['F1000', 'C16', 'c3', 'first']


@pytest.mark.parametrize('tag', ['4x4x8', '8x16', '8x12x12'])
@pytest.mark.parametrize('negative', [False, True])
def test_bits_integer_cases_are_exact(tag, negative):
    size = R.BITS_GEOMS[tag]
    n = max(R.BITS_N)
    x, pars = R.bits_exact_inputs(n, size, seed=40 + len(tag), negative=negative)
    a0, a1 = R.bits_exact_acts(x, pars)
    shape = tuple(size) + (8,)
    assert a1.shape == (n,) + shape and np.all(a1 == np.round(a1)) and np.all(a0 == np.round(a0))
    # both convs: |x| W sums below 2^24 by a wide margin (27 taps x 8 channels of values below 28)
    assert a0.max() <= 27 and a1.max() <= 27 * 8 * 27
    Wf, bf = pars['fc']
    R.assert_exact(a1, Wf, bf, shape)
    wv = R.w_mem(Wf, shape)
    wv = wv[0] - wv[1]
    R.assert_exact(a1, wv[None], bf[0] - bf[1])      # the fused head sums act (W0 - W1)
    assert np.abs(R.bits_dsum64(a1, wv)).max() <= 8 * 4
    sb = R.sign_bytes(a1)
    assert not sb[0].any()      # the all-zero patch
    if negative:
        assert not sb.any() and not a1.any()
    else:
        assert all(0 < np.count_nonzero(sb[i]) and np.count_nonzero(sb[i] != 15) for i in range(1, n))      # mixed
        assert len({int(v) for v in sb[2:].reshape(-1)}) == 16      # every nibble occurs
