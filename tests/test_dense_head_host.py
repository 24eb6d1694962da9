"""tests/dense_head_ref.py without a GPU: its matrix statements against plain triple loops in fp64, the first-maximum rule on
the constructed tie rows, the properties its input generators promise, and the launch-geometry helper of the library (host
arithmetic only: alq_dense_head_bwd_geometry makes no device call)."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_head_ref as ref


@pytest.mark.parametrize('R,Ci,c', [(1, 4, 2), (7, 12, 5), (9, 8, 8)])
def test_statements_equal_triple_loops(R, Ci, c):
    rs = np.random.RandomState(R + Ci + c)
    x, delta, W = (rs.randn(*s).astype(np.float32) for s in ((R, Ci), (R, c), (Ci, c)))
    b = rs.randn(c).astype(np.float32)
    fw, bw, loops = ref.forward(x, W, b), ref.backward(x, delta, W), ref.triple_loop(x, delta, W, b)
    for key, got in (('z', fw['z']), ('post', fw['post']), ('dX', bw['dX']), ('dW', bw['dW']), ('db', bw['db'])):
        assert got.shape == loops[key].shape and got.dtype == np.float64
        scale = np.abs(loops[key]).max()
        assert np.abs(got - loops[key]).max() <= 1e-14 * max(scale, 1.), key          # another order of fp64 additions
    assert np.array_equal(fw['pred'], loops['pred'])
    assert np.allclose(fw['post'].sum(0), 1., rtol=0, atol=1e-15)
    assert np.array_equal(ref.flat_grad(bw), np.concatenate([bw['dW'].reshape(-1), bw['db']]))
    # integer inputs: exact, whatever the order
    x, delta, W = ref.backward_ints(R, Ci, c, 3)
    bw, loops = ref.backward(x, delta, W), ref.triple_loop(x, delta, W, np.zeros(c))
    assert all(np.array_equal(bw[k], loops[k]) for k in ('dX', 'dW', 'db'))


def test_first_maximum_rule_on_tie_rows():
    assert np.array_equal(ref.first_argmax(np.asarray([[0., 1., 1.], [2., 2., 2.], [0., 1., 2.], [3., 1., 3.]])), [1, 0, 2, 0])
    for c in range(2, 9):
        z = ref.logits(np.zeros((1, 4), np.float32), np.ones((4, c), np.float32), ref.tie_bias(c))
        assert ref.first_argmax(z)[0] == 1 and (c == 2 or z[0, 1] == z[0, 2])
        for j in range(c - 1):
            x, W, b, want = ref.tie_case(12, c, j)
            fw = ref.forward(x, W, b)
            assert np.array_equal(fw['pred'], want) and np.array_equal(fw['pred'], ref.triple_loop(x, np.zeros((len(x), c)), W, b)['pred'])
            z = fw['z']
            assert (z[1::4, j] == z[1::4, j + 1]).all() and (z[1::4].max(1) == z[1::4, j]).all()          # the tie is the maximum
            assert (z[2::4] == 5).all() and (z[3::4].argmax(1) == c - 1).all()
            assert np.array_equal(z, np.round(z)) and {0, 1, 2, 3} == set(np.arange(len(x)) % 4)


@pytest.mark.parametrize('Ci', [4, 12, 64])
def test_input_generators_keep_their_promises(Ci):
    for c in (2, 5, 8):
        x, W, b = ref.forward_ints(1030, Ci, c, 5)
        fw = ref.forward(x, W, b)
        assert fw['spread'].max() <= 73 and np.array_equal(fw['z'], np.round(fw['z']))
        assert not x[0].any() and not x[-1].any() and (fw['pred'][[0, -1]] == 1).all()
        assert fw['post'].min() >= np.finfo(np.float32).tiny
        xw, Ww, _ = ref.forward_ints(1030, Ci, c, 5, wide=True)
        assert np.abs(Ww).max() == 4 and np.abs(xw).max() == 4
        x, d, W = ref.backward_ints(1000, Ci, c, 1)
        assert np.abs(x).max() == 4 and np.abs(d).max() == 3 and np.abs(W).max() <= 4 and x.dtype == d.dtype == W.dtype == np.float32


def test_bounds_cover_an_fp32_evaluation():
    """The bounds of the float cases hold for a NumPy fp32 evaluation in the device's order of operations (rows in chunks of
    64 summed in fp32, chunks folded in fp64): they are bounds of that arithmetic, whatever computes it."""
    rs = np.random.RandomState(0)
    R, Ci, c = 1000, 12, 5
    x, delta, W = (rs.randn(*s).astype(np.float32) for s in ((R, Ci), (R, c), (Ci, c)))
    b = rs.randn(c).astype(np.float32)
    bw = ref.backward(x, delta, W)
    bd = ref.grad_bounds(x, delta, W, bw)
    dW = np.zeros((Ci, c))
    for a in range(0, R, 64):
        acc = np.zeros((Ci, c), np.float32)
        for r in range(a, min(R, a + 64)):
            acc = (acc + np.outer(x[r], delta[r]).astype(np.float32)).astype(np.float32)
        dW += acc
    assert (np.abs(dW.astype(np.float32).reshape(-1) - bw['dW'].reshape(-1)) <= bd['g'][:Ci * c]).all()
    z32 = np.tile(b, (R, 1))
    for i in range(Ci):
        z32 = (z32 + np.outer(x[:, i], W[i]).astype(np.float32)).astype(np.float32)
    assert (np.abs(z32 - ref.logits(x, W, b)) <= ref.logit_bound(x, W, b)).all()
    assert ref.post_rel_bound(5) == 9 * 2. ** -24


def _geometry(R, Ci):
    from nnal_amd import _lib
    blocks, sweep, flush, per = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    rc = _lib.lib().alq_dense_head_bwd_geometry(R, Ci, C.byref(blocks), C.byref(per), C.byref(sweep), C.byref(flush))
    return rc, (blocks.value, per.value, sweep.value, flush.value)


def test_launch_geometry_helper():
    """What the regimes of the kernel-level cases rest on: 8 sweeps a workgroup up to 2048 workgroups, then more rows each; the second fold in
    fp64 past flush_rows * rows_per_sweep rows of a workgroup."""
    import nnal_amd  # noqa: F401
    from nnal_amd import _lib
    L = _lib.lib()
    assert _geometry(1, 4) == (0, (1, 1, 256, 64))
    assert _geometry(8 * 85, 12) == (0, (1, 680, 85, 64)) and _geometry(8 * 85 + 1, 12) == (0, (2, 341, 85, 64))
    assert _geometry(24 * 19 + 5, 52)[1][:3] == (4, 116, 19)
    assert _geometry(262144, 64)[1][:2] == (2048, 128) and _geometry(262145, 64)[1][:2] == (2048, 129)
    assert _geometry(3 * 262144 + 5, 64)[1][:2] == (2048, 385)
    assert _geometry(2048 * 16 * 64, 64)[1][:2] == (2048, 1024) and _geometry(2048 * 16 * 64 + 1, 64)[1][:2] == (2048, 1025)
    assert _geometry(2228227, 64)[1] == (2048, 1089, 16, 64)
    for R, Ci in ((1, 4), (5000, 20), (786437, 64), (2228227, 64), (10 ** 7, 28)):
        _, (blocks, per, sweep, flush) = _geometry(R, Ci)
        assert 1 <= blocks <= 2048 and blocks * per >= R and flush == 64 and sweep == 256 // (Ci // 4)
    for Ci in (0, 2, 6, 68, -4):
        assert _geometry(5, Ci)[0] == -4 and b'alq_dense_head_bwd_geometry' in L.alq_last_error()
    assert _geometry(0, 8)[0] == -1
    i, q = C.c_int(), C.c_int64()
    ok = (C.byref(i), C.byref(q), C.byref(i), C.byref(i))
    for k in range(4):
        assert L.alq_dense_head_bwd_geometry(5, 8, *(ok[:k] + (None,) + ok[k + 1:])) == -1
    assert L.alq_dense_head_work_bytes(12, 5) == 2048 * (12 * 5 + 5) * 8
    assert L.alq_dense_head_work_bytes(0, 5) == 0 and L.alq_dense_head_work_bytes(12, 0) == 0 and L.alq_dense_head_work_bytes(-4, -2) == 0
