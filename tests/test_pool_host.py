"""tests/pool_ref.py - the NumPy restatement of the max-pool kernels that tests/test_gpu_pool.py holds the device to -
against independent statements of the same operation, on the CPU: oracle/tfops.max_pool_same (torch's max_pool2d / 3d
over a -inf pad) bit for bit in fp32 and fp64, torch autograd through it on tie-free inputs, and windows written out by
hand for what neither fixes: which of two equal cells wins, and the arg-max numbering where the window starts outside the
tensor (lo > 0)."""
import numpy as np
import pytest
import torch

from oracle import tfops
from tests import pool_ref
from tests.pool_ref import GEOMETRIES


def _as5(a, nd):
    """[N, *sp, C] -> [N, D, H, W, C]."""
    return a[:, None] if nd == 2 else a


def _inputs(size, C, dtype, seed, ties):
    """N = 3 patches; tie-free: a permutation of distinct values; with ties: few distinct values, zeros of both signs."""
    rs = np.random.RandomState(seed)
    shape = (3,) + tuple(size) + (C,)
    n = int(np.prod(shape))
    if ties:
        x = rs.randint(-3, 3, size=shape).astype(dtype)
        x[rs.rand(*shape) < 0.2] = -0.0
        return x
    return ((rs.permutation(n).reshape(shape) - n // 3) * 0.37).astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('ties', [False, True], ids=['distinct', 'ties'])
@pytest.mark.parametrize('geom', list(GEOMETRIES))
def test_pool_fwd_equals_max_pool_same(geom, ties, dtype):
    size, w = GEOMETRIES[geom]
    nd = len(size)
    x = _inputs(size, 5, dtype, 11, ties)
    want = tfops.max_pool_same(torch.from_numpy(x), w, w).numpy()
    out, arg = pool_ref.pool_fwd(_as5(x, nd), pool_ref.win3(w))
    assert out.dtype == dtype and arg.dtype == np.uint8
    got = out[:, 0] if nd == 2 else out
    assert got.shape == want.shape
    # equal values (+0 == -0 here: which zero of a tie torch keeps is its own affair; the hand-written cases fix ours)
    np.testing.assert_array_equal(got, want)
    if not ties:
        view = np.uint32 if dtype == np.float32 else np.uint64
        np.testing.assert_array_equal(got.view(view), want.view(view))
    assert int(arg.max()) < int(np.prod(w))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('geom', list(GEOMETRIES))
def test_pool_bwd_equals_autograd_on_tie_free_inputs(geom, dtype):
    size, w = GEOMETRIES[geom]
    nd = len(size)
    x = _inputs(size, 3, dtype, 12, ties=False)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = tfops.max_pool_same(xt, w, w)
    dout = np.random.RandomState(13).randn(*y.shape).astype(dtype)
    y.backward(torch.from_numpy(dout))
    want = xt.grad.numpy()
    w3 = pool_ref.win3(w)
    out, arg = pool_ref.pool_fwd(_as5(x, nd), w3)
    din = pool_ref.pool_bwd(_as5(dout, nd), arg, _as5(x, nd).shape[1:4], w3)
    got = din[:, 0] if nd == 2 else din
    assert got.dtype == dtype
    np.testing.assert_array_equal(got, want)
    # every cotangent arrives exactly once
    assert np.count_nonzero(got) == np.count_nonzero(dout)


def test_same_pads_of_the_case_table():
    assert pool_ref.same_pads(8, 2) == (4, 0, 0)
    assert pool_ref.same_pads(7, 2) == (4, 0, 1)
    assert pool_ref.same_pads(4, 3) == (2, 1, 1)
    assert pool_ref.same_pads(5, 3) == (2, 0, 1)
    assert pool_ref.same_pads(5, 4) == (2, 1, 2)
    assert pool_ref.same_pads(2, 3) == (1, 0, 1)
    assert pool_ref.same_pads(1, 2) == (1, 0, 1)
    assert pool_ref.same_pads(7, 6) == (2, 2, 3)
    for n in range(1, 12):
        for w in range(1, 8):
            assert pool_ref.same_pads(n, w) == tfops.same_pads(n, w, w)


def test_hand_written_window_of_3_at_lo_1():
    """4 x 4, window 3: lo = 1, so output (0, 0) covers rows / columns -1 .. 1 and the cell (iy, ix) has the offset
    (iy + 1) * 3 + (ix + 1) there; output (1, 1) covers 2 .. 4, offsets (iy - 2) * 3 + (ix - 2)."""
    x = np.array([[5, 5, 1, 2],
                  [5, 7, 3, 3],
                  [0, -1, -4, -2],
                  [9, 9, -2, -3]], np.float32).reshape(1, 1, 4, 4, 1)
    out, arg = pool_ref.pool_fwd(x, [1, 3, 3])
    np.testing.assert_array_equal(out.reshape(2, 2), [[7, 3], [9, -2]])      # (1, 1): negative throughout, next to the pad: -2, not 0
    # (0, 1): 3 at (1, 2) and (1, 3): the first, offset 2 * 3 + 0; (1, 0): 9 at (3, 0) and (3, 1): offset 1 * 3 + 1
    np.testing.assert_array_equal(arg.reshape(2, 2), [[8, 6], [4, 1]])
    dout = np.array([[10, 20], [30, 40]], np.float32).reshape(1, 1, 2, 2, 1)
    din = pool_ref.pool_bwd(dout, arg, (1, 4, 4), [1, 3, 3])
    want = np.zeros((4, 4), np.float32)
    want[1, 1], want[1, 2], want[3, 0], want[2, 3] = 10, 20, 30, 40      # the tied cells (1, 3) and (3, 1) get nothing
    np.testing.assert_array_equal(din.reshape(4, 4), want)
    # ReLU mask and accumulate
    act = np.ones((1, 1, 4, 4, 1), np.float32)
    act[0, 0, 1, 2, 0] = 0.
    old = np.full((1, 1, 4, 4, 1), 0.5, np.float32)
    got = pool_ref.pool_bwd(dout, arg, (1, 4, 4), [1, 3, 3], act=act, old=old).reshape(4, 4)
    want2 = want + np.float32(0.5)
    want2[1, 2] = 0.
    np.testing.assert_array_equal(got, want2)


def test_hand_written_zero_signs_and_first_of_a_tie():
    """-0 > +0 and +0 > -0 are both false: the first zero of the window stays, with its sign."""
    x = np.array([-0., 0., 0., -0., -1., -0.], np.float32).reshape(1, 1, 1, 6, 1)
    out, arg = pool_ref.pool_fwd(x, [1, 1, 2])
    np.testing.assert_array_equal(arg.ravel(), [0, 0, 1])
    np.testing.assert_array_equal(np.signbit(out.ravel()), [True, False, True])
    np.testing.assert_array_equal(out.ravel(), [0., 0., 0.])


def test_hand_written_3d_numbering():
    """The byte counts the FULL window: D = 2, H = W = 1 under [2, 2, 2] (the window overhangs in y and x): the cell at
    z = 1 is offset (1 * 2 + 0) * 2 + 0 = 4.  D = 4 under [3, 3, 3]: lo = 1 on every axis, the only row and column are
    dy = dx = 1, so z = iz + 1 - 3 oz gives offset 9 dz + 4."""
    x = np.array([1, 3], np.float32).reshape(1, 2, 1, 1, 1)
    out, arg = pool_ref.pool_fwd(x, [2, 2, 2])
    assert out.ravel().tolist() == [3.] and arg.ravel().tolist() == [4]
    x = np.array([0, 0, 2, 8], np.float32).reshape(1, 4, 1, 1, 1)
    out, arg = pool_ref.pool_fwd(x, [3, 3, 3])
    assert out.ravel().tolist() == [0., 8.]
    assert arg.ravel().tolist() == [13, 13]      # output 0: z = 0 (dz = 1) before its equal z = 1; output 1: z = 3 (dz = 1)
    din = pool_ref.pool_bwd(np.array([5, 6], np.float32).reshape(1, 2, 1, 1, 1), arg, (4, 1, 1), [3, 3, 3])
    assert din.ravel().tolist() == [5., 0., 0., 6.]


def test_bytes_above_127_and_sums():
    size, w = GEOMETRIES['7x7x7_w666']
    x = _inputs(size, 4, np.float32, 14, ties=False)
    out, arg = pool_ref.pool_fwd(x, w)
    assert arg.max() > 127
    s, a = pool_ref.chan_sums64(out)
    assert s.dtype == np.float64 and s.shape == out.shape[:-1]
    f32 = out.sum(-1, dtype=np.float32)
    assert np.all(np.abs(f32 - s) <= pool_ref.sum_bound(a, 4))
