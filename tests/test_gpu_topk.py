"""The top-B sort (csrc/topk.hip, alq_topk_uncertain) on its own against tests/select_ref.topk_ref (GPU box).

Every query but `fi` ends in this sort, and a wrong pick is silent: the query still returns valid-looking indices.  The entry
point is called through ctypes so that the key, work and output buffers belong to the test: the work buffer is exactly
alq_topk_work_bytes(n) bytes carved out of a larger tensor, the output exactly B entries, both followed by a pattern that must
survive, and the keys must come back bit for bit.

Sizes (select_ref.TOPK_SIZES): n <= 2048 (one chunk, no global step), exact powers of two (no padding), one past them (all but one
padding), 6149 and 16385 (several global steps and several re-entries of the local kernel with kfirst = klast = k), 2^17 + 1, and
2^21 + 1 (P = 2^22: the grid-stride loops of topk_init_kernel and bitonic_global_kernel iterate twice), with B in
{0, 1, min(n, 700), n}.  Key sets (select_ref.KEY_SETS): distinct doubles of both signs, five values, all equal, sorted either way,
the specials (+-0.0, +-inf, NaNs of both signs, the NaN whose key equals the padding's, denormals, +-DBL_MAX, placed at 0, n - 1 and
on both sides of every 2048 boundary) and |fp32 p - 0.5|.  All comparisons are exact.

Measured on an MI355X (2026-10-20): every case passed against the kernel as it was - no product change.  The file's 130 tests take
4.3 s (pytest's own figure); the n = 2^21 + 1 cases take 0.15 - 0.31 s each (the slowest: specials), most of it the host's lexsort,
so all seven key sets stay, on B = 1 and 4096 in turn.  Nothing in the table is out of reach: every size above runs its global /
local step counts by construction.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import select_ref as R  # noqa: E402

GUARD = 0xA5
OUT_GUARD = -7070707


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev_f64(sess, k):
    """float64 host array -> device tensor, bit for bit (NaN payloads travel as integers)."""
    torch = sess.torch
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int64).copy()).to(sess.device).view(torch.float64)


def _work(sess, nbytes, slack=4096):
    return sess.torch.full((nbytes + slack,), GUARD, dtype=sess.torch.uint8, device=sess.device)


def _topk(sess, keys, B, work=None, work_n=None):
    """alq_topk_uncertain on host keys; checks the three buffers and returns the B indices."""
    from nnal_amd._lib import check
    torch = sess.torch
    n = len(keys)
    dk = _dev_f64(sess, keys)
    wb = sess.lib.alq_topk_work_bytes(n if work_n is None else work_n)
    if work is None:
        work = _work(sess, wb)
    out = torch.full((B + 64,), OUT_GUARD, dtype=torch.int64, device=sess.device)
    check(sess.lib.alq_topk_uncertain(sess.ctx, _ptr(dk), n, B, _ptr(out), _ptr(work)))
    torch.cuda.synchronize()
    assert np.array_equal(dk.view(torch.int64).cpu().numpy(), np.ascontiguousarray(keys).view(np.int64)), 'd_keys changed'
    assert bool((work[wb:] == GUARD).all()), 'write behind the work buffer'
    assert bool((out[B:] == OUT_GUARD).all()), 'write behind d_out[B]'
    return out[:B].cpu().numpy()


@pytest.mark.parametrize('n,B,name', R.topk_cases(), ids=lambda v: str(v))
def test_order(sess, n, B, name):
    keys = R.topk_keys(name, n)
    got = _topk(sess, keys, B)
    np.testing.assert_array_equal(got, R.topk_full_order(name, n)[:B])


@pytest.mark.parametrize('n', [n for n in R.TOPK_N if R.padded_size(n) != n])
def test_full_output_at_padded_sizes_is_a_permutation(sess, n):
    """B = n where the sorted array ends in padding: every index once, no padding index (-1), the NaN that shares the padding's
    key still ahead of it."""
    keys = R.topk_keys('specials', n)
    got = _topk(sess, keys, n)
    np.testing.assert_array_equal(np.sort(got), np.arange(n))
    np.testing.assert_array_equal(got, R.topk_full_order('specials', n))
    assert got[-1] == n - 1 and int(keys.view(np.uint64)[got[-1]]) == R.NAN_PAD


def test_B0_leaves_the_output_alone_and_null_pointers_pass_at_n0(sess):
    keys = R.topk_keys('distinct', 4097)
    assert len(_topk(sess, keys, 0)) == 0                        # _topk: out[0:] still holds the pattern
    assert sess.lib.alq_topk_uncertain(sess.ctx, _ptr(_dev_f64(sess, keys)), 4097, 0, None, _ptr(_work(sess, 1 << 17))) == 0
    assert sess.lib.alq_topk_uncertain(sess.ctx, None, 0, 0, None, None) == 0
    assert sess.lib.alq_topk_work_bytes(0) == 16 * 2048


def test_work_buffer_reuse_leaks_no_stale_pairs(sess):
    """One work buffer sized for 8193 serves n = 8193, then 100, then 4097 with other keys: stale pairs of an earlier, larger sort
    lie behind the region a smaller sort initialises and must stay out of it."""
    work = _work(sess, sess.lib.alq_topk_work_bytes(8193))
    for n, name in ((8193, 'specials'), (100, 'few_values'), (4097, 'distinct'), (100, 'descending')):
        keys = R.topk_keys(name, n)
        got = _topk(sess, keys, n, work=work, work_n=8193)
        np.testing.assert_array_equal(got, R.topk_full_order(name, n))


def test_work_bytes(sess):
    for n in R.TOPK_N + (R.TOPK_N_BIG,):
        p = 1
        while p < n:
            p <<= 1
        assert sess.lib.alq_topk_work_bytes(n) == 16 * max(2048, p)


def test_refusals(sess):
    from nnal_amd._lib import ALQ_EINVAL
    keys = R.topk_keys('distinct', 255)
    dk, work = _dev_f64(sess, keys), _work(sess, sess.lib.alq_topk_work_bytes(255))
    out = sess.torch.full((300,), OUT_GUARD, dtype=sess.torch.int64, device=sess.device)
    for n, B in ((255, 256), (255, -1), (-1, 0), (-3, -3)):
        assert sess.lib.alq_topk_uncertain(sess.ctx, _ptr(dk), n, B, _ptr(out), _ptr(work)) == ALQ_EINVAL
        msg = sess.lib.alq_last_error().decode()
        assert 'B=%d' % B in msg and 'n=%d' % n in msg, msg
    assert sess.lib.alq_topk_uncertain(sess.ctx, _ptr(dk), 255, 5, None, _ptr(work)) == ALQ_EINVAL
    assert 'null' in sess.lib.alq_last_error().decode()
    assert sess.lib.alq_topk_uncertain(sess.ctx, None, 255, 5, _ptr(out), _ptr(work)) == ALQ_EINVAL
    assert sess.lib.alq_topk_uncertain(sess.ctx, _ptr(dk), 255, 5, _ptr(out), None) == ALQ_EINVAL
    sess.torch.cuda.synchronize()
    assert bool((out == OUT_GUARD).all()) and bool((work == GUARD).all())


@pytest.mark.parametrize('n', [2049, 4097])
def test_through_the_wrappers(sess, n):
    """Session.topk_smallest and PW_NNAL.device_uncertainty_filter(with_keys=True) on posteriors with exact 0.5, 0, 1 and
    duplicates: the indices are binary_uncertainty_filter's, the keys ascending and |p - 0.5| bit for bit."""
    from nnal_amd import PW_NNAL
    torch = sess.torch
    p = R.absdev_posts(n, 77 + n)
    p64 = p.astype(np.float64)
    key = np.abs(p64 - 0.5)
    assert (key == 0).any() and (key == 0.5).sum() >= 2 and len(np.unique(key)) < n
    for B in (1, 700, n):
        want = PW_NNAL.binary_uncertainty_filter(p64, B)
        np.testing.assert_array_equal(want, R.topk_ref(key, B))
        got = sess.topk_smallest(_dev_f64(sess, key), B).cpu().numpy()
        np.testing.assert_array_equal(got, want)
        idx, k = PW_NNAL.device_uncertainty_filter(sess, sess.to_device(p, torch.float32), B, with_keys=True)
        np.testing.assert_array_equal(idx.cpu().numpy(), want)
        k = k.cpu().numpy()
        assert k.dtype == np.float64 and (np.diff(k) >= 0).all()
        np.testing.assert_array_equal(k.view(np.uint64), key[want].view(np.uint64))
        only = PW_NNAL.device_uncertainty_filter(sess, sess.to_device(p, torch.float32), B)
        np.testing.assert_array_equal(only.cpu().numpy(), want)
    big = sess.uncertainty_filter(sess.to_device(p, torch.float32), n + 5)          # B above n: clipped to n
    np.testing.assert_array_equal(big.cpu().numpy(), PW_NNAL.binary_uncertainty_filter(p64, n))
