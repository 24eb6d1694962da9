"""tests/select_ref.py held to its own statements without a GPU: the sort key against the contract of include/alq.h, the host-side
merge (alq_topk_merge) and the two CPU fakes against it, the similarity references against the NumPy the reference programs use,
and the exactness assertions and coverage claims of every case table.

No GPU is needed, but the alq_topk_merge tests call the host function inside libalq.so, so the library has to be built first
(`python __graft_entry__.py` cross-compiles it without a GPU), like for the other host tests that load it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import select_ref as R


def _f(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------------------------------------ order_key
@pytest.mark.parametrize('n', [1, 2, 3, 255, 2049])
def test_order_key_is_numeric_order_on_plain_keys(n):
    """NaN-free keys without -0.0: the key order is NumPy's (value, index) order, for distinct and for heavily tied keys."""
    for k in (R.topk_keys('distinct', n), np.round(R.topk_keys('distinct', n) * 40) / 4 + 0.0, R.topk_keys('absdev', n)):
        assert not np.isnan(k).any() and not (np.signbit(k) & (k == 0)).any()
        np.testing.assert_array_equal(R.topk_ref(k, n), np.lexsort((np.arange(n), k)))


def test_order_key_special_rules():
    key = lambda *bits: [int(x) for x in R.order_key(_f(list(bits)))]
    mz, pz = key(0x8000000000000000, 0x0000000000000000)
    assert pz == mz + 1                                                          # -0.0 IMMEDIATELY before +0.0
    dmin_n, dmin_p = key(0x8000000000000001, 0x0000000000000001)
    assert dmin_n == mz - 1 and dmin_p == pz + 1                                 # the nearest numbers on either side
    pinf, ninf, pmax, nmax = key(0x7FF0000000000000, 0xFFF0000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF)
    assert ninf < nmax < mz < pz < pmax < pinf
    for nan in (0x7FF0000000000001, 0x7FF8000000000000, R.NAN_PAD):              # sign clear: after +inf
        assert key(nan)[0] > pinf
    for nan in (0xFFF0000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF):     # sign set: before -inf
        assert key(nan)[0] < ninf
    assert key(R.NAN_PAD)[0] == int(R.PAD_KEY) and key(0xFFFFFFFFFFFFFFFF)[0] == 0


def test_order_key_is_a_strict_total_order():
    """Different bit patterns never share a key (on the specials sets and on random bit patterns), and no key exceeds the padding's."""
    rs = np.random.RandomState(0)
    rand = rs.randint(0, 1 << 62, size=4096).astype(np.uint64) << np.uint64(2) | rs.randint(0, 4, size=4096).astype(np.uint64)
    for k in [R.topk_keys('specials', n) for n in (255, 2049, 8193)] + [_f(list(R.SPECIAL_BITS)), rand.view(np.float64)]:
        bits = k.view(np.uint64)
        keys = R.order_key(k)
        assert len(np.unique(keys)) == len(np.unique(bits))
        assert keys.dtype == np.uint64 and (keys <= R.PAD_KEY).all()
        assert ((keys == R.PAD_KEY) == (bits == np.uint64(R.NAN_PAD))).all()
    # numeric order between any two numbers of the specials
    k = _f(list(R.SPECIAL_BITS))
    num = ~np.isnan(k)
    a, b = np.meshgrid(np.nonzero(num)[0], np.nonzero(num)[0])
    lt = k[a] < k[b]
    assert (R.order_key(k)[a][lt] < R.order_key(k)[b][lt]).all()


def test_specials_hold_what_they_claim():
    for n in R.TOPK_N:
        k = R.topk_keys('specials', n)
        bits = set(int(x) for x in k.view(np.uint64))
        pos = R.special_positions(n)
        assert 0 in pos and n - 1 in pos and len(set(pos)) == len(pos) and all(0 <= p < n for p in pos)
        for b in range(R.CHUNK, n, R.CHUNK):
            assert b - 1 in pos and b in pos
        assert int(k.view(np.uint64)[n - 1]) == R.NAN_PAD
        if n >= 255:
            assert bits >= set(R.SPECIAL_BITS)


def test_topk_case_table_covers_what_it_claims():
    rows = R.topk_cases()
    assert set((n, B) for n, B, _ in rows) == set(R.TOPK_SIZES)
    for n in R.TOPK_N + (R.TOPK_N_BIG,):
        assert set(s for m, _, s in rows if m == n) == set(R.KEY_SET_NAMES)
        assert R.topk_Bs(n) == (sorted(set([0, 1, min(n, 700), n])) if n != R.TOPK_N_BIG else [1, 4096])
    for s in R.KEY_SET_NAMES:
        assert any(B == n and R.padded_size(n) != n and n > R.CHUNK for n, B, t in rows if t == s), s
    assert R.padded_size(R.TOPK_N_BIG) == 1 << 22
    assert [R.padded_size(n) for n in (1, 2048, 2049, 4096, 4097)] == [2048, 2048, 4096, 4096, 8192]
    for name in R.KEY_SET_NAMES:                                                  # the key sets are what their names say
        k = R.topk_keys(name, 2049)
        assert k.dtype == np.float64 and k.shape == (2049,)
    assert len(np.unique(R.topk_keys('distinct', 2049))) == 2049 and (R.topk_keys('distinct', 2049) < 0).any()
    assert len(np.unique(R.topk_keys('few_values', 2049))) == 5 and len(np.unique(R.topk_keys('all_equal', 2049))) == 1
    assert (np.diff(R.topk_keys('ascending', 2049)) > 0).all() and (np.diff(R.topk_keys('descending', 2049)) < 0).all()
    p = R.absdev_posts(2049, 1)
    assert p.dtype == np.float32 and all((p == v).any() for v in (0.5, 0.0, 1.0)) and len(np.unique(p)) < 2049


# ------------------------------------------------------------------------------------------------ alq_topk_merge
def _merge(keys, idx, B):
    import nnal_amd  # noqa: F401
    from nnal_amd._lib import check, lib
    keys, idx = np.ascontiguousarray(keys, dtype=np.float64), np.ascontiguousarray(idx, dtype=np.int64)
    out = np.full(max(int(B), 1), -9, np.int64)
    n_out = C.c_int64(-1)
    check(lib().alq_topk_merge(keys.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), len(keys), int(B),
                               out.ctypes.data_as(C.c_void_p), C.byref(n_out)))
    return out[:n_out.value]


def _nonneg_keys(n, seed):
    rs = np.random.RandomState(seed)
    k = np.round(rs.rand(n), 2)                                                   # many ties, +0.0 among them
    k[rs.randint(0, n, size=5)] = np.inf
    k[rs.randint(0, n, size=5)] = _f([0x7FF8000000000000])[0]
    k[rs.randint(0, n, size=2)] = _f([R.NAN_PAD])[0]
    k[rs.randint(0, n, size=3)] = _f([0x0000000000000001])[0]
    return k


@pytest.mark.parametrize('n,B', [(1, 1), (500, 64), (500, 500), (2049, 700), (500, 0)])
def test_merge_equals_topk_ref_on_nonnegative_keys(n, B):
    """With global indices 0 .. n-1 in order and sign-clear keys (+NaN and +inf included) the merge is topk_ref of the same keys."""
    k = _nonneg_keys(n, n)
    assert not np.signbit(k).any()
    np.testing.assert_array_equal(_merge(k, np.arange(n), B), R.topk_ref(k, B))


def test_merge_orders_by_global_index_and_drops_padding():
    rs = np.random.RandomState(4)
    n = 600
    k = _nonneg_keys(n, 7)
    g = rs.permutation(5000)[:n].astype(np.int64)
    g[::7] = -1
    g[3] = -5
    keep = g >= 0
    want = g[keep][np.lexsort((g[keep], R.order_key(k[keep])))]
    for B in (0, 1, 64, int(keep.sum())):
        np.testing.assert_array_equal(_merge(k, g, B), want[:B])
    np.testing.assert_array_equal(_merge(k, g, n), want)                          # B above the kept count: every kept entry, once
    assert len(_merge(k, np.full(n, -1), 10)) == 0


def test_merge_differs_from_the_device_rule_on_signed_zero_and_negative_keys():
    """The documented difference (include/alq.h): the merge treats -0.0 as +0.0 (index decides) and compares the raw bits of
    everything else, so a negative key sorts BEHIND every sign-clear one; alq_topk_uncertain sorts numerically with -0.0 first."""
    k = np.array([0.0, -0.0, 0.0, -0.0, 1.0])
    np.testing.assert_array_equal(_merge(k, np.arange(5), 5), [0, 1, 2, 3, 4])
    np.testing.assert_array_equal(R.topk_ref(k, 5), [1, 3, 0, 2, 4])
    k = np.array([2.0, -1.0, np.inf, -3.0])
    np.testing.assert_array_equal(_merge(k, np.arange(4), 4), [0, 2, 1, 3])       # raw bits: -1.0 < -3.0, both behind +inf
    np.testing.assert_array_equal(R.topk_ref(k, 4), [3, 1, 0, 2])


# ------------------------------------------------------------------------------------------------ the CPU fakes
def test_both_fakes_follow_the_device_order_on_signed_keys():
    from tests.fake_device import FakeSession
    from tests.test_committee_host import CommitteeSession
    for name, n in (('distinct', 300), ('few_values', 300), ('specials', 2049), ('absdev', 64)):
        k = R.topk_keys(name, n)
        t = torch.as_tensor(k.view(np.int64).copy()).view(torch.float64)
        for B in (0, 1, 17, n):
            want = R.topk_ref(k, B)
            for sess in (FakeSession(), CommitteeSession()):
                got = sess.topk_smallest(t, B)
                assert got.dtype == torch.int64
                np.testing.assert_array_equal(got.numpy(), want)
    k = torch.as_tensor(np.array([0.5, -2.0, 0.0, -0.0, -0.25]))
    np.testing.assert_array_equal(FakeSession().topk_smallest(k, 5).numpy(), [1, 4, 3, 2, 0])


# ------------------------------------------------------------------------------------------------ similarity references
def test_similarity_refs_agree_with_the_reference_programs_numpy():
    """The reference keeps features as COLUMNS (F [f, n]): norms = sqrt(sum(F ** 2, 0)), sims = F.T @ G / outer(norms_F, norms_G),
    a greedy score np.sum(np.max(sims[:, Q + [j]], axis=1)), core-set's np.max(sims, axis=0) and np.maximum."""
    rs = np.random.RandomState(11)
    A, B = rs.randn(37, 19), rs.randn(23, 19)
    F, G = A.T, B.T
    na, nb = R.row_norms_ref(A), R.row_norms_ref(B)
    np.testing.assert_allclose(na, np.sqrt(np.sum(F ** 2, axis=0)), rtol=1e-15)
    np.testing.assert_allclose(R.dots_ref(A, B), F.T @ G, rtol=0, atol=1e-13)
    S = R.cosine_ref(A, B, na, nb)
    np.testing.assert_allclose(S, (F.T @ G) / np.outer(np.sqrt(np.sum(F ** 2, 0)), np.sqrt(np.sum(G ** 2, 0))), rtol=0, atol=1e-14)
    Q = [4, 9]
    cmax = np.max(S[:, Q], axis=1)
    np.testing.assert_allclose(R.colsum_max_ref(S, None, None), S.sum(0), rtol=0, atol=1e-13)
    np.testing.assert_allclose(R.colsum_max_ref(S, cmax, None), [np.sum(np.max(S[:, Q + [j]], axis=1)) for j in range(23)], rtol=0,
                               atol=1e-13)
    skip = (rs.rand(37) < 0.3).astype(np.uint8)
    np.testing.assert_allclose(R.colsum_max_ref(S, cmax, skip),
                               [np.sum(np.max(S[skip == 0][:, Q + [j]], axis=1)) for j in range(23)], rtol=0, atol=1e-13)
    np.testing.assert_array_equal(R.colsum_max_ref(S, cmax, np.ones(37, np.uint8)), np.zeros(23))
    np.testing.assert_array_equal(R.take_colmax_ref(S, 9, 1, np.full(37, np.nan)), S[:, 9])
    np.testing.assert_array_equal(R.take_colmax_ref(S, 9, 0, S[:, 4]), cmax)
    v = rs.randn(23) * 0.3
    np.testing.assert_array_equal(R.fold_rowmax_ref(S, v), np.maximum(v, np.max(S, axis=0)))
    np.testing.assert_array_equal(R.fold_rowmax_ref(S[20:], R.fold_rowmax_ref(S[:20], v)), R.fold_rowmax_ref(S, v))


def test_exact_builders_hold_their_assertions_at_every_table_size():
    """Integer features: every summation order gives the same double - shown by summing forwards, backwards and pairwise; dyadic S
    the same for column sums, with and without the running maximum."""
    for n, b, f in R.SIM_CASES:
        A, B = R.int_features(n, f, 1), R.int_features(b, f, 2, nonzero_rows=True)
        R.assert_int_exact(A)
        assert B.any(axis=1).all()
        d = R.dots_ref(A, B)
        assert np.array_equal(d, np.rint(d)) and np.abs(d).max() <= 64 * f
        d_rev = A.astype(np.float64)[:, ::-1] @ B.astype(np.float64)[:, ::-1].T
        np.testing.assert_array_equal(d, d_rev)
        np.testing.assert_array_equal(d, np.einsum('if,jf->ij', A.astype(np.int64), B.astype(np.int64)))
        sq = (A.astype(np.float64) ** 2).sum(1)
        np.testing.assert_array_equal(sq, (A.astype(np.int64) ** 2).sum(1))
        np.testing.assert_array_equal(R.row_norms_ref(A), np.sqrt(sq))
        S, cmax = R.dyadic((n, b), 3), R.dyadic((n,), 4)
        R.assert_dyadic_exact(S, n)
        for cm in (None, cmax):
            want = R.colsum_max_ref(S, cm, None)
            T = S if cm is None else np.maximum(cm[:, None], S)
            np.testing.assert_array_equal(want, T[::-1].sum(0))
            np.testing.assert_array_equal(want, (np.rint(T * R.DYADIC_ONE).astype(np.int64).sum(0)) / R.DYADIC_ONE)
    R.assert_dyadic_exact(np.zeros((1, 1)), 2 ** 20)
    with pytest.raises(AssertionError):
        R.assert_dyadic_exact(np.full((1, 1), 1.0 / 2048), 1)
    with pytest.raises(AssertionError):
        R.assert_int_exact(np.full((1, 1), 9, np.float32))


def test_sim_case_table_covers_what_it_claims():
    ns, bs, fs = (set(c[i] for c in R.SIM_CASES) for i in range(3))
    assert ns == set(R.SIM_N) and bs == set(R.SIM_B) and fs == set(R.SIM_F)
    nb = set(c[:2] for c in R.SIM_CASES)
    assert nb >= set((n, b) for n in (63, 64, 65) for b in (63, 64, 65)) | {(513, 257)}
    assert len(R.SIM_CASES) < len(R.SIM_N) * len(R.SIM_B)
