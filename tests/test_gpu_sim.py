"""The five similarity kernels behind `rep-entropy` and `core-set` (csrc/sim.hip) on their own, each through its C entry point,
against the fp64 references of tests/select_ref.py (GPU box).

Exact where arithmetic allows it: integer-valued fp32 features (every partial sum an integer below 2^53, so any summation order
gives the same double) make the dot products, the squared norms and - with the device's own norms read back - the cosine quotient
comparable bit for bit; similarity matrices of multiples of 2^-10 do the same for the column sums of alq_colsum_max.  On random
features the only error is the summation's, and the bar is the standard bound f 2^-53 sum |terms| on the ACCUMULATED value: the
device returns that value behind one more correctly rounded operation (a root, or a quotient by the rounded product of two norms),
so the check asks, in exact rational arithmetic, whether some accumulated value within the bound of the exact sum rounds to what the
device returned (_interval_miss).  Nothing is fitted to the device's output.

Every input is the front of a larger allocation whose tail is NaN (_dev): a kernel that reads one K slice or one chunk past its
input stays inside its allocation and sums the NaN into an entry it writes, and every output is followed by a pattern that must
survive.  What this cannot show is an over-read whose value never reaches a written entry: cos_gemm_kernel loading row b of B
(`j0 + r <= b`) puts it into the LDS column of output column j = b, which the write-back drops - C is bit-identical at every size
(see the mutation list in DESIGN.md).  Only a bounds-checking tool could see that one; comparing outputs cannot.

Sizes (select_ref.SIM_CASES): a covering table over n in {1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513} (row_norm_kernel's four rows
per block, the 64-row GEMM tile, colsum's 256-row chunks), b in {1, 15, 16, 63, 64, 65, 256, 257} (the 64-column tile: blockIdx.y
> 0; colsum's second column block at b = 257) and f in {1, 15, 16, 17, 63, 64, 65, 70} (the 16-deep K slice, the 64-lane row loop).

The whole queries at the end cross the same edges: rep-entropy with B = 70 candidates and 310 remaining voxels, core-set with 1001
labelled voxels (two batches through gen_batch_inds), each greedy step's margin asserted against the summation bound.

Measured on an MI355X (2026-10-20): every check passed against the kernels as they were - no product change.  alq_row_norms on
integer features: 0 of 1870 entries differ from sqrt(exact sum) (0 ulp); the cosine quotient on integer features is bit-exact in
all 17 cases (0 of 307 k entries differ), so the one-ulp fall-back was not needed.  Random features: the accumulated value is within
0.042 of the bound for the norms, 0.110 for the cosines, 0.176 for the unit diagonal.  The file's 91 tests take 2.8 s (pytest's own figure; the slowest call 0.07 s).
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import select_ref as R  # noqa: E402
from tests.test_gpu_strategies import _feats, _setup  # noqa: E402

# alq_row_norms against sqrt(exact sum) on integer features: one correctly rounded root on either side, so at most one ulp may
# separate them (measured on an MI355X, 2026-10-20: 0 ulp in all 1870 rows).
ROW_NORM_ULP_ALLOWED = 1
R_CS = 256                        # rows per chunk of colsum_max_kernel: the slack behind a similarity matrix
U = 2.0 ** -53
GUARD = -12345.675


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(sess, a, slack):
    """Host array -> the front of a device allocation whose `slack` further elements are NaN (uint8, the skip flags: 0, so that a
    row read past the end is not skipped but summed, NaN and all)."""
    torch = sess.torch
    a = np.ascontiguousarray(a)
    h = torch.from_numpy(a.reshape(-1).copy())
    t = torch.empty((a.size + slack,), dtype=h.dtype, device=sess.device)
    t[:a.size] = h.to(sess.device)
    t[a.size:] = 0 if a.dtype == np.uint8 else float('nan')
    return t[:a.size].view(a.shape) if a.size else t[:0]


def _feat(sess, A):
    return _dev(sess, A, 64 * A.shape[1] + 64)                  # a row tile and a K slice of NaN behind the features


def _sim(sess, S):
    return _dev(sess, S, R_CS * S.shape[-1] + 64)               # a 256-row chunk of NaN behind the similarity matrix


def _out(sess, n, fill=GUARD, slack=64):
    return sess.torch.full((n + slack,), fill, dtype=sess.torch.float64, device=sess.device)


def _tail_ok(t, n, fill=GUARD):
    return bool((t[n:] == fill).all())


def _ulps(a, b):
    return np.abs(np.asarray(a).view(np.int64) - np.asarray(b).view(np.int64))


def _row_norms(sess, dA, n, f):
    from nnal_amd._lib import check
    out = _out(sess, n)
    check(sess.lib.alq_row_norms(sess.ctx, _ptr(dA), n, f, _ptr(out)))
    sess.torch.cuda.synchronize()
    assert _tail_ok(out, n)
    return out[:n]


def _cosine(sess, dA, n, dB, b, f, na, nb):
    from nnal_amd._lib import check
    out = _out(sess, n * b)
    check(sess.lib.alq_cosine_sims(sess.ctx, _ptr(dA), n, _ptr(dB), b, f, _ptr(na), _ptr(nb), _ptr(out)))
    sess.torch.cuda.synchronize()
    assert _tail_ok(out, n * b), 'write behind d_C'
    return out[:n * b].view(n, b)


def _half_ulp(x):
    return Fraction(float(np.spacing(abs(x)))) / 2


def _interval_miss(lo, hi, exact):
    """Distance from `exact` to the interval [lo, hi] (0 inside), as a Fraction."""
    return max(Fraction(0), lo - exact, exact - hi)


def _exact_ints(A):
    """fp32 array -> Python integers x * 2^149 (exact for every finite fp32), as an object array."""
    return np.array([int(Fraction(float(x)) * (1 << 149)) for x in A.reshape(-1)], dtype=object).reshape(A.shape)


SCALE2 = 1 << 298


# ------------------------------------------------------------------------------------------------ alq_row_norms
def test_row_norms_integer_features(sess):
    """The squared sum is exact, so the result is sqrt of it, correctly rounded: at most one ulp apart is allowed, the count of
    entries that differ at all and the largest difference are printed.  A zero row gives exactly 0.0."""
    worst, differ, total = 0, 0, 0
    for n, _, f in R.SIM_CASES:
        A = R.int_features(n, f, 100 + n)
        A[n // 2] = 0
        got = _row_norms(sess, _feat(sess, A), n, f).cpu().numpy()
        want = np.sqrt((A.astype(np.int64) ** 2).sum(1).astype(np.float64))
        np.testing.assert_array_equal(want, R.row_norms_ref(A))
        d = _ulps(got, want)
        worst, differ, total = max(worst, int(d.max())), differ + int((d > 0).sum()), total + n
        assert got[n // 2] == 0.0 and not np.signbit(got[n // 2])
        assert d.max() <= ROW_NORM_ULP_ALLOWED, (n, f, int(d.max()))
    print('alq_row_norms, integer features: %d of %d entries differ from sqrt(exact sum), largest difference %d ulp' % (differ, total, worst))


@pytest.mark.parametrize('n,f', [(5, 1), (65, 17), (64, 63), (7, 64), (9, 65), (257, 70)])
def test_row_norms_random_features_within_the_summation_bound(sess, n, f):
    rs = np.random.RandomState(n * 131 + f)
    A = (rs.randn(n, f) * np.exp(rs.randn(n, 1) * 3)).astype(np.float32)
    got = _row_norms(sess, _feat(sess, A), n, f).cpu().numpy()
    Ai = _exact_ints(A)
    worst = 0.0
    for i in range(n):
        s = Fraction(int((Ai[i] * Ai[i]).sum()), SCALE2)                           # the exact sum of squares
        g, h = Fraction(float(got[i])), _half_ulp(got[i])
        miss = _interval_miss((g - h) ** 2, (g + h) ** 2, s)                       # what the device accumulated lies in here
        worst = max(worst, float(miss / (f * Fraction(U) * s)))
        assert miss <= f * Fraction(U) * s, (i, float(miss / s))
    print('alq_row_norms random n=%d f=%d: largest miss / bound %.3f' % (n, f, worst))


# ------------------------------------------------------------------------------------------------ alq_cosine_sims
@pytest.mark.parametrize('n,b,f', R.SIM_CASES, ids=lambda v: str(v))
def test_plain_dots_integer_features(sess, n, b, f):
    A, B = R.int_features(n, f, 200 + n), R.int_features(b, f, 300 + b)
    got = _cosine(sess, _feat(sess, A), n, _feat(sess, B), b, f, None, None).cpu().numpy()
    np.testing.assert_array_equal(got, R.dots_ref(A, B))


@pytest.mark.parametrize('n,b,f', R.SIM_CASES, ids=lambda v: str(v))
def test_cosine_integer_features_bit_exact(sess, n, b, f):
    """dots are exact; the quotient by the product of the device's own norms is two IEEE operations on either side."""
    A, B = R.int_features(n, f, 400 + n, nonzero_rows=True), R.int_features(b, f, 500 + b, nonzero_rows=True)
    dA, dB = _feat(sess, A), _feat(sess, B)
    na, nb = _row_norms(sess, dA, n, f), _row_norms(sess, dB, b, f)
    got = _cosine(sess, dA, n, dB, b, f, na, nb).cpu().numpy()
    want = R.cosine_ref(A, B, na.cpu().numpy(), nb.cpu().numpy())
    d = _ulps(got, want)
    print('alq_cosine_sims integer (%d, %d, %d): %d of %d entries differ, largest %d ulp' % (n, b, f, int((d > 0).sum()), d.size, int(d.max())))
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize('n,b,f', [(5, 16, 1), (65, 65, 17), (64, 63, 70), (70, 15, 64)])
def test_cosine_random_features_within_the_summation_bound(sess, n, b, f):
    """got = fl(acc / fl(na nb)) with the device's norms: acc lies in [(got -+ ulp / 2) fl(na nb)], and that interval must reach
    within f 2^-53 sum |a||b| of the exact dot product."""
    rs = np.random.RandomState(n * 977 + b * 31 + f)
    A = (rs.randn(n, f) * np.exp(rs.randn(n, 1))).astype(np.float32)
    B = (rs.randn(b, f) * np.exp(rs.randn(b, 1))).astype(np.float32)
    dA, dB = _feat(sess, A), _feat(sess, B)
    na, nb = _row_norms(sess, dA, n, f), _row_norms(sess, dB, b, f)
    got = _cosine(sess, dA, n, dB, b, f, na, nb).cpu().numpy()
    na, nb = na.cpu().numpy(), nb.cpu().numpy()
    Ai, Bi = _exact_ints(A), _exact_ints(B)
    dots, absd = Ai @ Bi.T, np.abs(Ai) @ np.abs(Bi).T
    worst = 0.0
    for i in range(n):
        for j in range(b):
            p = Fraction(float(na[i] * nb[j]))
            g, h = Fraction(float(got[i, j])), _half_ulp(got[i, j])
            bound = f * Fraction(U) * Fraction(int(absd[i, j]), SCALE2)
            miss = _interval_miss((g - h) * p, (g + h) * p, Fraction(int(dots[i, j]), SCALE2))
            worst = max(worst, float(miss / bound))
            assert miss <= bound, (i, j, float(miss / bound))
    print('alq_cosine_sims random (%d, %d, %d): largest miss / bound %.3f' % (n, b, f, worst))


@pytest.mark.parametrize('n,f', [(5, 1), (65, 17), (64, 64), (257, 70)])
def test_cosine_of_a_matrix_with_itself_has_a_unit_diagonal(sess, n, f):
    rs = np.random.RandomState(n + f)
    A = rs.randn(n, f).astype(np.float32)
    dA = _feat(sess, A)
    na = _row_norms(sess, dA, n, f)
    got = _cosine(sess, dA, n, dA, n, f, na, na).cpu().numpy()
    nh = na.cpu().numpy()
    bound = f * U * (A.astype(np.float64) ** 2).sum(1) / (nh * nh)
    dev = np.abs(np.diag(got) - 1.0)
    print('cosine diagonal n=%d f=%d: largest |diag - 1| / bound %.3f' % (n, f, (dev / bound).max()))
    assert (dev <= bound).all()
    np.testing.assert_array_equal(got, got.T)


def test_cosine_empty_sides_and_refusals(sess):
    from nnal_amd._lib import ALQ_EINVAL
    A = R.int_features(5, 16, 1, nonzero_rows=True)
    dA = _feat(sess, A)
    na = _row_norms(sess, dA, 5, 16)
    out = _out(sess, 25)
    for n, b in ((0, 5), (5, 0), (0, 0)):
        assert sess.lib.alq_cosine_sims(sess.ctx, _ptr(dA), n, _ptr(dA), b, 16, _ptr(na), _ptr(na), _ptr(out)) == 0
        assert sess.lib.alq_cosine_sims(sess.ctx, None, n, None, b, 16, None, None, None) == 0
    assert sess.lib.alq_row_norms(sess.ctx, None, 0, 16, None) == 0
    for a_, b_ in ((na, None), (None, na)):
        assert sess.lib.alq_cosine_sims(sess.ctx, _ptr(dA), 5, _ptr(dA), 5, 16, _ptr(a_), _ptr(b_), _ptr(out)) == ALQ_EINVAL
        assert 'alq_cosine_sims' in sess.lib.alq_last_error().decode()
    assert sess.lib.alq_cosine_sims(sess.ctx, _ptr(dA), 5, _ptr(dA), 5, 0, None, None, _ptr(out)) == ALQ_EINVAL
    assert sess.lib.alq_cosine_sims(sess.ctx, _ptr(dA), 5, _ptr(dA), 5, 16, None, None, None) == ALQ_EINVAL
    sess.torch.cuda.synchronize()
    assert _tail_ok(out, 0)


# ------------------------------------------------------------------------------------------------ alq_colsum_max
def _colsum(sess, dS, n, b, cmax, skip):
    from nnal_amd._lib import check
    torch = sess.torch
    wb = sess.lib.alq_colsum_work_bytes(n, b)
    assert wb == ((n + 255) // 256) * b * 8
    work = torch.full((wb + 256,), 0xA5, dtype=torch.uint8, device=sess.device)
    out = _out(sess, b)
    check(sess.lib.alq_colsum_max(sess.ctx, _ptr(dS), n, b, _ptr(cmax), _ptr(skip), _ptr(out), _ptr(work)))
    torch.cuda.synchronize()
    assert _tail_ok(out, b), 'write behind d_out'
    assert bool((work[wb:] == 0xA5).all()), 'write behind the work buffer'
    return out[:b].cpu().numpy()


def _skip_patterns(n, seed):
    rs = np.random.RandomState(seed)
    z = np.zeros(n, np.uint8)
    first, last, chunk = z.copy(), z.copy(), z.copy()
    first[0], last[n - 1] = 1, 255
    chunk[:256] = 1
    return [('none', z), ('all', np.ones(n, np.uint8)), ('row 0', first), ('row n-1', last), ('first chunk', chunk),
            ('random', (rs.rand(n) < 0.4).astype(np.uint8) * rs.randint(1, 256, size=n).astype(np.uint8))]


@pytest.mark.parametrize('n,b', [c[:2] for c in R.SIM_CASES], ids=lambda v: str(v))
def test_colsum_max_dyadic_all_forms(sess, n, b):
    S, cmax = R.dyadic((n, b), 600 + n + b), R.dyadic((n,), 700 + n)
    dS, dc = _sim(sess, S), _dev(sess, cmax, R_CS + 64)
    for cm, dcm in ((None, None), (cmax, dc)):
        np.testing.assert_array_equal(_colsum(sess, dS, n, b, dcm, None), R.colsum_max_ref(S, cm, None))
        for name, skip in _skip_patterns(n, n * 7 + b):
            got = _colsum(sess, dS, n, b, dcm, _dev(sess, skip, R_CS + 64))
            np.testing.assert_array_equal(got, R.colsum_max_ref(S, cm, skip), err_msg='skip: %s, cmax %s' % (name, cm is not None))
            if name == 'all' or (name == 'first chunk' and n <= 256):
                assert (got == 0).all() and not np.signbit(got).any()


@pytest.mark.parametrize('n,b', [(513, 257), (65, 64), (1000, 70)])
def test_colsum_max_repeats_bit_for_bit(sess, n, b):
    """The header's "fixed summation order", on random fp64 S where the order matters; and within the summation bound of fp64."""
    rs = np.random.RandomState(n + b)
    S, cmax = rs.randn(n, b), rs.randn(n) * 0.3
    skip = (rs.rand(n) < 0.2).astype(np.uint8)
    dS, dc, dk = _sim(sess, S), _dev(sess, cmax, R_CS + 64), _dev(sess, skip, R_CS + 64)
    for dcm, cm, dsk, sk in ((None, None, None, None), (dc, cmax, None, None), (dc, cmax, dk, skip)):
        a = _colsum(sess, dS, n, b, dcm, dsk)
        for _ in range(3):
            np.testing.assert_array_equal(_colsum(sess, dS, n, b, dcm, dsk).view(np.uint64), a.view(np.uint64))
        T = np.abs(S if cm is None else np.maximum(cm[:, None], S))
        np.testing.assert_allclose(a, R.colsum_max_ref(S, cm, sk), rtol=0, atol=2 * n * U * T.sum(0).max())


def test_colsum_max_refusals(sess):
    from nnal_amd._lib import ALQ_EINVAL
    dS, out, work = _sim(sess, R.dyadic((4, 4), 1)), _out(sess, 4), _out(sess, 4)
    for args in ((None, 4, 4, None, None, _ptr(out), _ptr(work)), (_ptr(dS), 0, 4, None, None, _ptr(out), _ptr(work)),
                 (_ptr(dS), 4, 0, None, None, _ptr(out), _ptr(work)), (_ptr(dS), 4, 4, None, None, None, _ptr(work)),
                 (_ptr(dS), 4, 4, None, None, _ptr(out), None)):
        assert sess.lib.alq_colsum_max(sess.ctx, *args) == ALQ_EINVAL


# ------------------------------------------------------------------------------------------------ alq_take_colmax
@pytest.mark.parametrize('n,b', [(513, 257), (65, 65), (5, 1), (257, 256)])
def test_take_colmax(sess, n, b):
    from nnal_amd._lib import ALQ_EINVAL, check
    torch = sess.torch
    S = R.dyadic((n, b), 800 + n)
    dS = _sim(sess, S)
    v0 = R.dyadic((n,), 900 + n) * 0.5
    for j in sorted(set(j for j in (0, b - 1, 64, 255, 256) if j < b)):
        # first != 0 overwrites: the start above all of S must not survive (this is the case that catches a kernel that always takes
        # fmax; the NaN start only shows that no entry is left unwritten, fmax(NaN, s) being s either way)
        for first, start in ((1, np.full(n, np.nan)), (1, np.full(n, 100.0)), (7, np.full(n, 100.0)), (0, v0)):
            dv = _out(sess, n)
            dv[:n] = torch.from_numpy(start).to(sess.device)
            check(sess.lib.alq_take_colmax(sess.ctx, _ptr(dS), n, b, j, first, _ptr(dv)))
            torch.cuda.synchronize()
            assert _tail_ok(dv, n)
            got = dv[:n].cpu().numpy()
            assert not np.isnan(got).any()                                           # first: every entry overwritten
            np.testing.assert_array_equal(got, R.take_colmax_ref(S, j, first, start), err_msg='j=%d first=%d' % (j, first))
    np.testing.assert_array_equal(dS.cpu().numpy(), S)
    dv = _out(sess, n)
    for j in (b, -1, b + 64):
        assert sess.lib.alq_take_colmax(sess.ctx, _ptr(dS), n, b, j, 0, _ptr(dv)) == ALQ_EINVAL
    torch.cuda.synchronize()
    assert _tail_ok(dv, 0)


# ------------------------------------------------------------------------------------------------ alq_fold_rowmax
def _fold(sess, dS, t, n, v):
    from nnal_amd._lib import check
    torch = sess.torch
    dv = _out(sess, n)
    dv[:n] = torch.from_numpy(np.ascontiguousarray(v)).to(sess.device)
    check(sess.lib.alq_fold_rowmax(sess.ctx, _ptr(dS), t, n, _ptr(dv)))
    torch.cuda.synchronize()
    assert _tail_ok(dv, n)
    return dv[:n].cpu().numpy()


@pytest.mark.parametrize('t', [1, 2, 333])
@pytest.mark.parametrize('n', [1, 255, 257, 513])
def test_fold_rowmax(sess, t, n):
    """The running vector mixes -inf, values above every column maximum and values below it, so a kernel that ignored v[j], or
    that always took it, fails."""
    S = R.dyadic((t, n), 1000 + t + n)
    v = np.full(n, -np.inf)
    v[1::3] = S.max(0)[1::3] + 0.5
    v[2::3] = S.max(0)[2::3] - 0.5
    want = R.fold_rowmax_ref(S, v)
    if n >= 3:
        assert (want == v).any() and (want != v).any() and np.isfinite(want).all()
    dS = _sim(sess, S)
    np.testing.assert_array_equal(_fold(sess, dS, t, n, v), want)
    np.testing.assert_array_equal(dS.cpu().numpy(), S)
    if t >= 2:                                                   # two blocks one after the other = their concatenation
        h = t // 2
        mid = _fold(sess, _sim(sess, S[:h]), h, n, v)
        np.testing.assert_array_equal(mid, R.fold_rowmax_ref(S[:h], v))
        np.testing.assert_array_equal(_fold(sess, _sim(sess, S[h:]), t - h, n, mid), want)


# ------------------------------------------------------------------------------------------------ non-finite inputs (pinned)
def test_zero_norm_rows_give_nan_rows_and_columns(sess):
    """0 / (0 * nb) is NaN: a zero feature vector has no cosine, and the kernel says so like the reference's NumPy does."""
    n, b, f = 65, 66, 17
    A, B = R.int_features(n, f, 1, nonzero_rows=True), R.int_features(b, f, 2, nonzero_rows=True)
    A[[0, 64]] = 0
    B[[3, 65]] = 0
    dA, dB = _feat(sess, A), _feat(sess, B)
    na, nb = _row_norms(sess, dA, n, f), _row_norms(sess, dB, b, f)
    got = _cosine(sess, dA, n, dB, b, f, na, nb).cpu().numpy()
    nan = np.zeros((n, b), bool)
    nan[[0, 64], :] = True
    nan[:, [3, 65]] = True
    np.testing.assert_array_equal(np.isnan(got), nan)
    with np.errstate(invalid='ignore'):
        want = R.cosine_ref(A, B, na.cpu().numpy(), nb.cpu().numpy())
    np.testing.assert_array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))
    np.testing.assert_array_equal(np.isnan(want), nan)


def test_max_kernels_follow_fmax_and_ignore_a_nan_operand(sess):
    """Pinned, not judged: fmax(NaN, x) = x on the device, where the reference's np.max / np.maximum give NaN."""
    from nnal_amd._lib import check
    torch = sess.torch
    n, b = 300, 5
    S, cmax = R.dyadic((n, b), 1), R.dyadic((n,), 2)
    Sn, cn = S.copy(), cmax.copy()
    Sn[7, 1] = Sn[299, 4] = np.nan
    cn[7] = cn[100] = np.nan
    # colsum: NaN cmax -> the S entry; NaN S entry under a cmax -> the cmax; both NaN -> NaN; without cmax the sum is NaN
    dSn, dcn = _sim(sess, Sn), _dev(sess, cn, R_CS + 64)
    got = _colsum(sess, dSn, n, b, dcn, None)
    want = np.fmax(cn[:, None], Sn).sum(0)
    np.testing.assert_array_equal(got, want)
    assert np.isnan(got[1]) and not np.isnan(got[[0, 2, 3, 4]]).any()
    assert np.isnan(R.colsum_max_ref(Sn, cn, None)).all()                           # the reference's NumPy: every column NaN
    plain = _colsum(sess, dSn, n, b, None, None)
    np.testing.assert_array_equal(np.isnan(plain), [False, True, False, False, True])
    # take_colmax
    for j in (1, 4):
        dv = _out(sess, n)
        dv[:n] = torch.from_numpy(cn).to(sess.device)
        check(sess.lib.alq_take_colmax(sess.ctx, _ptr(dSn), n, b, j, 0, _ptr(dv)))
        np.testing.assert_array_equal(dv[:n].cpu().numpy(), np.fmax(cn, Sn[:, j]))
        assert np.isnan(np.maximum(cn, Sn[:, j])).sum() > np.isnan(np.fmax(cn, Sn[:, j])).sum()
    dv = _out(sess, n)
    check(sess.lib.alq_take_colmax(sess.ctx, _ptr(dSn), n, b, 1, 1, _ptr(dv)))
    np.testing.assert_array_equal(dv[:n].cpu().numpy(), Sn[:, 1])                    # first: a copy, NaN included
    # fold_rowmax: a [t, n] block
    T = R.dyadic((4, 9), 3)
    v = R.dyadic((9,), 4)
    T[2, 1] = T[0, 5] = np.nan
    T[:, 7] = np.nan
    v[5] = v[6] = np.nan
    got = _fold(sess, _sim(sess, T), 4, 9, v)
    np.testing.assert_array_equal(got, np.fmax(v, np.fmax.reduce(T, axis=0)))
    assert not np.isnan(got).any() and got[7] == v[7]
    assert np.isnan(R.fold_rowmax_ref(T, v)[[1, 5, 6, 7]]).all()
    v[7] = np.nan
    assert np.isnan(_fold(sess, _sim(sess, T), 4, 9, v)[7])                          # nothing but NaN: NaN


# ------------------------------------------------------------------------------------------------ whole queries across the edges
def _big_setup(sess, B):
    """tests/test_gpu_strategies._setup (net_b_small, 5x5x3 patches, its stats) on volumes and index sets large enough to cross the
    64-column tile, the 256-row chunk and the 1000-row labelled batch: subject 1 is 12 x 12 x 8 with 1001 labelled voxels."""
    expr, model, _, _, _ = _setup(sess)
    rs = np.random.RandomState(181)
    vols = []
    for shp in ((9, 10, 8), (12, 12, 8)):
        mods = [np.pad(rs.randn(*shp), [(2, 2), (2, 2), (1, 1)], 'constant') for _ in range(2)]
        vols.append(mods + [rs.randint(0, 2, size=shp)])
    pools = [np.sort(rs.permutation(720)[:230]), np.sort(rs.permutation(1152)[:150])]
    labeled = [np.sort(rs.permutation(720)[:30]), np.sort(rs.permutation(1152)[:1001])]
    expr.pars['B'] = B
    return expr, model, vols, pools, labeled


def test_rep_entropy_across_the_tile_and_chunk_edges(sess):
    from nnal_amd import PW_NNAL, patch_utils
    B = 70
    expr, model, vols, pools, labeled = _big_setup(sess, B)
    got = PW_NNAL.query_multimg(expr, model, sess, vols, pools, labeled, 'rep-entropy')
    F = _feats(expr, model, sess, vols, pools)
    k = expr.pars['k']
    sel_inds, _ = PW_NNAL.bin_uncertainty_filter_multimg(expr, model, sess, vols, pools, B)
    F_unc = np.concatenate([F[i][:, sel_inds[i]] for i in range(2) if len(sel_inds[i]) > 0], axis=1)
    F_rem = np.concatenate([F[i][:, np.setdiff1d(np.arange(len(pools[i])), sel_inds[i])] for i in range(2)], axis=1)
    f, nR = F_rem.shape
    assert F_unc.shape[1] == B > 64 and nR >= 300 > 256
    nr, nu = np.sqrt((F_rem ** 2).sum(0)), np.sqrt((F_unc ** 2).sum(0))
    assert nr.min() > 0 and nu.min() > 0
    sims = (F_rem.T @ F_unc) / np.outer(nr, nu)
    # a score is a sum of nR entries of magnitude <= 1, each off by at most (f + 3) 2^-53 of sum |a||b| / (na nb) <= 1 on either
    # side, summed in some order: two scores compare safely when they differ by more than twice this
    bound = 2 * (nR + 2 * (f + 3)) * U * nR
    Q, nQ = [], np.arange(B)
    for i in range(k):
        rep = np.array([np.sum(np.max(sims[:, Q + [nQ[j]]], axis=1)) for j in range(B - i)])
        top = np.sort(rep)[::-1]
        assert top[0] - top[1] > bound, (i, top[0] - top[1], bound)
        Q += [nQ[np.argmax(rep)]]
        nQ = np.delete(nQ, np.argmax(rep))
    local = patch_utils.global2local_inds(Q, [len(s_) for s_ in sel_inds])
    want = [np.array(sel_inds[i])[local[i]] for i in range(2)]
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert sum(len(a) for a in got) == k
    model.close()


def test_core_set_with_two_labelled_batches(sess):
    from nnal_amd import NN, PW_NNAL, patch_utils
    expr, model, vols, pools, labeled = _big_setup(sess, 70)
    assert len(labeled[1]) == 1001 and len(list(NN.gen_batch_inds(1001, 1000))) == 2
    np.random.seed(5)
    got = PW_NNAL.query_multimg(expr, model, sess, vols, pools, labeled, 'core-set')
    F_u = np.concatenate(_feats(expr, model, sess, vols, pools), axis=1)
    F_T = _feats(expr, model, sess, vols, labeled, 'labeled_stats')[1]
    f = F_u.shape[0]
    assert F_T.shape[1] == 1001 and F_u.shape[1] > 256
    norms_u = np.sqrt((F_u ** 2).sum(0))
    assert norms_u.min() > 0 and (F_T ** 2).sum(0).min() > 0
    sims = np.max((F_T.T @ F_u) / np.outer(np.sqrt((F_T ** 2).sum(0)), norms_u), axis=0)
    # every entry is one cosine, off by at most (f + 3) 2^-53 on either side: the minimum is safe when the runner-up is further
    bound = 2 * 2 * (f + 3) * U
    Q = []
    for step in range(expr.pars['k']):
        low = np.sort(sims)
        assert low[1] - low[0] > bound, (step, low[1] - low[0], bound)
        q = int(np.argmin(sims))
        Q.append(q)
        sims = np.maximum(sims, (F_u[:, q] @ F_u) / (norms_u * norms_u[q]))
        sims[q] = np.inf
    want = patch_utils.global2local_inds(Q, [len(p) for p in pools])
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    model.close()
