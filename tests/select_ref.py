"""References and case tables for the two kernel families that end a query: the top-B sort (csrc/topk.hip) and the similarity
kernels of the representativeness strategies (csrc/sim.hip).  NumPy only: tests/test_select_ref_host.py holds every function and
table here to its own statement without a GPU, tests/test_gpu_topk.py and tests/test_gpu_sim.py compare the kernels with them.

The sort order is written from the contract in include/alq.h (alq_topk_uncertain), not from the kernel:
    numeric order for either sign; -0.0 immediately before +0.0; a NaN with the sign bit clear after +inf; a NaN with the sign
    bit set before -inf; ties -> lower index.
As a map to uint64: split the 64 bits into sign and magnitude m (the low 63 bits, which order |x| for every double, with inf above
every number and the NaNs above inf).  A sign-clear key goes to 2^63 + m, a sign-set key to 2^63 - 1 - m: the two halves meet at
-0.0 -> 2^63 - 1, +0.0 -> 2^63.  Nothing maps above 2^64 - 1, the key of the sort's padding entries, and exactly one input maps ONTO
it: the NaN 0x7FFFFFFFFFFFFFFF, which only its index (below the padding index ~0) keeps ahead of the padding."""
import functools

import numpy as np

PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
_HALF = np.uint64(1 << 63)
_MAG = np.uint64((1 << 63) - 1)
CHUNK = 2048                      # pairs per workgroup of the bitonic sort; also its smallest padded size


def order_key(keys):
    """uint64 sort keys of float64 `keys`: ascending uint64 order is the order include/alq.h promises (see the module text)."""
    u = np.ascontiguousarray(keys, dtype=np.float64).view(np.uint64)
    m = u & _MAG
    return np.where((u >> np.uint64(63)) != 0, _MAG - m, _HALF + m)


def topk_ref(keys, B):
    k = order_key(keys)
    return np.lexsort((np.arange(len(k)), k))[:int(B)].astype(np.int64)


def padded_size(n):
    p = CHUNK
    while p < n:
        p <<= 1
    return p


# ------------------------------------------------------------------------------------------------ top-B case tables
TOPK_N = (1, 2, 3, 255, 2047, 2048, 2049, 4095, 4096, 4097, 6149, 8192, 8193, 16385, (1 << 17) + 1)
TOPK_N_BIG = (1 << 21) + 1        # P = 2^22: the grid-stride loops of topk_init_kernel / bitonic_global_kernel iterate twice
TOPK_B_BIG = (1, 4096)


def topk_Bs(n):
    if n == TOPK_N_BIG:
        return list(TOPK_B_BIG)
    return sorted(set([0, 1, min(n, 700), n]))


TOPK_SIZES = [(n, B) for n in TOPK_N + (TOPK_N_BIG,) for B in topk_Bs(n)]

# special doubles by bit pattern; NAN_PAD maps onto the padding key
NAN_PAD = 0x7FFFFFFFFFFFFFFF
SPECIAL_BITS = (
    NAN_PAD,
    0x0000000000000000, 0x8000000000000000,                      # +0.0, -0.0
    0x7FF0000000000000, 0xFFF0000000000000,                      # +inf, -inf
    0x7FF8000000000000, 0xFFF8000000000000,                      # quiet NaN of either sign
    0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,                      # the smallest sign-clear NaN payload, the largest sign-set one
    0x0000000000000001, 0x8000000000000001,                      # smallest denormals
    0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,                      # largest denormals
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,                      # +-DBL_MAX
)


def _distinct(n, seed):
    """n distinct doubles of both signs in random order (distinct by construction: |x| = rank + a fraction below 1)."""
    rs = np.random.RandomState(seed)
    mag = (np.arange(n) + rs.rand(n) * 0.5 + 0.25) * 1e-3
    sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    return (mag * sign)[rs.permutation(n)]


def _few_values(n, seed):
    rs = np.random.RandomState(seed)
    return np.array([-1.5, -0.25, 0.0, 0.25, 3.0])[rs.randint(0, 5, size=n)]


def _all_equal(n, seed):
    return np.full(n, 0.125)


def _ascending(n, seed):
    return np.sort(_distinct(n, seed))


def _descending(n, seed):
    return np.sort(_distinct(n, seed))[::-1].copy()


def special_positions(n):
    """Positions of the `specials` set: 0, n - 1 and both sides of every 2048 boundary inside [0, n), then random others until
    there are twice as many as SPECIAL_BITS has entries."""
    pos = [0, n - 1]
    for b in range(CHUNK, n, CHUNK):
        pos += [b - 1, b]
    pos = [p for p in dict.fromkeys(pos) if 0 <= p < n]
    rs = np.random.RandomState(n % 100003)
    want = min(n, max(len(pos), 2 * len(SPECIAL_BITS)))
    for p in rs.permutation(n):
        if len(pos) >= want:
            break
        if p not in pos:
            pos.append(int(p))
    return pos


def _specials(n, seed):
    k = _distinct(n, seed).view(np.uint64).copy()
    pos = special_positions(n)
    # NAN_PAD at the last position (next to the padding), the others cycled over the rest
    k[pos[1 if len(pos) > 1 else 0]] = np.uint64(NAN_PAD)
    rest = [p for p in pos if p != n - 1] if len(pos) > 1 else []
    for i, p in enumerate(rest):
        k[p] = np.uint64(SPECIAL_BITS[1 + i % (len(SPECIAL_BITS) - 1)])
    return k.view(np.float64)


def absdev_posts(n, seed):
    """fp32 posteriors with exact 0.5, 0, 1 and duplicated values, as a pool sweep returns them."""
    rs = np.random.RandomState(seed)
    p = rs.rand(n).astype(np.float32)
    p[rs.randint(0, n, size=max(1, n // 8))] = p[rs.randint(0, n, size=max(1, n // 8))]     # duplicates
    for v in (0.5, 0.0, 1.0):
        p[rs.randint(0, n, size=max(1, n // 50))] = v
    return p


def _absdev(n, seed):
    return np.abs(absdev_posts(n, seed).astype(np.float64) - 0.5)


KEY_SETS = {'distinct': _distinct, 'few_values': _few_values, 'all_equal': _all_equal, 'descending': _descending,
            'ascending': _ascending, 'specials': _specials, 'absdev': _absdev}
KEY_SET_NAMES = tuple(KEY_SETS)


def _keys(name, n):
    k = KEY_SETS[name](n, 1000 + n % 9973)
    k.setflags(write=False)
    return k


def _full_order(name, n):
    o = topk_ref(topk_keys(name, n), n)
    o.setflags(write=False)
    return o


_keys_cached = functools.lru_cache(maxsize=None)(_keys)
_full_order_cached = functools.lru_cache(maxsize=None)(_full_order)


def topk_keys(name, n):
    """The keys of one (key set, n): built once and shared, read-only (the 2^21 + 1 case is rebuilt instead of kept)."""
    return (_keys_cached if n < TOPK_N_BIG else _keys)(name, n)


def topk_full_order(name, n):
    """The whole reference order of one (key set, n), computed once and shared by every B."""
    return (_full_order_cached if n < TOPK_N_BIG else _full_order)(name, n)


def topk_cases():
    """(n, B, key set) rows of the order test: every n meets every key set, every (n, B) of TOPK_SIZES appears, every key set meets
    B = n at a padded n (the rotation by the n's rank does it; tests/test_select_ref_host.py checks the three properties)."""
    rows = []
    for i, n in enumerate(TOPK_N + (TOPK_N_BIG,)):
        Bs = topk_Bs(n)
        for s, name in enumerate(KEY_SET_NAMES):
            rows.append((n, Bs[(s + i) % len(Bs)], name))
    return rows


# ------------------------------------------------------------------------------------------------ similarity references (fp64)
def row_norms_ref(A):
    A = np.asarray(A, dtype=np.float64)
    return np.sqrt((A * A).sum(axis=1))


def dots_ref(A, B):
    return np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64).T


def cosine_ref(A, B, na, nb):
    return dots_ref(A, B) / (np.asarray(na, dtype=np.float64)[:, None] * np.asarray(nb, dtype=np.float64)[None, :])


def colsum_max_ref(S, cmax=None, skip=None):
    """out[j] = sum_i max(cmax[i], S[i, j]) over the rows with skip[i] == 0 (cmax None: S[i, j]; skip None: every row)."""
    S = np.asarray(S, dtype=np.float64)
    T = S if cmax is None else np.maximum(np.asarray(cmax, dtype=np.float64)[:, None], S)
    if skip is not None:
        T = T[np.asarray(skip) == 0]
    return T.sum(axis=0) if len(T) else np.zeros(S.shape[1])


def take_colmax_ref(S, j, first, v):
    S = np.asarray(S, dtype=np.float64)
    return S[:, j].copy() if first else np.maximum(np.asarray(v, dtype=np.float64), S[:, j])


def fold_rowmax_ref(S, v):
    return np.maximum(np.asarray(v, dtype=np.float64), np.asarray(S, dtype=np.float64).max(axis=0))


# ------------------------------------------------------------------------------------------------ exact input builders
INT_MAX = 8


def int_features(n, f, seed, nonzero_rows=False):
    """fp32 [n, f] features that are integers with |x| <= 8.  Every product is an integer <= 64 and every partial sum of a row's
    squares or of a dot product is an integer <= 64 f < 2^53 (asserted): any summation order gives the same double."""
    rs = np.random.RandomState(seed)
    A = rs.randint(-INT_MAX, INT_MAX + 1, size=(n, f)).astype(np.float32)
    if nonzero_rows:
        z = ~A.any(axis=1)
        A[z, 0] = 1.0 + (np.arange(n)[z] % INT_MAX)
    assert_int_exact(A)
    return A


def assert_int_exact(A):
    A = np.asarray(A)
    assert A.dtype == np.float32 and np.array_equal(A, np.rint(A)) and np.abs(A).max(initial=0) <= INT_MAX
    assert INT_MAX * INT_MAX * A.shape[1] < 2 ** 53


DYADIC_ONE = 1024                 # entries are multiples of 2^-10
DYADIC_MAX = 4


def dyadic(shape, seed):
    """float64 multiples of 2^-10 with |x| <= 4: a sum of up to 2^20 of them is a multiple of 2^-10 below 2^22, exact in any order."""
    rs = np.random.RandomState(seed)
    S = rs.randint(-DYADIC_MAX * DYADIC_ONE, DYADIC_MAX * DYADIC_ONE + 1, size=shape).astype(np.float64) / DYADIC_ONE
    assert_dyadic_exact(S, int(np.prod(shape[:1])))
    return S


def assert_dyadic_exact(S, rows):
    S = np.asarray(S, dtype=np.float64)
    assert np.array_equal(S * DYADIC_ONE, np.rint(S * DYADIC_ONE)) and np.abs(S).max(initial=0) <= DYADIC_MAX
    assert rows <= 2 ** 20 and rows * DYADIC_MAX * DYADIC_ONE < 2 ** 53


# ------------------------------------------------------------------------------------------------ similarity size tables
SIM_N = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)      # row_norm_kernel's 4 rows per block, the 64-row tile, colsum's 256-row chunks
SIM_B = (1, 15, 16, 63, 64, 65, 256, 257)                 # the 64-column tile, colsum's 256-column blocks
SIM_F = (1, 15, 16, 17, 63, 64, 65, 70)                   # the 16-deep K slice, the 64-lane row loop
_EDGE = (63, 64, 65)


def sim_cases():
    """Covering table of (n, b, f): every value of each list, every (n, b) of {63, 64, 65}^2, and 513 x 257 - not the product."""
    nb = [(n, b) for n in _EDGE for b in _EDGE] + [(513, 257)]
    nb += [(1, 256), (3, 15), (4, 16), (5, 1), (255, 257), (256, 256), (257, 16)]
    return [(n, b, SIM_F[i % len(SIM_F)]) for i, (n, b) in enumerate(nb)]


SIM_CASES = sim_cases()
