"""CPU references of a fully connected layer for tests/test_gpu_fcgemm.py, and NumPy emulators of the operand splits of the
streaming GEMM (csrc/fcgemm.hip).  No device and no library call in this file.

fp64 statement (W as TF holds it, [N units, K inputs]; a [M, K]; b [N]):
    out  = [relu](a @ W.T + b)
    din  = (dout @ W) * (a_prev > 0)         a_prev the output of the layer below; no mask when that layer is 'M'
    dW_s = outer(dout_s, a_s),  db_s = dout_s      per sample s; their sums over s for a summed gradient

Splits.  The engine writes every fp32 operand as a short sum of narrow pieces and keeps the piece products that matter:
  bf16 triples   x = hi + mid + lo, each piece x rounded to nearest even and subtracted (fc_bf16_rne on the host for the weights,
                 fc_split2 on the device for the activations, whose third piece is the remainder's upper 16 bits: it is exact by
                 then).  Kept: (mid, mid), (lo, hi), (hi, lo), (mid, hi), (hi, mid), (hi, hi)  [weight piece, activation piece] -
                 with the pieces numbered hi = 0, mid = 1, lo = 2 the pairs (i, j) with i + j <= 2.
  fp16 pairs     x 2^e = h + l with e = 14 - ex where max |x| < 2^ex: per row of the activations (fc_row_exp: clamped at 96, 0 for an
                 all-zero row; forward launches), from one static bound (backward launches of a Fisher pass), over the whole matrix
                 for the weights (fcgemm_pack_weights_f16).  Kept: (l, h), (h, l), (h, h).
`subset_eval` sums any chosen subset of piece products in fp64.

Exactness.  `assert_exact` checks, for given a, W, b and a form, the conditions under which the kernel's kept subset - summed in
any order in fp32 - equals the fp64 statement bit for bit:
  1. every piece product of an output (and its bias) is a multiple of one power of two q,
  2. the sum of their absolute values is below 2^24 q (every partial sum is then a multiple of q below 2^24 q: an fp32 number),
  3. no product outside the kept subset is non-zero, and the pieces add up to the operand.
`dense_ints` (|a|, |w|, |b| <= 15, K <= 512) and `probe_set` satisfy them for both forms; every builder asserts so."""
from collections import OrderedDict

import numpy as np

FC_BM, FC_BN, FC_BK = 128, 64, 32
PAIR_KEPT = ((1, 0), (0, 1), (0, 0))                                        # (weight piece, activation piece); h = 0, l = 1
TRIPLE_KEPT = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))            # hi = 0, mid = 1, lo = 2
KEPT = {'pairs': PAIR_KEPT, 'triples': TRIPLE_KEPT}
NPIECES = {'pairs': 2, 'triples': 3}


# ------------------------------------------------------------------------------------------ fp64 statement
def forward64(a, W, b, relu):
    y = np.asarray(a, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64).reshape(1, -1)
    return np.maximum(y, 0.) if relu else y


def din64(dout, W, a_prev=None):
    d = np.asarray(dout, np.float64) @ np.asarray(W, np.float64)
    return d if a_prev is None else d * (np.asarray(a_prev) > 0)


def wgrad64(a, dout):
    """Per-sample (dW [M, N, K], db [M, N])."""
    a, dout = np.asarray(a, np.float64), np.asarray(dout, np.float64)
    return dout[:, :, None] * a[:, None, :], dout.copy()


def forward_torch(a, W, b, relu, dtype):
    import torch
    y = torch.as_tensor(np.asarray(a)).to(dtype) @ torch.as_tensor(np.asarray(W)).to(dtype).t() + torch.as_tensor(np.asarray(b).reshape(1, -1)).to(dtype)
    return (torch.relu(y) if relu else y).numpy()


def din_torch(dout, W, a_prev, dtype):
    import torch
    d = torch.as_tensor(np.asarray(dout)).to(dtype) @ torch.as_tensor(np.asarray(W)).to(dtype)
    if a_prev is not None:
        d = d * torch.as_tensor(np.asarray(a_prev) > 0).to(dtype)
    return d.numpy()


def wgrad_torch(a, dout, dtype):
    import torch
    a, dout = torch.as_tensor(np.asarray(a)).to(dtype), torch.as_tensor(np.asarray(dout)).to(dtype)
    return (dout[:, :, None] * a[:, None, :]).numpy(), dout.numpy().copy()


# ------------------------------------------------------------------------------------------ geometry, as the issue's table states it
def geometry(K, N, M, form=0):
    """What alq_fcgemm_geometry must report: (wide, BN, tall, grid.x, grid.y, k-steps); form 0 / 1 / 2 = default / ALQ_FC_SQUARE /
    ALQ_FC_BN64."""
    if K % FC_BK or N % FC_BN or K < 256 or N < 256:
        return (0, 0, 0, 0, 0, 0)
    w128 = N % (2 * FC_BN) == 0 and form != 2
    bn = 2 * FC_BN if w128 else FC_BN
    return (1, bn, int(w128 and form == 0), N // bn, -(-M // FC_BM), K // FC_BK)


# ------------------------------------------------------------------------------------------ splits (bit operations)
def _f32(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x


def bf16_rne(x):
    """fc_bf16_rne followed by fc_bf16_to_f: x rounded to the nearest bf16 (ties to even), as a float32."""
    u = _f32(x).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffffffff
    return ((u >> 16) << 16).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_trunc(x):
    """fc_pack2: the upper 16 bits."""
    return (_f32(x).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32).reshape(np.shape(x))


def triples(x, device=False):
    """[3, ...] float64 pieces hi, mid, lo of fp32 x.  device = False: three roundings (fcgemm_pack_weights); True: two roundings and
    the upper half of what is left (fc_split2, fc_split2, fc_pack2)."""
    r = _f32(x).copy()
    out = []
    for p in range(3):
        h = bf16_trunc(r) if (device and p == 2) else bf16_rne(r)
        out.append(h.astype(np.float64))
        r = (r - h).astype(np.float32)
    return np.stack(out)


def row_exp(amax):
    """fc_row_exp on the float bits of a row maximum: the scale exponent of the row."""
    fm = _f32(amax).view(np.uint32).astype(np.int64)
    ex = ((fm >> 23) & 255) - 126
    ce = np.minimum(14 - ex, 96)
    return np.where(fm != 0, ce, 0).reshape(np.shape(amax))


def matrix_exp(W):
    """fcgemm_pack_weights_f16: 14 - ex with max |w| = f 2^ex, f in [0.5, 1); 14 for a zero matrix."""
    amax = float(np.abs(_f32(W)).max()) if np.size(W) else 0.
    return 14 - (int(np.frexp(np.float32(amax))[1]) if amax > 0 else 0)


def bound_exp(bound):
    """fcgemm_launch under a static bound: 14 - ex with bound = f 2^ex."""
    return 14 - int(np.frexp(np.float32(bound))[1])


def pairs(x, e):
    """[2, ...] float64 pieces h, l of fp32 x at scale 2^e (e a scalar or one exponent per row), divided by the scale again."""
    x = _f32(x)
    e = np.asarray(e, dtype=np.int64)
    e = e.reshape(e.shape + (1,) * (x.ndim - e.ndim))
    with np.errstate(over='ignore'):
        xs = (x * np.ldexp(np.float32(1), e).astype(np.float32)).astype(np.float32)      # the device multiplies by the fp32 scale
        h = xs.astype(np.float16)
        l = (xs - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    inv = np.ldexp(1., -e)
    return np.stack([h.astype(np.float64) * inv, l.astype(np.float64) * inv])


def split(a, W, form, a_exp=None):
    """(activation pieces [P, M, K], weight pieces [P, N, K]) of a form; a_exp: the activations' scale exponent(s) of the pair form
    (None: per row, the forward rule)."""
    if form == 'triples':
        return triples(a, device=True), triples(W)
    if a_exp is None:
        a_exp = row_exp(np.abs(_f32(a)).max(axis=1))
    return pairs(a, a_exp), pairs(W, matrix_exp(W))


def subset_eval(ap, wp, subset, weights=None):
    """sum over (i, j) in subset of weights[(i, j)] * ap[j] @ wp[i].T in fp64 (weights default 1)."""
    out = np.zeros((ap.shape[1], wp.shape[1]))
    for i, j in subset:
        out += (1. if weights is None else weights.get((i, j), 1.)) * (ap[j] @ wp[i].T)
    return out


# ------------------------------------------------------------------------------------------ exactness conditions
def _lowbit_exp(v):
    """Exponent of the lowest set bit of every non-zero float64 (+inf for zeros)."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)
    mi = np.abs(m * 2. ** 53).astype(np.int64)      # exact: 53-bit mantissa
    low = np.zeros(v.shape)
    nz = mi != 0
    low[nz] = np.log2((mi[nz] & -mi[nz]).astype(np.float64))
    return np.where(nz, e - 53 + low, np.inf)


def assert_exact(a, W, b, form, a_exp=None):
    """The three conditions of the module docstring for out = a @ W.T + b on `form`; returns the worst log2(sum |products| / q)
    (below 24).  q is taken per output as 2^(lowest bit of any piece of the row + lowest bit of any piece of the unit), the bias's
    lowest bit if lower: a power of two that divides every piece product of the output (not always the largest one: the
    condition asserted is the stricter for it)."""
    a, W = _f32(a), _f32(W)
    b = np.zeros(W.shape[0], np.float32) if b is None else _f32(b).reshape(-1)
    ap, wp = split(a, W, form, a_exp)
    P = NPIECES[form]
    assert np.array_equal(ap.sum(0), a.astype(np.float64)) and np.array_equal(wp.sum(0), W.astype(np.float64)), 'the pieces do not add up'
    kept = set(KEPT[form])
    for i, j in [(i, j) for i in range(P) for j in range(P) if (i, j) not in kept]:      # non-zero only where both pieces are
        hit = (ap[j] != 0).astype(np.float64) @ (wp[i] != 0).astype(np.float64).T
        assert not hit.any(), 'a product outside the kept subset is non-zero: weight piece %d, activation piece %d' % (i, j)
    S = np.abs(b.astype(np.float64))[None, :].repeat(a.shape[0], 0)
    for i, j in kept:
        S = S + np.abs(ap[j]) @ np.abs(wp[i]).T
    q = _lowbit_exp(ap).min(axis=(0, 2))[:, None] + _lowbit_exp(wp).min(axis=(0, 2))[None, :]
    q = np.minimum(q, _lowbit_exp(b.astype(np.float64))[None, :])
    nz = S > 0
    assert np.all(np.isfinite(q[nz]))
    r = np.log2(S[nz]) - q[nz]
    assert np.all(r < 24), 'sum |piece products| reaches 2^%.2f q' % r.max()
    return r.max() if r.size else -np.inf


# ------------------------------------------------------------------------------------------ inputs
def dense_ints(M, K, N, seed, bias=True):
    """Dense small integers: |a|, |w|, |b| <= 15, K <= 512: |out| <= 225 K + 15 < 2^17."""
    assert K <= 512
    rs = np.random.RandomState(seed)
    a = rs.randint(-15, 16, size=(M, K)).astype(np.float32)
    W = rs.randint(-15, 16, size=(N, K)).astype(np.float32)
    b = rs.randint(-15, 16, size=N).astype(np.float32) if bias else np.zeros(N, np.float32)
    for form in KEPT:
        assert_exact(a, W, b, form)
    return a, W, b


# element kinds of a probe: (bf16 pieces of the weight, of the activation); both numbers' ranges (odd integers, either sign).
# (1, 1): the (hi, hi) / (h, h) product alone.  (2, 2): 11 bits each: mid pieces on both sides, no l piece: (mid, mid), (mid, hi),
# (hi, mid).  (3, 1): an 18-bit weight whose lo piece is not zero (drawn until it is not) - (lo, hi) of the triples, (l, h) of the
# pairs - against 6 bits.  (1, 3): the mirror image.  Products stay below 2^24.
KINDS = OrderedDict([((1, 1), ((129, 255), (129, 255))), ((2, 2), ((1025, 2047), (1025, 2047))),
                     ((3, 1), ((2 ** 17 + 1, 2 ** 18 - 1), (33, 63))), ((1, 3), ((33, 63), (2 ** 17 + 1, 2 ** 18 - 1)))])
KS_CLASSES = ('first', 'middle', 'last')
NCLASS = len(KINDS) * 4 * 3      # kind x k-group q x k-step class = 48


def probe_class(c, K):
    """Class c = (kind * 4 + q) * 3 + ksc -> (kind index, q, ksc, the class's k index)."""
    kind, q, ksc = c // 12, (c // 3) % 4, c % 3
    nks = K // FC_BK
    ks = (0, nks // 2, nks - 1)[ksc]
    return kind, q, ksc, ks * FC_BK + q * 8 + (kind * 2 + ksc + q) % 8


def _odd(rs, lo, hi, size):
    """Odd integers of either sign in [lo, hi]; above 2^16 only those with three non-zero bf16 pieces."""
    v = rs.randint(lo // 2, hi // 2 + 1, size=8 * size + 64) * 2 + 1
    v = (v * rs.choice([-1, 1], size=v.size)).astype(np.float32)
    if lo > 2 ** 16:
        v = v[triples(v)[2] != 0]
    assert v.size >= size
    return v[:size]


def probe_set(M, K, N, seed, bias=False):
    """Sparse probes.  Row m (i = m % 16) holds one element of each class c = i, i + 16, i + 32; unit n (j = n % 16, g = n // 128)
    holds one of each class c with c // 16 == (j + g) % 3.  Every dot product therefore has exactly ONE non-zero term, of class
    i + 16 ((j + g) % 3): over the 16 x 16 outputs of any MFMA tile every class occurs, in every 16-row class of every 128-row tile
    (MFMA row tile of either wave layout, both staging rows of a thread) and every 16-unit class of every 128 units.
    All entries of one k index are of one kind, so no dropped product can be non-zero.
    Returns a, W, b and cls [M, N]: the class of each output's term."""
    assert K % FC_BK == 0 and K // FC_BK >= 3 and M >= 1
    rs = np.random.RandomState(seed)
    a, W = np.zeros((M, K), np.float32), np.zeros((N, K), np.float32)
    kinds = list(KINDS.values())
    ks_of = [probe_class(c, K) for c in range(NCLASS)]
    assert len({k[3] for k in ks_of}) == NCLASS
    for c, (kind, q, ksc, k) in enumerate(ks_of):
        (wl, wh), (xl, xh) = kinds[kind]
        rows = np.arange(M)[np.arange(M) % 16 == c % 16]
        cols = np.arange(N)[(np.arange(N) % 16 + np.arange(N) // 128) % 3 == c // 16]
        a[rows, k] = _odd(rs, xl, xh, len(rows))
        W[cols, k] = _odd(rs, wl, wh, len(cols))
    b = rs.randint(-15, 16, size=N).astype(np.float32) if bias else np.zeros(N, np.float32)
    cls = (np.arange(M) % 16)[:, None] + 16 * (((np.arange(N) % 16 + np.arange(N) // 128) % 3)[None, :])
    for form in KEPT:      # the conditions of exactness, for the rows as they are and under the 'mixed' row pattern (which takes no bias)
        assert_exact(a, W, b, form)
        if not bias:
            assert_exact(row_pattern(a, 'mixed'), W, b, form)
    return a, W, b, cls


# rows of the 'mixed' pattern, several inside the first 128-row tile and on both sides of rows 63 / 64
ZERO_ROWS = (5, 63, 130)
POW2_ROWS = (17, 64, 200)          # maximum exactly 2^p
CLAMP_ROWS = (33, 62, 65, 256)      # maximum 2^-100: fc_row_exp's clamp at 96


def spread_exp(m):
    """The row scales of the 'mixed' pattern: 2^-40 .. 2^40; rows m and m + 64 (one thread's two staging rows) 19 apart."""
    return (np.asarray(m) * 37) % 81 - 40


def row_pattern(a, pattern):
    """'one': a itself.  'mixed': row m times 2^spread_exp(m); ZERO_ROWS zero; in POW2_ROWS and CLAMP_ROWS the non-zero entries
    become +-{1, 3/4, 5/8} 2^p (one bf16 piece: allowed at every k index of a probe), the first of them 1 so that the row's
    maximum is 2^p exactly, p = the row's spread exponent resp. -100."""
    a = np.array(a, dtype=np.float32)
    if pattern == 'one':
        return a
    assert pattern == 'mixed'
    M = a.shape[0]
    e = spread_exp(np.arange(M))
    for m in POW2_ROWS + CLAMP_ROWS:
        if m < M:
            nz = np.flatnonzero(a[m])
            vals = np.array([1., .75, .625], np.float32)[np.arange(len(nz)) % 3]
            vals[1:] *= np.sign(a[m, nz[1:]])
            a[m, nz] = vals
            if m in CLAMP_ROWS:
                e[m] = -100
    a = np.ldexp(a, e[:, None]).astype(np.float32)
    for m in ZERO_ROWS:
        if m < M:
            a[m] = 0
    return a


def coverage(cls, a, W, K, bn=128):
    """The set of (class, 16-row class of the 128-row tile, 16-unit class of bn units) over the outputs with a non-zero term."""
    M, N = cls.shape
    out = set()
    for c in range(NCLASS):
        k = probe_class(c, K)[3]
        live = (cls == c) & (a[:, k] != 0)[:, None] & (W[:, k] != 0)[None, :]
        mm, nn = np.nonzero(live)
        out |= {(c, int(r), int(s)) for r, s in zip((mm % FC_BM) // 16, (nn % bn) // 16)}
    return out
