"""tests/fcgemm_ref.py without a GPU: its matrix statements against plain triple loops in fp64, the split emulators against the
rules of csrc/fcgemm.hip on hand-made values, the exactness conditions of the input builders, the sensitivity of the piece probes
to every kept product, and the launch-geometry helper of the library (host arithmetic only: alq_fcgemm_geometry makes no device
call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fcgemm_ref as R

# K -> N of the layer under test (tests/test_gpu_fcgemm.py runs the same table)
SHAPES = [(256, 256), (256, 320), (320, 256), (288, 384), (384, 288), (512, 256), (224, 256)]


# ------------------------------------------------------------------------------------------ fp64 statement
def test_statements_against_triple_loops():
    rs = np.random.RandomState(1)
    M, K, N = 3, 5, 4
    a, W, b = rs.randn(M, K), rs.randn(N, K), rs.randn(N)
    dout, prev = rs.randn(M, N), rs.randn(M, K)
    out = np.zeros((M, N))
    din = np.zeros((M, K))
    dW = np.zeros((M, N, K))
    for m in range(M):
        for n in range(N):
            acc = 0.
            for k in range(K):
                acc += a[m, k] * W[n, k]
                din[m, k] += dout[m, n] * W[n, k]
                dW[m, n, k] = dout[m, n] * a[m, k]
            out[m, n] = acc + b[n]
    np.testing.assert_allclose(R.forward64(a, W, b, False), out, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(R.forward64(a, W, b, True), np.where(out > 0, out, 0.), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(R.din64(dout, W), din, rtol=1e-14, atol=1e-15)
    masked = R.din64(dout, W, prev)
    assert np.array_equal(masked != 0, (prev > 0) & (din != 0))
    np.testing.assert_allclose(masked, din * (prev > 0), rtol=1e-14, atol=1e-15)
    gW, gb = R.wgrad64(a, dout)
    np.testing.assert_allclose(gW, dW, rtol=1e-15)
    assert np.array_equal(gb, dout)
    import torch
    for dt, tol in ((torch.float64, 1e-14), (torch.float32, 1e-5)):
        np.testing.assert_allclose(R.forward_torch(a, W, b, True, dt), R.forward64(a, W, b, True), rtol=tol, atol=tol)
        np.testing.assert_allclose(R.din_torch(dout, W, prev, dt), masked, rtol=tol, atol=tol)
        np.testing.assert_allclose(R.wgrad_torch(a, dout, dt)[0], dW, rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------ splits
def _bf16_rne_scalar(x):
    """Round to 8 significant bits, ties to even, with Python integers."""
    if x == 0:
        return 0.
    m, e = np.frexp(np.float64(x))
    n = int(abs(m) * 2 ** 53)          # exact
    q, r = divmod(n, 2 ** 45)          # keep 8 bits
    if r > 2 ** 44 or (r == 2 ** 44 and q & 1):
        q += 1
    return float(np.sign(x) * q * 2. ** (e - 8))


def test_bf16_triples():
    rs = np.random.RandomState(2)
    vals = np.concatenate([rs.randn(2000).astype(np.float32) * np.float32(2.) ** rs.randint(-30, 30, 2000),
                           np.array([0., 1., -1., 257., 258., 259., 383., 385., 1 + 2. ** -8, 1 + 3 * 2. ** -8, 2. ** -100, 3 * 2. ** 40, 2 ** 24 - 1.],
                                    np.float32)])
    got = R.bf16_rne(vals)
    want = np.array([_bf16_rne_scalar(float(v)) for v in vals])
    assert np.array_equal(got.astype(np.float64), want)
    assert got[list(vals).index(257.)] == 256. and got[list(vals).index(259.)] == 260.      # a tie goes to the even neighbour; 259 rounds up
    assert np.all(got.view(np.uint32) & 0xffff == 0)
    for dev in (False, True):
        p = R.triples(vals, device=dev)
        assert np.array_equal(p.sum(0), vals.astype(np.float64))           # hi + mid + lo is exact for every fp32
        assert np.all(p.astype(np.float32).view(np.uint32) & 0xffff == 0)
    # the device's third piece (the upper half of what two roundings leave) is the host's third rounding
    assert np.array_equal(R.triples(vals, device=True), R.triples(vals))


def test_fp16_pair_exponents():
    f = np.float32
    #                  max |x|            ex: max < 2^ex     e = 14 - ex
    for amax, e in ((1., 13), (1.5, 13), (2., 12), (np.nextafter(f(2), f(0)), 13), (0.5, 14), (2. ** 13, 0), (2. ** 40, -27),
                    (2. ** -82, 95), (2. ** -83, 96), (2. ** -84, 96), (2. ** -100, 96), (0., 0), (3 * 2. ** -100, 96)):
        assert R.row_exp(f(amax)) == e, amax
        if amax and e < 96:
            assert 2 ** 13 <= amax * 2. ** e < 2 ** 14
    # the matrix rule is the same rule without the clamp; a zero matrix takes 14
    assert R.matrix_exp(np.zeros((2, 2))) == 14 and R.matrix_exp(np.array([[1., -3.]])) == 12 and R.matrix_exp(np.array([2. ** -100])) == 113
    assert R.matrix_exp(np.array([4.])) == R.row_exp(f(4.)) == 11 and R.bound_exp(4.) == 11 and R.bound_exp(5.) == 11 and R.bound_exp(8.) == 10


def test_fp16_pairs():
    x = np.array([[2049., 1., 0., -2047.], [0., 0., 0., 0.], [2. ** -100, -2. ** -101, 2. ** -110, 0.], [3 * 2. ** 38, 2. ** 40 + 2. ** 20, 0, 1.]], np.float32)
    e = R.row_exp(np.abs(x).max(axis=1))
    assert list(e) == [2, 0, 96, -27]
    p = R.pairs(x, e)
    assert p.shape == (2, 4, 4)
    # 22 significant bits survive; a remainder below the smallest fp16 subnormal at the row's scale is lost (last entries of rows 2, 3)
    want = x.astype(np.float64).copy()
    want[2, 2] = 0.             # 2^-110 2^96 = 2^-14 is the smallest normal: kept ...
    want[2, 2] = 2. ** -110
    want[3, 3] = 0.             # 1 2^-27 is below 2^-24
    assert np.array_equal(p.sum(0), want)
    assert p[0, 0, 0] == 2048. and p[1, 0, 0] == 1. and p[1, 0, 1] == 0. and not p[:, 1].any()
    assert p[0, 3, 1] == 2. ** 40 and p[1, 3, 1] == 2. ** 20
    # every piece is an fp16 number at the row's scale
    for pc in p:
        s = pc * np.ldexp(1., e)[:, None]
        assert np.array_equal(s.astype(np.float16).astype(np.float64), s)


def test_subset_eval_is_the_product_when_nothing_is_dropped():
    rs = np.random.RandomState(3)
    a, W = rs.randn(9, 64).astype(np.float32), rs.randn(7, 64).astype(np.float32)
    ap, wp = R.split(a, W, 'triples')
    every = [(i, j) for i in range(3) for j in range(3)]
    np.testing.assert_allclose(R.subset_eval(ap, wp, every), R.forward64(a, W, np.zeros(7), False), rtol=1e-13, atol=1e-13)
    kept = R.subset_eval(ap, wp, R.TRIPLE_KEPT)
    assert np.abs(kept - R.forward64(a, W, np.zeros(7), False)).max() < 64 * 3 * 2. ** -24 * np.abs(a).max() * np.abs(W).max()
    ap, wp = R.split(a, W, 'pairs')
    assert np.abs(R.subset_eval(ap, wp, R.PAIR_KEPT) - R.forward64(a, W, np.zeros(7), False)).max() < 64 * 4 * 2. ** -21 * np.abs(a).max() * np.abs(W).max()
    w2 = R.subset_eval(ap, wp, R.PAIR_KEPT, {(0, 0): 2.})
    assert np.array_equal(w2 - R.subset_eval(ap, wp, R.PAIR_KEPT), R.subset_eval(ap, wp, [(0, 0)]))


# ------------------------------------------------------------------------------------------ probes and dense sets
def _probe(M, K, N, pattern, bias):
    a, W, b, cls = R.probe_set(M, K, N, seed=K + N, bias=bias)
    return R.row_pattern(a, pattern), W, b, cls


@pytest.mark.parametrize('K,N', SHAPES, ids=['%dto%d' % s for s in SHAPES])
def test_probe_sets_are_exact_and_cover_every_tile_position(K, N):
    M = 257
    for pattern, bias in (('one', False), ('one', True), ('mixed', False)):
        a, W, b, cls = _probe(M, K, N, pattern, bias)
        for form in ('pairs', 'triples'):
            worst = R.assert_exact(a, W, b, form)
            assert worst < 24
            ap, wp = R.split(a, W, form)
            assert np.array_equal(R.subset_eval(ap, wp, R.KEPT[form]) + b[None, :].astype(np.float64), R.forward64(a, W, b, False))
        out = R.forward64(a, W, b, False)
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out)      # the statement itself is an fp32 array
        nz = np.count_nonzero(a, axis=1)
        assert nz.max() == 3 and np.count_nonzero(W, axis=1).max() == 16
        if pattern == 'one':
            # every class in every 16-row class of the 128-row tile and every 16-unit class of 128 (and of 64) units
            for bn in (128, 64):
                cov = R.coverage(cls, a, W, K, bn)
                assert cov == {(c, r, s) for c in range(R.NCLASS) for r in range(8) for s in range(bn // 16)}
            assert sorted({R.probe_class(c, K)[1:3] for c in range(R.NCLASS)}) == [(q, t) for q in range(4) for t in range(3)]
            ks = sorted({R.probe_class(c, K)[3] // 32 for c in range(R.NCLASS)})
            assert ks == sorted({0, K // 64, K // 32 - 1})
        else:
            e = R.row_exp(np.abs(a).max(axis=1))
            assert not a[list(R.ZERO_ROWS)].any() and all(e[m] == 96 and np.abs(a[m]).max() == 2. ** -100 for m in R.CLAMP_ROWS)
            for m in R.POW2_ROWS:
                assert np.frexp(np.abs(a[m]).max())[0] == 0.5 and np.count_nonzero(a[m]) == 3
            live = [m for m in range(128) if m not in R.ZERO_ROWS + R.CLAMP_ROWS]
            assert e[live].max() - e[live].min() >= 70                         # 2^-40 .. 2^40 inside one 128-row tile
            assert all(e[m] != e[m + 64] for m in range(64) if m in live and m + 64 in live)


@pytest.mark.parametrize('form', ['pairs', 'triples'])
def test_probes_notice_every_kept_product(form):
    """Removing any one kept product from the subset, or doubling it, changes an output - of every probe set the device test runs."""
    for K, N in ((256, 256), (288, 384), (512, 256)):
        for pattern in ('one', 'mixed'):
            a, W, b, cls = _probe(257, K, N, pattern, False)
            ap, wp = R.split(a, W, form)
            full = R.subset_eval(ap, wp, R.KEPT[form])
            assert np.array_equal(full, R.forward64(a, W, b, False))
            for prod in R.KEPT[form]:
                less = R.subset_eval(ap, wp, [p for p in R.KEPT[form] if p != prod])
                twice = R.subset_eval(ap, wp, R.KEPT[form], {prod: 2.})
                n_less, n_twice = np.count_nonzero(less != full), np.count_nonzero(twice != full)
                assert n_less > 0 and n_twice > 0, (K, N, pattern, form, prod)
                if pattern == 'one':      # ... and in every tile position class: the outputs that move cover rows and units classes
                    mm, nn = np.nonzero(less != full)
                    assert {(r, s) for r, s in zip((mm % 128) // 16, (nn % 128) // 16)} == {(r, s) for r in range(8) for s in range(8)}, (form, prod)
                    kk = {R.probe_class(c, K)[1:3] for c in np.unique(cls[mm, nn])}
                    assert kk == {(q, t) for q in range(4) for t in range(3)}, (form, prod, kk)


def test_a_blind_probe_set_would_be_caught():
    """The sensitivity test is itself sensitive: one-piece numbers everywhere exercise (hi, hi) only."""
    a, W, b = R.dense_ints(8, 256, 64, seed=5)
    ap, wp = R.split(a, W, 'triples')
    full = R.subset_eval(ap, wp, R.TRIPLE_KEPT)
    assert np.array_equal(R.subset_eval(ap, wp, [(0, 0)]), full)
    with pytest.raises(AssertionError):
        x = np.full((4, 64), 2049., np.float32)      # two fp16 pieces on both sides: the dropped (l, l) product is not zero
        R.assert_exact(x, x, None, 'pairs')
    with pytest.raises(AssertionError):
        x = np.full((4, 64), 4095., np.float32)      # 64 products of 24 bits: the sum leaves fp32
        R.assert_exact(x, x, None, 'triples')


@pytest.mark.parametrize('K,N', SHAPES, ids=['%dto%d' % s for s in SHAPES])
def test_dense_integer_sets_are_exact(K, N):
    a, W, b = R.dense_ints(65, K, N, seed=K * N)
    assert np.abs(a).max() == 15 and np.abs(W).max() == 15 and np.abs(b).max() == 15
    for form in ('pairs', 'triples'):
        assert R.assert_exact(a, W, b, form) <= np.log2(225 * 512 + 15)
    # the backward contraction of an integer cotangent under a static bound (fp16 pairs at one scale)
    dout = np.random.RandomState(7).randint(-30, 31, size=(65, N)).astype(np.float32)
    for bound in (30., 4096., 2. ** 20):
        R.assert_exact(dout, W.T.copy(), None, 'pairs', a_exp=R.bound_exp(bound))


# ------------------------------------------------------------------------------------------ the library's geometry helper
class _env(object):
    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ('ALQ_FC_BN64', 'ALQ_FC_SQUARE')}
        for k in self.old:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _geometry(K, N, M, out=True):
    from nnal_amd import _lib
    buf = (C.c_int * 6)(*([-1] * 6))
    rc = _lib.lib().alq_fcgemm_geometry(K, N, M, buf if out else None)
    return rc, tuple(buf)


def test_launch_geometry_helper():
    from nnal_amd import _lib
    assert 'alq_fcgemm_geometry' in _lib.exported_names()
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'alq.h')).read()
    assert re.search(r'\bint alq_fcgemm_geometry\(int K, int N, int M, int \*out\);', hdr)
    # the issue's table: forward K -> N, backward N -> K
    with _env():
        assert _geometry(256, 256, 257) == (0, (1, 128, 1, 2, 3, 8))
        assert _geometry(256, 320, 128) == (0, (1, 64, 0, 5, 1, 8)) and _geometry(320, 256, 128) == (0, (1, 128, 1, 2, 1, 10))
        assert _geometry(288, 384, 129) == (0, (1, 128, 1, 3, 2, 9)) and _geometry(384, 288, 129) == (0, (0,) * 6)
        assert _geometry(512, 256, 1) == (0, (1, 128, 1, 2, 1, 16)) and _geometry(224, 256, 1) == (0, (0,) * 6) and _geometry(256, 224, 1) == (0, (0,) * 6)
        assert _geometry(6144, 4096, 2048) == (0, (1, 128, 1, 32, 16, 192))
        assert _geometry(272, 256, 1) == (0, (0,) * 6) and _geometry(256, 272, 1) == (0, (0,) * 6)      # K % 32, N % 64
    for form, env in ((0, {}), (1, {'ALQ_FC_SQUARE': '1'}), (2, {'ALQ_FC_BN64': '1'}), (2, {'ALQ_FC_BN64': '1', 'ALQ_FC_SQUARE': '1'})):
        with _env(**env):
            for K, N in SHAPES + [(N, K) for K, N in SHAPES]:
                for M in (1, 128, 129, 257):
                    assert _geometry(K, N, M) == (0, R.geometry(K, N, M, form)), (K, N, M, env)
    L = _lib.lib()
    for bad in ((0, 256, 1), (256, 0, 1), (256, 256, 0), (-256, 256, 1), (256, -256, 1), (256, 256, -1)):
        assert _geometry(*bad)[0] == -1 and b'alq_fcgemm_geometry' in L.alq_last_error(), bad
    assert _geometry(256, 256, 1, out=False)[0] == -1
