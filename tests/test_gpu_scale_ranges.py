"""The fp16-pair scale logic across weight, bias and input ranges (GPU box).

Every fast route contracts on fp16 pairs under a power-of-two scale it picks itself: from measured per-patch maxima (the first
conv + pool kernel, the igemm4 epilogues, rowmax_u32_kernel), from derived per-patch bounds (rowmax_abs_kernel +
fwd_bounds_kernel over weight_layout.h::conv_norms), from the static cotangent bounds of passes.hip::bwd_bounds, and from the
weights' own exponent (f16_pair.h::f16_pair_exp).  A bound that is too small, an exponent field outside [1, 254] or an engaged
clamp faults nothing: some patches silently lose accuracy.  Read-back: alq_model_debug_copy what = 15 .. 18, and the two kernels
on caller buffers (alq_debug_rowmax_abs, alq_debug_fwd_bounds).

(a) rowmax_abs_kernel and fwd_bounds_kernel alone.
    rowmax_abs: fmaxf drops a NaN, so a row holding one yields the maximum of the rest (asserted; kernels.hip says so too).
(b) soundness: derived bounds bound the fp64 oracle's activations, stay below tests/scale_ref.l1_chain, do not depend on the batch;
    measured maxima are the maxima; the cotangent bounds bound the cotangents.
    Rules.  A measured maximum (what = 16 / 17) equals max |.| of the tensor the pass stored (what = 0; the network input for 17)
    bit for bit.  A derived bound of a layer behind at least one conv / conv_transpose of the chain is >= the fp64 maximum
    outright.  Row 0 of a chain that starts at layer 0's measured output maximum, and the pool rows that only pass it on (L = 1,
    B = 0), ARE that fp32 measurement: they are held to the fp64 maximum within 2^-18 relative (fp32 rounding of a 27-term dot
    product), not to >=.  Which layers: NET-C at 32^3 measures enc1 and up2 in both kinds of pass, both tensors are stored, so
    both fall under the bit-for-bit rule (and lie within 2^-18 of fp64, asserted as well); its chain starts at enc1's maximum.
    NET-C at 8^3 measures and derives nothing.  NET-B measures the input only (17) and derives every row from it.
(c) exact equivariance under tests/scale_ref.rescale (the network is the same function, every scale moves by the same power of
    two, so the scaled operands entering the matrix cores are the same bits): p1 and every layer score but those of the rescaled
    layer j and of its consumers are bit-identical to the base model's; layer j's are exactly 2^-k times the base; the engine info
    (1, 6, 10, 12 and the backward indices) is the base model's.  Asserted bit for bit for layer = input, bott, dec1, dec2 of NET-C
    and input, conv1 .. conv4 of NET-B on every route, and for every layer under knob 4 (no fp16 pairs at all).
    What is legitimately NOT exact, each held to the fp64 bar of (d) instead:
      * the scores of the CONSUMER layers (and of the first layer for layer = 'input'): a layer score is sum dW + sum db
        (the box-dot kernels: sum dsum * (box(asum) + 1), tests/factored_ref.py:142); the consumer's bias is not rescaled, so only
        the dW share moves by 2^k and the sum is no power-of-two multiple of the base;
      * everything behind a layer whose output is read as ONE SLICE OF A CONCAT (enc1, enc2, up1, up2 of NET-C), on every fp16
        route: the consumer over the concat (dec1 / dec2) has ONE weight exponent for both input slices (d3d.hip:491,
        c3d.hip:1387, igemm4's w16_exp: f16_pair_exp over the whole filter) and ONE input scale per patch from the larger of the
        two parts' bounds (d3d.hip:87, c3d.hip:185, igemm4.hip:1023), so scaling one slice moves the hi / lo split of the two
        slices relative to each other.  Measured with the exact assertion still on them: up1 k = 12 moved p1 by 2 ulp, up2 k = -37 by 2 %.
        These layers take k = +-12 only: from about 2^25 between the slices the smaller one loses pieces, from 2^38 (fp16 reaches
        2^-24 below 1, the pairs are scaled to 2^14) nothing of it is left; beyond 2^20 the model leaves the fp16 routes ((e) below),
        which is another route than the base model's.
    A bug this section found (fixed in passes.hip::bwd_bounds + weight_layout.h::conv_bwd_l1_slices): the static cotangent bound took
    ONE backward L1 norm per layer, the maximum over ALL input channels of a concat.  With enc1 or enc2 rescaled by 2^-12 the bound
    handed to the producer of the other slice was 2^12 too large, the fp16 pairs of the backward launches below it lost 12 of their 22
    bits: e_dev / e_32 = 654 on enc1's score (enc1 k = -12) and 698 (enc2 k = -12), 4.5e-4 of the maximum, against 7.5 on the bf16x3
    arm.  Each producer now gets the norm of its own slice; both cases are back under the bar.
(d) against fp64 where nothing is exact: zero bias, bias times 2^10, the 37 x / 2^-9 layer scalings of test_gpu_weights_reset, the
    tight_input passes.  Truth OracleModel(float64), yardstick the fp32 OracleModel; patches with no fragile decision at
    ref64.DEFAULT_EPS (tests/convt_ref.first_stable_patches; none left out; a tight_input patch is zero but for one window, so its
    pools are all ties: it is taken as it is).
    Bar per layer score column of g = S / size, g0 and g1: e_dev <= 4 R e_32 + 6e-8 mean |ref|, never looser than
    2e-4 max |ref| + 1e-9; p1 within 2e-6 of fp64.
(e) the ends of the range: k = +-64 and +-90 on the input (NET-C 32^3, NET-B 32^3) and on enc2 (NET-C 32^3).
    A bug this section found (fixed in igemm3.hip, locate()): the forward fp16-pair launches of igemm3 clamped the bound's exponent
    field to [40, 200]; NET-B's input times 2^90 (first layer's weights times 2^-90) kept the scale of 2^73, x 2^f left fp16's range
    and p1 was off by 0.124.  The window is now [40, 254]: every bound from 2^-87 up keeps its own scale; the lower end stays, it also keeps the
    accumulator (output times the product scale, bias included) finite under a tiny input bound.
    A limit this section found, and what the model does about it (weight_layout.h::slices_within_f16_range, model.hip::apply_knobs):
    enc2 is a skip source, dec1 reads [enc2, up1] as one concat under one input scale and one weight exponent (above).  With the
    slices 2^64 apart the smaller one was flushed, dec1's output was its bias and p1 was off by 0.1325 at all four k.  No clamp is
    involved.  A conv / conv_transpose over a concat whose two weight slices lie more than 20 binades apart now takes the whole
    model off the fp16-pair launches: every pass runs on bf16 triples, which keep fp32's exponent range (the ALQ_NO_F16X2 arm;
    asserted from the engine info), and p1 is within 6.6e-07 of the base.  What stays: two parts of a concat INPUT further apart
    than fp16 holds under slices of similar weights - one input scale per patch - lose the smaller part on the fp16 routes.
"""
import ctypes as C
import time
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests import convt_ref, factored_ref, scale_ref  # noqa: E402
from tests.test_gpu_convt import _copy, _dev, _env, _knob  # noqa: E402
from tests.test_gpu_hvp import EPS, fragile_units  # noqa: E402
from tests.test_gpu_weights_device import WIDE  # noqa: E402

ALQ_EUNSUPPORTED = -4      # include/alq.h

# Largest e_dev / e_32 over the 2120 (case, route, array, layer) figures of this file whose e_32 is above the floor 6e-8 mean |ref|
# (below it the fp32 oracle's error is one rounding of a typical entry and the quotient says nothing), measured on an MI355X on
# 2026-10-21: 73.248 at NET-C 32^3 with every bias zero, dec1 rescaled by 2^12, unit-cotangent score of up2 (e_dev 3.440e-04,
# e_32 4.696e-06, max |ref| 92.8: 3.7e-6 of the maximum).  The next are 60.272 (same model, input and bott rescaled, up2), 41.357
# (37 x dec2, 2^-9 x enc2, up2), 43.489 (enc2 rescaled by 2^-90, on bf16 triples, bott), 26.928 (ALQ_NO_F16X2=1, enc2 rescaled by 2^-12, bott) and 25.940 (bias x 2^10, up2).  up2's
# column leads on every route, the exact-fp32 arm (knob 4) included: it is the summation order of the conv_transpose box-dot, not a
# scale.  The largest figure relative to its column's max |ref| is 1.97e-4 (NET-B 32^3, tight_input at amax 37, conv3; fp32 oracle
# 4.9e-5), the next 3.2e-5.  DESIGN.md's accuracy table has the figures per case.
R_DEV_OVER_F32 = 73.248
R_FACTOR = 4.0
_T0 = time.time()


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    yield device.default_session()
    for r in sorted(_RATIOS, reverse=True)[:5]:      # what R_DEV_OVER_F32 is taken from
        print('e_dev / e_32 = %.3f at %s | %s | %s' % r)
    print('tests/test_gpu_scale_ranges.py: %.1f s from import to the last test' % (time.time() - _T0))


# ------------------------------------------------------------------------------------------ (a) the two kernels alone
def _rowmax(sess, x, K, offset=0):
    """rowmax_abs_kernel on x [N, K] placed `offset` floats behind an aligned allocation; (bits [N], the words behind them)."""
    from nnal_amd._lib import check
    torch = sess.torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    N = x.shape[0]
    assert x.shape == (N, K)
    buf = torch.zeros((N * K + offset + 8,), dtype=torch.float32, device=sess.device)
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + N * K] = torch.from_numpy(x.reshape(-1)).to(sess.device)
    out = torch.full((N + 8,), 0x5a5a5a5a, dtype=torch.int32, device=sess.device)
    sess.bind_stream()
    check(sess.lib.alq_debug_rowmax_abs(sess.ctx, C.c_void_p(buf.data_ptr() + 4 * offset), N, K, C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return o[:N], o[N:]


def _rowmax_ref(x):
    return np.fmax.reduce(np.abs(np.asarray(x, np.float32)), axis=1, initial=np.float32(0)).astype(np.float32).view(np.uint32)


ROWMAX_K = [4 * q for q in (63, 64, 65, 255, 256, 257, 448, 449)] + [75, 1251]


@pytest.mark.parametrize('K', ROWMAX_K)
def test_rowmax_abs_rows(sess, K):
    """Against np.abs(x).max(1) bit for bit: the four-vector unroll and its tail, K % 4 != 0, N = 1 .. 9 (four rows per workgroup),
    the base pointer 4 bytes off a 16-byte boundary with K % 4 == 0 (the alignment test reads x, not the row); the maximum in the
    first / last element of a row and in the last row, negative."""
    rs = np.random.RandomState(K)
    for N in (1, 3, 4, 5, 9):
        x = rs.randn(N, K).astype(np.float32)
        x[0, 0] = 9.0                       # first element of a row
        x[N - 1, K - 1] = -11.0             # last element of the last row, negative
        if N > 2:
            x[1, K - 1] = 10.0
        ref = _rowmax_ref(x)
        assert (N == 1 or ref[0] == np.float32(9.0).view(np.uint32)) and ref[N - 1] == np.float32(11.0).view(np.uint32)
        for off in ((0, 1) if K % 4 == 0 else (0, 1, 3)):
            got, tail = _rowmax(sess, x, K, off)
            np.testing.assert_array_equal(got, ref, err_msg='K=%d N=%d offset=%d' % (K, N, off))
            assert (tail == 0x5a5a5a5a).all(), 'wrote behind out[N]'


@pytest.mark.parametrize('K', (256, 1028, 75))
def test_rowmax_abs_special_values(sess, K):
    """-0.0 and an all-zero row give +0; a subnormal maximum stays; +inf wins; a NaN is dropped by fmaxf: the row's result is the
    maximum of the rest (0 for a row of NaN only)."""
    rs = np.random.RandomState(K + 1)
    x = rs.randn(9, K).astype(np.float32)
    x[0] = 0.0
    x[1] = 0.0
    x[1, K // 2] = -0.0
    x[2] = 0.0
    x[2, K - 1] = np.float32(-3e-42)        # subnormal, negative, last element
    x[3, 5] = np.inf
    x[4, 0] = np.nan
    x[5, K - 1] = np.nan
    x[5, K - 2] = -77.0
    x[6] = np.nan
    x[7, 3] = -np.inf
    x[7, 4] = np.nan
    ref = _rowmax_ref(x)
    assert ref[0] == 0 and ref[1] == 0 and ref[2] == np.float32(3e-42).view(np.uint32) and ref[3] == 0x7f800000
    assert np.isfinite(ref[4:5].view(np.float32)).all() and ref[5] == np.float32(77.0).view(np.uint32) and ref[6] == 0 and ref[7] == 0x7f800000
    for off in (0, 1):
        got, _ = _rowmax(sess, x, K, off)
        np.testing.assert_array_equal(got, ref, err_msg='K=%d offset=%d' % (K, off))


def _fwd_bounds(sess, amax0, stride, L, B, src2, from_input):
    from nnal_amd._lib import check
    torch = sess.torch
    N, nl = len(amax0), len(L)
    a = sess.to_device(np.ascontiguousarray(amax0, np.float32).view(np.int32), torch.int32)
    out = torch.full((nl * stride + 8,), 0x5a5a5a5a, dtype=torch.int32, device=sess.device)
    sess.bind_stream()
    check(sess.lib.alq_debug_fwd_bounds(sess.ctx, C.c_void_p(a.data_ptr()), N, stride, (C.c_float * nl)(*[float(v) for v in L]),
                                        (C.c_float * nl)(*[float(v) for v in B]), (C.c_int32 * nl)(*[int(v) for v in src2]), nl,
                                        int(from_input), C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    rows = o[:nl * stride].reshape(nl, stride)
    assert (rows[:, N:] == 0x5a5a5a5a).all() and (o[nl * stride:] == 0x5a5a5a5a).all(), 'wrote outside [nl, N]'
    return np.ascontiguousarray(rows[:, :N]).view(np.float32)


def _chain_case(nl, seed, zero_bias):
    """L, B in 2^[-40, 40] (B = 0 for some layers, for all under zero_bias) with the running bound of an input of 1 kept inside
    2^+-100, src2 as NET-C's skips (8 <- 0, 6 <- 2) and two more beyond its 10 layers."""
    rs = np.random.RandomState(seed)
    src2 = [-1] * nl
    for dst, src in ((6, 2), (8, 0), (12, 10), (15, 3)):
        if dst < nl:
            src2[dst] = src
    L, B, run = [], [], 0.0
    for k in range(nl):
        e = int(rs.randint(-40, 41))
        if abs(run + e) > 40:
            e = -e
        run += e
        L.append(np.float32(np.ldexp(rs.uniform(1.0, 2.0), e)))
        B.append(np.float32(0.0) if (zero_bias or k % 3 == 1) else np.float32(np.ldexp(rs.uniform(1.0, 2.0), int(rs.randint(-40, 41)))))
        run = max(run, np.log2(float(B[-1])) if B[-1] > 0 else -1e9) + 1      # (+1: the mantissas)
    return np.array(L, np.float32), np.array(B, np.float32), src2


@pytest.mark.parametrize('nl', (1, 2, 10, 16))
@pytest.mark.parametrize('from_input', (0, 1))
def test_fwd_bounds_chain(sess, nl, from_input):
    """Step by step each value lies within 1 fp32 ulp of in * L + B evaluated in fp64 on the kernel's own inputs of that step and
    rounded to float (the compiler may or may not contract the multiply-add; all terms are positive, so both forms are within
    1 ulp of the exact value's rounding); end to end within nl * 2^-23 of scale_ref.chain in fp64; monotone in amax0; nothing
    written outside [nl, N] under stride > N."""
    for N in (1, 256, 257):
        for zero_bias in (False, True):
            L, B, src2 = _chain_case(nl, 100 * nl + N + from_input, zero_bias)
            rs = np.random.RandomState(N)
            amax0 = np.ldexp(rs.uniform(1.0, 2.0, size=N), rs.randint(-20, 21, size=N)).astype(np.float32)
            if N > 4:
                amax0[3] = amax0[2]
                amax0[1] = 0.0
            got = _fwd_bounds(sess, amax0, N + 3, L, B, src2, from_input)
            ref = scale_ref.chain(amax0, L.astype(np.float64), B.astype(np.float64), src2, from_input)
            nzr = ref > 0
            assert np.isfinite(got).all() and (ref[nzr] > 2.0 ** -120).all() and (ref < 2.0 ** 120).all()
            g64 = got.astype(np.float64)
            for k in range(nl):
                if k == 0:
                    step = amax0.astype(np.float64) * L[0] + B[0] if from_input else amax0.astype(np.float64)
                else:
                    x = np.maximum(g64[k - 1], g64[src2[k]]) if src2[k] >= 0 else g64[k - 1]
                    step = x * np.float64(L[k]) + np.float64(B[k])
                want = step.astype(np.float32)
                ulps = np.abs(got[k].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
                assert ulps.max() <= 1, (nl, N, k, ulps.max())
            assert (np.abs(g64 - ref) <= nl * 2.0 ** -23 * ref).all(), (nl, N, np.max(np.abs(g64 - ref) / (ref + 1e-300)))
            order = np.argsort(amax0, kind='stable')
            assert (np.diff(got[:, order], axis=1) >= 0).all(), 'not monotone in amax0'
            if N > 4:
                np.testing.assert_array_equal(got[:, 3].view(np.uint32), got[:, 2].view(np.uint32))


def test_debug_entry_points_refuse_bad_arguments(sess):
    from nnal_amd._lib import ALQ_EINVAL
    torch = sess.torch
    buf = torch.zeros((64,), dtype=torch.int32, device=sess.device)
    p = C.c_void_p(buf.data_ptr())
    f, i = (C.c_float * 2)(1.0, 1.0), (C.c_int32 * 2)(-1, 1)
    assert sess.lib.alq_debug_rowmax_abs(sess.ctx, p, 0, 4, p) == ALQ_EINVAL
    assert sess.lib.alq_debug_rowmax_abs(sess.ctx, p, 1, 0, p) == ALQ_EINVAL
    assert sess.lib.alq_debug_fwd_bounds(sess.ctx, p, 2, 1, f, f, i, 2, 0, p) == ALQ_EINVAL          # stride < N
    assert sess.lib.alq_debug_fwd_bounds(sess.ctx, p, 1, 1, f, f, i, 2, 0, p) == ALQ_EINVAL          # src2[1] = 1 names no earlier layer
    assert sess.lib.alq_debug_fwd_bounds(sess.ctx, p, 1, 1, f, f, i, 17, 0, p) == ALQ_EINVAL


# ------------------------------------------------------------------------------------------ models and oracles (CPU, computed once)
def _stable(ld, in_shape, sk, pars, xseed, n, scale=1.0):
    import torch
    om64 = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
    for seed in range(xseed, xseed + 8):
        xs, chosen = convt_ref.first_stable_patches(om64, in_shape, seed, n, 64, fragile_units)
        if len(chosen) == n:
            return np.ascontiguousarray(xs * np.float32(scale)), seed, chosen
    raise AssertionError('no %d stable patches within 64 scanned of 8 streams' % n)


_MODELS = {}


def model(name):
    """name -> record(ld, sk, in_shape, pars, x [n stable patches], n, mb): computed once, never modified."""
    if name in _MODELS:
        return _MODELS[name]
    if name == 'netc32':
        from tests.test_gpu_grads_fp64 import assert_no_fragile_decision, case
        c = case('netc_32')
        assert_no_fragile_decision(c)
        d = dict(ld=c['ld'], sk=c['sk'], in_shape=c['in_shape'], pars=c['pars'], x=c['x'], n=c['n'])
    else:
        if name == 'netc8':
            ld, sk = netspec.net_c()
            in_shape, n, wseed = (8, 8, 8, 1), 5, 85
        elif name == 'netb25':
            ld, sk, in_shape, n, wseed = netspec.net_b_small(width=WIDE), [], (25, 25, 2), 3, 86
        else:
            assert name == 'netb32'
            ld, sk, in_shape, n, wseed = netspec.net_b_small(width=WIDE), [], (32, 32, 32), 3, 87
        pars = netspec.he_init(ld, in_shape, seed=wseed, skips=sk, bias_std=0.05)
        x, seed, chosen = _stable(ld, in_shape, sk, pars, wseed + 100, n)
        print('%s: patches %r of stream %d' % (name, chosen, seed))
        d = dict(ld=ld, sk=sk, in_shape=in_shape, pars=pars, x=x, n=n)
    d['name'] = name
    d['mb'] = 8 if name == 'netc8' else 4
    _MODELS[name] = d
    return d


_ORACLE = {}


def oracle(d, pars, x, key):
    """fp64 truth and fp32 yardstick of (pars, x): p [2, n], S [n, L], sizes, and the fp64 details.  Cached under `key`."""
    if key in _ORACLE:
        return _ORACLE[key]
    import torch
    assert fragile_units(OracleModel(d['ld'], d['in_shape'], pars, skips=d['sk'], dtype=torch.float64), x) == 0, (key, 'a fragile decision in fp64')
    det = {}
    p64, S64, sizes = factored_ref.factored_unit_scores(OracleModel(d['ld'], d['in_shape'], pars, skips=d['sk'], dtype=torch.float64), x.astype(np.float64), details=det)
    p32, S32, _ = factored_ref.factored_unit_scores(OracleModel(d['ld'], d['in_shape'], pars, skips=d['sk']), x)
    assert S32.dtype == np.float32 and S64.dtype == np.float64
    r = dict(p64=p64, S64=S64, p32=p32, S32=S32, sizes=sizes.astype(np.float64), det=det)
    _ORACLE[key] = r
    return r


ROUTES = OrderedDict([('default', ({}, None)), ('no_f16_derived', ({'ALQ_NO_F16_DERIVED': '1'}, None)), ('no_f16x2', ({'ALQ_NO_F16X2': '1'}, None)),
                      ('knob4', ({}, 4)), ('no_v3_f16_fwd', ({'ALQ_NO_V3_F16_FWD': '1'}, None))])
INFO_FWD = (1, 6, 10, 12)
INFO_BWD = (2, 8, 9, 11, 13, 17)


def _mk(sess, d, pars, route='default', mb=None):
    from nnal_amd import device
    with _env(ROUTES[route][0]):
        m = device.DeviceModel(sess, d['ld'], d['in_shape'], d['sk'], max_batch=mb or d['mb'])
        with _knob(sess, ROUTES[route][1]):
            m.set_weights(pars)
    return m


def _fisher(sess, m, x, route='default'):
    """One Fisher pass: p1, g0, g1, S (what = 4) as numpy, and the engine info of the pass."""
    n = len(x)
    with _knob(sess, ROUTES[route][1]):
        r = m.fisher_device(_dev(sess, x), n, None, 1e-3, want=('p1', 'g0', 'g1'))
        out = {k: r[k].cpu().numpy() for k in ('p1', 'g0', 'g1')}
        out['S'] = _copy(sess, m, 0, 4, n, (n, m.L)).astype(np.float64)
        out['info'] = tuple(int(sess.lib.alq_model_engine_info(m._m, k)) for k in INFO_FWD + INFO_BWD)
    for k in ('p1', 'g0', 'g1', 'S'):
        assert np.isfinite(out[k]).all(), k
    return out


def _try_copy(sess, m, layer, what, n, shape):
    """_copy, or None where the last pass produced none (ALQ_EUNSUPPORTED)."""
    torch = sess.torch
    buf = torch.zeros((int(np.prod(shape)) + 64,), dtype=torch.float32, device=sess.device)
    e = C.c_int64()
    rc = m.lib.alq_model_debug_copy(m._m, int(layer), int(what), int(n), C.c_void_p(buf.data_ptr()), C.byref(e))
    if rc == ALQ_EUNSUPPORTED:
        return None
    assert rc == 0 and e.value == int(np.prod(shape)), (layer, what, rc, e.value)
    torch.cuda.synchronize()
    return buf[:e.value].cpu().numpy().reshape(shape)


_RATIOS = []


def fp64_bar(tag, dev, o, names, exact_cols=None):
    """Bar (d) on the unit-cotangent layer scores g = S / size [n, L] and on g0 = p1 g, g1 = -(1 - p1) g: per layer column,
    e_dev <= 4 R e_32 + 6e-8 mean |ref|, never looser than 2e-4 max |ref| + 1e-9; p1 within 2e-6 of fp64.  Prints every figure."""
    p1_64 = o['p64'][1]
    e_p = np.abs(dev['p1'].astype(np.float64) - p1_64).max()
    print('%s | p1: max |dev - fp64| %.3e (bar 2e-6)' % (tag, e_p))
    bad = []
    if not e_p <= 2e-6:
        bad.append(('p1', e_p))
    g64 = o['S64'] / o['sizes']
    g32 = o['S32'].astype(np.float64) / o['sizes']
    # g0 = p1 g, g1 = -(1 - p1) g, and the saturation branch of the query (kernels.hip, fisher_finalize_kernel; PW_NNAL.py:770-814):
    # p1 < 1e-6 leaves g1 = 0, p1 > 1 - 1e-6 leaves g0 = 0
    # (p0 is the softmax's own output, not 1 - p1: next to a saturated p1 it keeps its digits)
    def sat(p, S):
        g = np.asarray(S, np.float64) / o['sizes']
        assert not ((np.abs(p1_64 - 1e-6) < 1e-8) | (np.abs(1 - p1_64 - 1e-6) < 1e-8)).any(), 'a posterior on the branch boundary'
        g0, g1 = np.asarray(p[1], np.float64)[:, None] * g, -np.asarray(p[0], np.float64)[:, None] * g
        return np.where((p1_64 > 1 - 1e-6)[:, None], 0., g0), np.where((p1_64 < 1e-6)[:, None], 0., g1)
    g0_64, g1_64 = sat(o['p64'], o['S64'])
    g0_32, g1_32 = sat(o['p32'], o['S32'])
    refs = OrderedDict([('g', (dev['S'] / o['sizes'], g64, g32)), ('g0', (dev['g0'], g0_64, g0_32)), ('g1', (dev['g1'], g1_64, g1_32))])
    for what, (a, r64, r32) in refs.items():
        for t, nme in enumerate(names):
            e_dev, e_32 = np.abs(a[:, t] - r64[:, t]).max(), np.abs(r32[:, t] - r64[:, t]).max()
            floor = 6e-8 * np.abs(r64[:, t]).mean()
            bar = min(R_FACTOR * R_DEV_OVER_F32 * e_32 + floor, 2e-4 * np.abs(r64[:, t]).max() + 1e-9)
            print('%s | %s | %s | e_dev %.3e | e_32 %.3e | ratio %.3f | floor %.3e | max|ref| %.3e | bar %.3e'
                  % (tag, what, nme, e_dev, e_32, e_dev / max(e_32, 1e-300), floor, np.abs(r64[:, t]).max(), bar))
            if e_32 > floor:
                _RATIOS.append((e_dev / e_32, tag, what, nme))
            if not e_dev <= bar:
                bad.append((what, nme, e_dev, bar))
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------ (b) soundness
def _layer_max(det, n):
    """max |activation| per layer and patch of the fp64 oracle [layers, n]."""
    return np.stack([np.abs(o).max(0) if o.ndim == 2 else np.abs(o).reshape(n, -1).max(1) for o in det['out']])


def _check_bounds(sess, m, d, o, tag, x):
    """The read-back of the last pass on patches x: derived bounds (15), measured maxima (16, 17).  Returns the bounds or None."""
    n, ld, sk, pars = len(x), d['ld'], d['sk'], d['pars']
    nl = len(ld)
    types = scale_ref.layer_types(ld)
    acts = _layer_max(o['det'], n)
    derived = int(sess.lib.alq_model_engine_info(m._m, 6))
    in_amax = _try_copy(sess, m, 0, 17, n, (n,))
    bounds = _try_copy(sess, m, 0, 15, n, (nl, n))
    assert (bounds is not None) == (derived == 1 or in_amax is not None), (tag, derived)
    measured = {}
    for i in range(nl):
        a = _try_copy(sess, m, i, 16, n, (n,))
        if a is None:
            continue
        measured[i] = a
        e = C.c_int64()
        buf = sess.torch.zeros((n * int(np.prod(o['det']['out'][i].shape[1:])) + 64,), dtype=sess.torch.float32, device=sess.device)
        rc = m.lib.alq_model_debug_copy(m._m, i, 0, n, C.c_void_p(buf.data_ptr()), C.byref(e))
        rel = np.abs(a.astype(np.float64) - acts[i]) / acts[i]
        if rc == 0:
            sess.torch.cuda.synchronize()
            t = np.abs(buf[:e.value].cpu().numpy().reshape(n, -1)).max(1)
            print('%s | measured maxima of layer %d (%s): equal to max |stored tensor|; rel. to fp64 %.2e' % (tag, i, list(ld)[i], rel.max()))
            np.testing.assert_array_equal(a.view(np.uint32), t.view(np.uint32), err_msg='%s layer %d' % (tag, i))
        else:
            print('%s | measured maxima of layer %d (%s): tensor not stored; rel. to fp64 %.2e (bar 2^-18)' % (tag, i, list(ld)[i], rel.max()))
        assert (rel <= 2.0 ** -18).all(), (tag, i, rel.max())
    if in_amax is not None:
        np.testing.assert_array_equal(in_amax.view(np.uint32), np.abs(x.reshape(n, -1)).max(1).astype(np.float32).view(np.uint32), err_msg=tag)
    if bounds is None:
        print('%s | no derived bounds in this pass; measured: %r' % (tag, sorted(measured)))
        return None
    assert np.isfinite(bounds).all()
    from_input = in_amax is not None
    if from_input:
        assert not derived
        start = in_amax
    else:
        assert 0 in measured, (tag, 'the chain starts at layer 0\'s measured maximum')
        start = measured[0]
        np.testing.assert_array_equal(bounds[0].view(np.uint32), start.view(np.uint32))
    chain = scale_ref.l1_chain(pars, ld, sk, start.astype(np.float64), 1 if from_input else 0)
    b64 = bounds.astype(np.float64)
    assert (b64 <= chain * (1 + 2.0 ** -20)).all() and (b64 >= chain * (1 - 2.0 ** -20)).all(), (tag, np.max(b64 / chain), np.min(b64 / chain))
    behind_param = from_input
    for i in range(nl):
        behind_param = behind_param or (i > 0 and types[i] in ('conv', 'conv_transpose'))
        ratio = b64[i] / acts[i]
        print('%s | layer %d (%s): bound / fp64 max in [%.4g, %.4g]%s' % (tag, i, list(ld)[i], ratio.min(), ratio.max(), '' if behind_param else ' (the measurement itself)'))
        if behind_param:
            assert (b64[i] >= acts[i]).all(), (tag, i, ratio.min())
        else:
            assert (np.abs(ratio - 1) <= 2.0 ** -18).all(), (tag, i, ratio)
    return bounds


@pytest.mark.parametrize('name', ('netc32', 'netc8', 'netb25', 'netb32'))
def test_bounds_and_maxima_are_sound(sess, name):
    """(b) of the module docstring after a Fisher pass and after a forward-only pass; patch 0 and the last patch alone give the same
    bound bits as in the full batch; the cotangent bounds (18) bound the fp64 oracle's masked cotangents and the device's own
    (what = 1) where the pass stored them."""
    d = model(name)
    o = oracle(d, d['pars'], d['x'], name)
    n, nl = d['n'], len(d['ld'])
    # patches of very different magnitude: the bounds are per patch
    m = _mk(sess, d, d['pars'])
    t = _dev(sess, d['x'])
    seen = 0
    for kind in ('fisher', 'forward'):
        if kind == 'fisher':
            m.fisher_device(t, n, None, 1e-3, want=('p1',))
        else:
            m.forward_device(t, n)
        bounds = _check_bounds(sess, m, d, o, '%s %s' % (name, kind), d['x'])
        if bounds is not None:
            seen += 1
            for i in (0, n - 1):
                if kind == 'fisher':
                    m.fisher_device(t[i:i + 1], 1, None, 1e-3, want=('p1',))
                else:
                    m.forward_device(t[i:i + 1], 1)
                alone = _try_copy(sess, m, 0, 15, 1, (nl, 1))
                np.testing.assert_array_equal(alone[:, 0].view(np.uint32), bounds[:, i].view(np.uint32), err_msg='%s %s patch %d alone' % (name, kind, i))
    # NET-C at 8^3 has no launch on derived bounds (no first conv + pool kernel, no f3d / d3d plan): only its measured maxima are checked
    assert (seen >= 1) == (name != 'netc8'), (name, seen)
    # cotangent bounds of the Fisher backward
    m.forward_device(t, n)
    assert _try_copy(sess, m, 0, 18, n, (nl,)) is None          # refused after a forward-only call
    m.fisher_device(t, n, None, 1e-3, want=('p1',))
    cb = _copy(sess, m, 0, 18, n, (nl,))
    names = list(d['ld'])
    pidx = [i for i, ty in enumerate(scale_ref.layer_types(d['ld'])) if ty != 'pool']
    assert cb[nl - 1] == 1.0
    for t_, i in enumerate(pidx):
        truth = np.abs(o['det']['delta'][t_]).max()
        e = C.c_int64()
        buf = sess.torch.zeros((int(o['det']['delta'][t_].size) + 64,), dtype=sess.torch.float32, device=sess.device)
        rc = m.lib.alq_model_debug_copy(m._m, i, 1, n, C.c_void_p(buf.data_ptr()), C.byref(e))
        sess.torch.cuda.synchronize()
        own = float(np.abs(buf[:e.value].cpu().numpy()).max()) if rc == 0 else None
        print('%s | cotangent bound of layer %d (%s): %.4g, fp64 max %.4g, device max %s' % (name, i, names[i], cb[i], truth, own))
        if cb[i] < 0:
            continue
        assert cb[i] >= truth, (name, i, cb[i], truth)
        if own is not None and abs(own - truth) <= 1e-4 * truth:      # (a buffer the fused launches did not write holds something else)
            assert cb[i] >= own, (name, i, cb[i], own)
    assert (cb[pidx[1:]] > 0).any()
    m.close()


def _tight_pars(d):
    """d's weights with the first layer's bias arranged so that the channel of the largest L1 norm holds +max |b|: the bound
    amax * L1 + max |b| is then attained, through the ReLU."""
    pars = OrderedDict((nme, [np.array(W), np.array(b)]) for nme, (W, b) in d['pars'].items())
    first = list(pars)[0]
    W, b = pars[first]
    _, _, co = scale_ref.tight_input(W, b, 1.0, d['in_shape'])
    b[co] = np.abs(b).max()
    return pars, first, co


@pytest.mark.parametrize('amax', (1.0, 2.0 ** -9, 37.0))
@pytest.mark.parametrize('name', ('netb25', 'netb32'))
def test_tight_input_on_the_igemm3_route(sess, name, amax):
    """The input that attains layer 0's L1 bound at one voxel: the derived layer-0 bound of the pass (from the measured input
    maximum) is >= the fp64 oracle's |out| there and <= (1 + 1e-5) times it; the pass's scores meet the fp64 bar."""
    d = model(name)
    pars, first, co = _tight_pars(d)
    W, b = pars[first]
    x1, voxel, co2 = scale_ref.tight_input(W, b, amax, d['in_shape'])
    assert co2 == co
    x = x1[None]
    import torch
    det = {}
    p64, S64, sizes = factored_ref.factored_unit_scores(OracleModel(d['ld'], d['in_shape'], pars, skips=d['sk'], dtype=torch.float64), x.astype(np.float64), details=det)
    p32, S32, _ = factored_ref.factored_unit_scores(OracleModel(d['ld'], d['in_shape'], pars, skips=d['sk']), x)
    out = float(det['out'][0][(0,) + voxel + (co,)])
    assert out > 0 and out == np.abs(det['out'][0]).max()
    m = _mk(sess, d, pars)
    r = _fisher(sess, m, x)
    in_amax = _try_copy(sess, m, 0, 17, 1, (1,))
    assert in_amax is not None and in_amax[0] == np.float32(amax), 'the pass did not scale layer 0 by the measured input maximum'
    bound = float(_copy(sess, m, 0, 15, 1, (len(d['ld']), 1))[0, 0])
    m.close()
    print('%s amax %g: layer-0 bound %.9g, fp64 |out| at the voxel %.9g, ratio - 1 = %.3e' % (name, amax, bound, out, bound / out - 1))
    assert bound >= out and bound <= (1 + 1e-5) * out
    o = dict(p64=p64, S64=S64, p32=p32, S32=S32, sizes=sizes.astype(np.float64))
    fp64_bar('%s tight amax %g' % (name, amax), r, o, list(pars))


# ------------------------------------------------------------------------------------------ (c) exact equivariance
_BASE = {}


def _base(sess, name, route):
    if (name, route) not in _BASE:
        d = model(name)
        m = _mk(sess, d, d['pars'], route)
        _BASE[(name, route)] = _fisher(sess, m, d['x'], route)
        m.close()
    return _BASE[(name, route)]


def _equivariance(sess, name, layer, k, route, zero_bias=False):
    d = model(name)
    ld, sk = d['ld'], d['sk']
    pnames = list(d['pars'])
    base_pars, x, key = d['pars'], d['x'], name
    if zero_bias:      # another function: its own stable patches
        key = name + '/b0'
        if key not in _MODELS:
            bp = OrderedDict((nme, [W, np.zeros_like(b)]) for nme, (W, b) in d['pars'].items())
            _MODELS[key] = (bp, _stable(ld, d['in_shape'], sk, bp, 400, d['n'])[0])
        base_pars, x = _MODELS[key]
    tag = '%s%s | %s | %s k=%d' % (name, ' zero bias' if zero_bias else '', route, layer, k)
    if (key, route) not in _BASE:
        m = _mk(sess, d, base_pars, route)
        _BASE[(key, route)] = _fisher(sess, m, x, route)
        m.close()
    base = _BASE[(key, route)]
    p2, kx = scale_ref.rescale(base_pars, ld, sk, layer, k)
    x2 = np.ldexp(x, kx)
    m = _mk(sess, d, p2, route)
    got = _fisher(sess, m, x2, route)
    m.close()
    assert got['info'] == base['info'], (tag, 'rescaling changed the route', got['info'], base['info'])
    names = list(ld)
    cons = [pnames.index(names[i]) for i, _ in scale_ref.consumers(ld, sk, layer)]
    j = pnames.index(layer) if layer != 'input' else None
    src2 = scale_ref.skip_src_of(ld, sk)
    into_concat = any(src2[i] >= 0 for i, _ in scale_ref.consumers(ld, sk, layer))
    assert into_concat == (layer in _INTO_CONCAT)
    exact = route == 'knob4' or not into_concat
    # the power-of-two correction of layer j's own column: exact
    fixed = {kk: np.array(got[kk]) for kk in ('S', 'g0', 'g1')}
    if j is not None:
        for kk in fixed:
            fixed[kk][:, j] = np.ldexp(fixed[kk][:, j], k)
    if exact:
        np.testing.assert_array_equal(got['p1'].view(np.uint32), base['p1'].view(np.uint32), err_msg=tag + ' p1')
        same = [t for t in range(len(pnames)) if t not in cons]
        for kk in ('S', 'g0', 'g1'):
            np.testing.assert_array_equal(fixed[kk][:, same], base[kk][:, same], err_msg='%s %s' % (tag, kk))
    # what is not exact: against fp64 (the consumers' columns; every column behind a skip source)
    o = oracle(d, p2, x2, (key, layer, k))
    fp64_bar(tag, got, o, pnames)
    return got


NETC_LAYERS = ('input', 'enc1', 'enc2', 'bott', 'up1', 'dec1', 'up2', 'dec2')
NETB_LAYERS = ('input', 'conv1', 'conv2', 'conv3', 'conv4')
_INTO_CONCAT = ('enc1', 'enc2', 'up1', 'up2')      # a consumer of their output reads it as one slice of a concat


def _ks(i, layer):
    if layer in _INTO_CONCAT:
        return (12, -12)
    return (12, -37) if i % 2 == 0 else (37, -12)


DEFAULT_CASES = [(n, l, k) for n in ('netc32', 'netc8') for i, l in enumerate(NETC_LAYERS) for k in _ks(i, l)] + \
                [(n, l, k) for n in ('netb25', 'netb32') for i, l in enumerate(NETB_LAYERS) for k in _ks(i, l)]
ROUTE_CASES = [(n, r, l, k) for n in ('netc32', 'netc8') for r in ('no_f16_derived', 'no_f16x2', 'knob4')
               for l, k in (('input', 37), ('enc2', -12), ('dec1', -37))] + \
              [(n, 'no_v3_f16_fwd', l, k) for n in ('netb25', 'netb32') for l, k in (('input', -37), ('conv2', 12), ('conv4', 37))]


@pytest.mark.parametrize('name,layer,k', DEFAULT_CASES, ids=['%s-%s-%d' % c for c in DEFAULT_CASES])
def test_rescaled_model_same_bits_default_route(sess, name, layer, k):
    _equivariance(sess, name, layer, k, 'default')


@pytest.mark.parametrize('name,route,layer,k', ROUTE_CASES, ids=['%s-%s-%s-%d' % c for c in ROUTE_CASES])
def test_rescaled_model_same_bits_other_routes(sess, name, route, layer, k):
    got = _equivariance(sess, name, layer, k, route)
    if name == 'netc32' and route != 'default':      # the arm is another route than the default: no derived bounds on any of them
        assert got['info'][1] == 0 and _base(sess, name, 'default')['info'][1] == 1, (route, got['info'])


@pytest.mark.parametrize('name', ('netc32', 'netc8'))
@pytest.mark.parametrize('layer,k', (('input', -12), ('bott', 37), ('dec1', 12)))
def test_rescaled_model_same_bits_zero_bias(sess, name, layer, k):
    """Every bias zero: out_bmax = 0, flip_bias_nonzero off, bound = L * in exactly."""
    _equivariance(sess, name, layer, k, 'default', zero_bias=True)


# ------------------------------------------------------------------------------------------ (d) against fp64
def _variant(d, what):
    pars = OrderedDict((nme, [np.array(W), np.array(b)]) for nme, (W, b) in d['pars'].items())
    if what == 'bias_x1024':
        for nme in pars:
            pars[nme][1] = np.ldexp(pars[nme][1], 10)
    elif what == 'zero_bias':
        for nme in pars:
            pars[nme][1][...] = 0
    else:
        up, down = what
        pars[up][0] *= np.float32(37.0)
        pars[down][0] *= np.float32(2.0 ** -9)
    return pars


VARIANTS = [('netc32', 'bias_x1024'), ('netc32', 'zero_bias'), ('netc32', ('dec2', 'enc2')), ('netc8', 'bias_x1024'), ('netc8', ('bott', 'dec1')),
            ('netb32', 'bias_x1024'), ('netb32', ('conv4', 'conv2')), ('netb25', 'zero_bias')]


@pytest.mark.parametrize('name,what', VARIANTS, ids=['%s-%s' % (n, w if isinstance(w, str) else '37x%s_2m9x%s' % w) for n, w in VARIANTS])
def test_other_functions_against_fp64(sess, name, what):
    """Another function than the base model's (a bias 2^10 times he_init's dominates every bound; no bias; one layer 37 times and one
    2^-9 times its draw as in test_gpu_weights_reset): its own stable patches, the fp64 bar, and the bounds of (b) on it."""
    d = model(name)
    pars = _variant(d, what)
    x, seed, chosen = _stable(d['ld'], d['in_shape'], d['sk'], pars, 300, d['n'])
    tag = '%s %s' % (name, what if isinstance(what, str) else '37x%s 2^-9x%s' % what)
    print('%s: patches %r of stream %d' % (tag, chosen, seed))
    o = oracle(d, pars, x, (name, str(what)))
    m = _mk(sess, d, pars)
    r = _fisher(sess, m, x)
    _check_bounds(sess, m, dict(d, pars=pars), o, tag, x)
    m.close()
    fp64_bar(tag, r, o, list(pars))


# ------------------------------------------------------------------------------------------ (e) the ends of the range
ENDS = [(n, l, k) for n, l in (('netc32', 'input'), ('netc32', 'enc2'), ('netb32', 'input')) for k in (-90, -64, 64, 90)]


@pytest.mark.parametrize('name,layer,k', ENDS, ids=['%s-%s-%d' % c for c in ENDS])
def test_ends_of_the_range(sess, name, layer, k):
    """Far from the centre of every exponent window.  On the CPU first: the bound chain and every fp64 activation stay inside
    [2^-120, 2^120].  Then every output finite, p1 within 2e-6 of the base model's, the scores on the fp64 bar after the exact
    power-of-two correction.

    enc2 at these k puts dec1's two weight slices 2^64 and 2^90 apart: the model then runs on bf16 triples (module docstring,
    (e)); the engine info must say so, and must be the base model's for the input cases."""
    d = model(name)
    p2, kx = scale_ref.rescale(d['pars'], d['ld'], d['sk'], layer, k)
    x2 = np.ldexp(d['x'], kx)
    o = oracle(d, p2, x2, (name, layer, k))
    acts = _layer_max(o['det'], d['n'])
    if name.startswith('netb'):      # igemm3's chain starts at the input maxima, NET-C's at layer 0's measured output maxima
        chain = scale_ref.l1_chain(p2, d['ld'], d['sk'], np.abs(x2.reshape(d['n'], -1)).max(1), 1)
    else:
        chain = scale_ref.l1_chain(p2, d['ld'], d['sk'], acts[0], 0)
    # NET-C: the rows a launch consumes end at up1 (f3d reads pool1's, d3d up1's and enc2's); behind dec1 the chain multiplies the
    # larger slice's bound with the norm of BOTH slices and only has to stay finite
    used = chain if name.startswith('netb') else chain[:list(d['ld']).index('up1') + 1]
    assert (acts > 2.0 ** -120).all() and (acts < 2.0 ** 120).all() and (used > 2.0 ** -120).all() and (used < 2.0 ** 120).all()
    assert (chain < 2.0 ** 127).all()
    base = _base(sess, name, 'default')
    m = _mk(sess, d, p2)
    got = _fisher(sess, m, x2)
    m.close()
    tag = '%s | ends | %s k=%d' % (name, layer, k)
    if layer == 'enc2':      # dec1's two weight slices lie 2^64 or more apart: the model left the fp16-pair launches (c3d, derived, d3d, f3d)
        assert got['info'][:4] == (0, 0, 0, 0) and base['info'][:4] == (1, 1, 1, 1), (tag, got['info'], base['info'])
    else:
        assert got['info'] == base['info'], (tag, got['info'], base['info'])
    e_p = np.abs(got['p1'].astype(np.float64) - base['p1']).max()
    print('%s | max |p1 - base p1| %.3e' % (tag, e_p))
    assert e_p <= 2e-6, (tag, e_p)
    fp64_bar(tag, got, o, list(d['pars']))
