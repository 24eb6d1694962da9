"""The skinny fully connected layers (cout <= 8) and the two-class head on their own: every kernel form against the fp64 statement of
the layer in tests/fc_small_ref.py (GPU box).

plan_fc (csrc/model.hip) routes every fc layer with cout <= 8 to a family of small kernels in csrc/kernels.hip - fc_small_fwd_kernel
<NOUT, BITS> + fc_small_finish_kernel, fc_small_finish_diff_kernel behind the fused head, fc_small_bwd_kernel<G>,
fc_small_bwd_scalar_kernel, fc_small_dsum_bits_kernel, flip_scan_kernel / flip_fix_kernel, rowmax_u32_kernel, softmax_kernel - and
weights.hip builds d_Wp (activation-memory order), wv = W0 - W1 and its 16-bit pieces for them.  The rest of the suite runs the
family as the tail of whole models and judges it through scores.  Here: models built through device.DeviceModel, internals read
with alq_model_debug_copy (index 14, the head's sign bytes, was added for this file), helpers of tests/test_gpu_convt.py.

Checks:
  1  first-layer models fc(F -> c), integer x, W and b (tests/fc_small_ref.FIRST): the logits EQUAL the fp64 statement after
     alq_forward and after alq_fisher (c != 2: alq_fisher is refused behind its forward pass, "Fisher scoring is binary"; the
     refusal is asserted and the logits of that pass are still compared), N in {1, 3, 5} under max_batch = 4.  c = 1 is refused at
     model creation (the refusal and its text are the check; NOUT = 1 runs as the hidden layer fc(F -> 1, 'MA') -> fc(2)); c = 9
     runs with no fc_small launch.  fc(F -> 8 | 1, 'MA') -> fc(2): the finish kernel's ReLU, and a backward launch of N * 2
     threads (8 hidden units: G = 2) or N (one hidden unit: the scalar kernel), fewer than a wave.
  2  softmax_kernel through fc(c -> c) with identity weights: designed logits, |p - p64| <= K e_32 + 2^-24, predictions exact.
  3  below-conv models conv(8) -> conv(C, ops) [-> pool] -> fc(c) on float inputs (fc_small_ref.BELOW): the fc layer's input
     activation and its own cotangent are read from the device and taken as given; logits, the cotangent of the layer below
     (masked where that layer has a ReLU), its channel-sum field after a Fisher pass and the layer's dW / db rows follow in fp64
     under tests/test_gpu_convt._bar, unchanged.  The form a case names (G = C / 4 lanes per voxel, G = 0, the scalar kernel)
     follows from (C, F % 4, pool) in k_fc_small_bwd: tests/test_fc_small_ref_host.py holds the table to that rule, and every pass
     here asserts its fc_small launch count (forward 2; Fisher pass and general sweep 3).
  4  the two-class bits head conv(8) -> conv(8) -> fc(2), F % 1024 == 0: integer inputs (everything EQUAL: logits, the
     logit-difference partials of the fused head, sign bytes, the channel sums of fc_small_dsum_bits_kernel, the cotangent below)
     on every route and N in {1, 7, 8, 9}; float inputs (the same under _bar, posteriors within 2e-6 of the ALQ_NO_FC_BITS arm, sign
     bytes equal to act > 0 of that arm, FLIP_OVERFLOW 0); heads that must not take the bits; NET-C at 32^3 for the plane-sweep
     engine's 4 partials.
  5  whole models through tests/test_gpu_convt.whole_record and its check_* bodies.

Which form a case is in is asserted from the profiler's fc_small launch count per pass, alq_model_engine_info(1 | 5), the element
count of debug index 5 (the fused head's partials per patch; the call is refused where the last pass did not run the fused head)
and whether debug index 14 exists (the head keeps sign bytes).  Measured on an MI355X (2026-10-20): the head is fused at 8x12x12
(16 partials per patch), 16^3 (32) and 32^3 (256: the only geometry tried with more than 64, the two-slot tile being 512 voxels
there); at F = 1024 (4x4x8, 8x16) the head keeps the bits - fc_small_fwd_kernel<2, true> writes them - but the conv's plans are not
the forms the bits need (plan_fc, head_bits_apply), so the backward launch is fc_small_bwd_kernel<2> on the stored activation:
fc_small_dsum_bits_kernel and the conv's backward launch from the bits run from 8x12x12 up (one-line corruptions of either kernel
fail exactly these cases); knob 5 takes the conv off the two-slot engine: bits written, head not fused.

FORMS_UNREACHABLE lists what no case reaches or no evidence can show, with the reasons.

Runtime of the file on an MI355X, 2026-10-20: 4.0 s (RUNTIME below; tests/test_gpu_convt.py: 6.5 s in the same session).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec, tfops  # noqa: E402
from tests import conv_ref  # noqa: E402
from tests import fc_small_ref as R  # noqa: E402
from tests.test_gpu_convt import (_bar, _copy, _dev, _figure, _knob, _make, _passes, check_fisher_pass, check_other_entry_points,  # noqa: E402,F401
                                  check_packing, check_param_grads, whole_record)

# Largest e_dev / e_32 of softmax_kernel over the designed and the random logits of check 2, measured on an MI355X on 2026-10-20:
# 1.000 (the device's posteriors carried the same error as torch's fp32 softmax on every row: e_dev 1.089e-07 at c = 8); times 2
# for another exp implementation.
K_SOFTMAX_MEASURED = 1.000
K_SOFTMAX = 2.0 * K_SOFTMAX_MEASURED
# Largest e_dev / e_32 over the 531 of the file's 628 figures whose e_dev exceeds the floor 6e-8 mean |ref64| (below it the floor
# alone carries the assertion), measured on an MI355X on 2026-10-20; the bar is tests/test_gpu_convt._bar, unchanged
# (e_dev <= 4 x 5.092 e_32 + floor, never looser than 2e-4 max |ref64| + 1e-9), and no figure came nearer to it than 0.15 of it:
#   checks 3 and 4   2.759  cotangent below the head conv (8x12x12-Ci16, knob 5: e_dev 3.126e-08, e_32 1.133e-08, max |ref64| 6.6e-02)
#                    2.283  logits (C16-c2, mode 0 class 1, patch 4: 8.289e-08, 3.632e-08); 2.254 channel sums (C8-c2-2d, Fisher pass);
#                    1.496  masked cotangent below the fc layer; 1.000 dW / db rows and the head conv's masked cotangent
#                    0.312  the plane-sweep head's 4 partials, NET-C at 32^3 (4.432e-06 against fp32 torch's 1.421e-05 over 262144
#                           terms); 0.052 the two-slot head's partials (8x12x12: 1.881e-07, 3.645e-06)
#   check 5          3.079  fc/b, mode 1 batch sum of the hidden chain (2.207e-08, 7.168e-09)
R_MEASURED = 3.079
# The file's 61 tests on an MI355X, 2026-10-20: 4.0 s (pytest's own figure; the slowest call 0.15 s, the 32^3 chain);
# tests/test_gpu_convt.py in the same session: 6.5 s.  No route of the 32^3 cases had to be thinned for time - they run the three
# routes that differ there (default, no_fc_fuse, no_fc_bits).
RUNTIME = 4.0

N = 5
ROUTES = OrderedDict([
    ('default', ({}, None)),
    ('no_fc_fuse', ({'ALQ_NO_FC_FUSE': '1'}, None)),
    ('no_fc_bits', ({'ALQ_NO_FC_BITS': '1'}, None)),
    ('no_flipfix', ({'ALQ_NO_FLIPFIX': '1'}, None)),
    ('no_presplit', ({'ALQ_NO_PRESPLIT': '1'}, None)),
    ('no_f16x2', ({'ALQ_NO_F16X2': '1'}, None)),
    ('knob5', ({}, 5)),
])
NOT_FUSED = ('no_fc_fuse', 'no_fc_bits', 'knob5')
# partials per patch of the fused head (debug index 5) by geometry; None: the head is not fused there (F = 1024)
PARTIALS = {'4x4x8': None, '8x16': None, '8x12x12': 16, '8x12x12-Ci16': 'at most 64', '16x16x16': 32, '32x32x32': 256}

# (form, why no case of this file shows it)
FORMS_UNREACHABLE = [
    ('fc_small_fwd_kernel<1, *> as the last layer', 'alq_model_create refuses one class ("1 classes unsupported"); NOUT = 1 runs as a hidden layer'),
    ('fc_small_fwd_kernel<NOUT != 2, true>', 'the sign bytes exist only for a two-class last layer (plan_fc)'),
    ('the fused head and fc_small_dsum_bits_kernel at F = 1024', 'the conv plans of 4x4x8 and 8x16 are not the pair form: no fc_part2, head_bits_apply false; the smallest geometry with both is 8x12x12'),
    ('flip_fix_kernel: list path against sweep path', 'nothing counts the marked groups below the overflow; the sweep path is test_gpu_parity\'s overflow test'),
    ('flip_fix_kernel<16, 3, 3, 3> against <0, 0, 0, 0>', 'chosen by (Ci, k) alone in k_flip_fix: the Ci = 16 cases run the first, the Ci = 8 cases the second; no launch count tells them apart'),
    ('fc_small_bwd_kernel<G>: which G', 'chosen by (C, F % 4, dsum) alone in k_fc_small_bwd; the table is held to that rule on the host'),
    ('rowmax_u32_kernel on its own', 'no debug index reads the per-patch maxima it folds; they scale the fp16 pairs of the launch that follows, which the '
     'exact integer cases and the figures of the cotangent below the head conv cover'),
    ('alq_fisher behind a head of c != 2 classes', 'refused: Fisher scoring is binary; the with-sums forward of such a head runs and is compared'),
]


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


# ------------------------------------------------------------------------------------------ helpers
def _mk(sess, ld, in_shape, pars, mb, route='default'):
    return _make(sess, ld, in_shape, (), pars, mb, route, routes=ROUTES)


def _fc_launches(sess, fn):
    """(fn's result, the fc_small launch count of the profiler over fn())."""
    sess.prof_reset()
    sess.prof_enable(1)
    try:
        out = fn()
        sess.torch.cuda.synchronize()
    finally:
        sess.prof_enable(False)
    return out, sess.prof_read()['fc_small']['launches']


def _try_copy(sess, m, layer, what, n):
    """Element count of a debug index, or None where the library refuses it (ALQ_EUNSUPPORTED = -4)."""
    e = C.c_int64(-1)
    buf = sess.torch.zeros((1 << 20,), dtype=sess.torch.float32, device=sess.device)
    rc = m.lib.alq_model_debug_copy(m._m, int(layer), int(what), int(n), C.c_void_p(buf.data_ptr()), C.byref(e))
    sess.torch.cuda.synchronize()
    assert rc in (0, -4), rc
    return e.value if rc == 0 else None


def _sign_bytes(sess, m, layer, n, F):
    return _copy(sess, m, layer, 14, n, (n, F // 16)).view(np.uint8).reshape(n, F // 4)


def _equal(got, want, msg):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, '%s: %d of %d values differ, first at %r: %r != %r' % (msg, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _fisher(m, t, n):
    return m.fisher_device(t, n, None, 1e-3, want=('p1', 'g0', 'g1'))


def _fisher_or_refusal(m, t, n, c):
    """A Fisher pass; behind a head of c != 2 classes the library refuses it after the forward pass: the refusal is the check."""
    from nnal_amd._lib import AlqError
    if c == 2:
        return _fisher(m, t, n)
    with pytest.raises(AlqError) as ei:
        _fisher(m, t, n)
    assert str(ei.value) == 'libalq error -4: Fisher scoring is binary (PW_NNAL.py:766), got %d classes' % c
    return None


def test_forms_unreachable_have_reasons():
    assert len(FORMS_UNREACHABLE) == 8 and all(len(f) == 2 and len(f[1]) > 20 for f in FORMS_UNREACHABLE)


# ------------------------------------------------------------------------------------------ 1. first-layer models, exact
@pytest.mark.parametrize('c', R.FIRST + [R.WIDE], ids=[c.tag for c in R.FIRST + [R.WIDE]])
def test_first_layer_exact_on_integers(sess, c):
    """fc(F -> c) on the caller's x: the logits of every pass EQUAL the statement (a wrong slice bound, a permuted d_Wp row or a
    dropped tail element moves an integer sum); posteriors within 2e-6, predictions exact."""
    from nnal_amd._lib import AlqError
    ld = R.first_model(c)
    x, W, b = R.exact_fc_inputs(max(R.BATCHES), c.in_shape, c.c, seed=100 + len(c.tag))
    pars = OrderedDict([('fc', [W, b.reshape(-1, 1)])])
    if c.c == 1:
        with pytest.raises(AlqError) as ei:
            _mk(sess, ld, c.in_shape, pars, 4)
        assert str(ei.value) == 'libalq error -4: 1 classes unsupported'
        return
    want = R.logits64(x, W, b, c.in_shape)
    m = _mk(sess, ld, c.in_shape, pars, 4)
    t = _dev(sess, x)
    skinny = c.c <= 8
    for nb in R.BATCHES:
        for a, e in _passes(nb, 4):
            n = e - a
            (post, pred, _), k = _fc_launches(sess, lambda: m.forward_device(t[a:e], n, want_pred=True))
            assert k == (2 if skinny else 0), (c, k)
            _equal(_copy(sess, m, 0, 0, n, (n, c.c)), want[a:e], '%s, forward pass, patches %d..%d' % (c.tag, a, e - 1))
            p64, pred64 = R.softmax64(want[a:e])
            assert np.array_equal(pred.cpu().numpy(), pred64) and np.abs(post.cpu().numpy().T - p64).max() <= 2e-6
            _, k = _fc_launches(sess, lambda: _fisher_or_refusal(m, t[a:e], n, c.c))
            assert k == (2 if skinny else 0), (c, k)      # the first parameter layer has no backward launch
            _equal(_copy(sess, m, 0, 0, n, (n, c.c)), want[a:e], '%s, Fisher pass, patches %d..%d' % (c.tag, a, e - 1))
    m.close()


@pytest.mark.parametrize('h', [8, 1])
def test_skinny_hidden_layer_exact_on_integers(sess, h):
    """fc(F -> h, 'MA') -> fc(2): fc_small_finish_kernel's ReLU; the head's backward launch has one "voxel" of h channels per patch
    (h = 8: G = 2, N * 2 threads, fewer than a wave; h = 1: F % 4 != 0, the scalar kernel) - its cotangent and channel sums EQUAL the
    statement too; the general sweep is held to its launch count here (its figures: the below-conv models)."""
    x, W, b, W2, b2 = R.hidden_inputs(max(R.BATCHES), seed=5)
    W, b, W2 = W[:h], b[:h], W2[:, :h]
    in_shape = (1, 1, R.HIDDEN_F)
    ld = R.hidden_model(h)
    pars = OrderedDict([('hid', [W, b.reshape(-1, 1)]), ('fc', [W2, b2.reshape(-1, 1)])])
    hid = R.logits64(x, W, b, in_shape, relu=True)
    want = R.logits64(hid, W2, b2, (1, 1, h))
    R.assert_exact(hid, W2, b2, (1, 1, h))
    m = _mk(sess, ld, in_shape, pars, 4)
    t = _dev(sess, x)
    for nb in R.BATCHES:
        for a, e in _passes(nb, 4):
            n = e - a
            tag = 'hidden %d, patches %d..%d' % (h, a, e - 1)
            _, k = _fc_launches(sess, lambda: m.forward_device(t[a:e], n))
            assert k == 4, k
            _equal(_copy(sess, m, 0, 0, n, (n, h)), hid[a:e], tag + ', forward pass, hidden layer')
            _equal(_copy(sess, m, 1, 0, n, (n, 2)), want[a:e], tag + ', forward pass, logits')
            _, k = _fc_launches(sess, lambda: _fisher(m, t[a:e], n))
            assert k == 5, k
            _equal(_copy(sess, m, 1, 0, n, (n, 2)), want[a:e], tag + ', Fisher pass, logits')
            delta = np.tile([[1., -1.]], (n, 1))
            _equal(_copy(sess, m, 1, 1, n, (n, 2)), delta, tag + ', the unit cotangent')
            din = R.din64(delta, W2, (1, 1, h), act=hid[a:e])
            _equal(_copy(sess, m, 0, 1, n, (n, h)), din, tag + ', Fisher pass, masked cotangent of the hidden layer')
            _equal(_copy(sess, m, 0, 3, n, (n, 1)), R.chansum64(din, h), tag + ', Fisher pass, channel sums')
            _, k = _fc_launches(sess, lambda: m.param_grads_device(t[a:e], n, 0, cls=1))
            assert k == 5, k
    m.close()


# ------------------------------------------------------------------------------------------ 2. softmax_kernel
def _softmax_logits(c):
    """Designed rows: all equal; two equal maxima, not in first place; +-100 and +-1e4 (posteriors of exactly 0 and 1); random."""
    rows = [np.zeros(c), np.full(c, 3.25), np.full(c, -7.5)]
    two = np.full(c, -1.0)
    two[[c - 2, c - 1] if c > 2 else [0, 1]] = 2.0
    rows.append(two)
    if c > 2:
        two = np.zeros(c)
        two[[1, c - 1]] = 0.5
        rows.append(two)
    for big in (100., 1e4):
        for s in (1., -1.):
            for hot in (0, c - 1):
                r = np.full(c, -s * big)
                r[hot] = s * big
                rows.append(r)
                r = np.zeros(c)
                r[hot] = s * big
                rows.append(r)
    rs = np.random.RandomState(c)
    rows += list(rs.randn(20, c)) + list(10 * rs.randn(20, c)) + list(50 * rs.randn(20, c))
    return np.asarray(rows, np.float32)


@pytest.mark.parametrize('c', [2, 3, 8])
def test_softmax_kernel(sess, c):
    torch = sess.torch
    z = _softmax_logits(c)
    n = len(z)
    pars = OrderedDict([('fc', [np.eye(c, dtype=np.float32), np.zeros((c, 1), np.float32)])])
    m = _mk(sess, OrderedDict([('fc', ['fc', [c]])]), (1, 1, c), pars, n)
    post, pred, _ = m.forward_device(_dev(sess, z), n, want_pred=True)
    _equal(_copy(sess, m, 0, 0, n, (n, c)), z, 'identity weights: x sets the logits')
    m.close()
    post, pred = post.cpu().numpy().T, pred.cpu().numpy()
    p64, pred64 = R.softmax64(z)
    p32 = torch.softmax(torch.tensor(z), dim=1).numpy()
    assert np.isfinite(post).all() and post.dtype == np.float32
    assert np.array_equal(pred, pred64), (pred, pred64)
    assert pred[0] == pred[1] == pred[2] == 0 and pred[3] == (c - 2 if c > 2 else 0)      # the first maximum
    exact = (p64 == 0) | (p64 == 1)
    assert np.count_nonzero(exact) >= 4 * c and (p64[exact] == 1).any() and np.array_equal(post[exact], p64[exact])
    e_dev, e_32 = np.abs(post - p64).max(axis=1), np.abs(p32 - p64).max(axis=1)
    print('FCS_SOFTMAX | c %d | e_dev %.3e | e_32 %.3e | largest row ratio %.3f' % (c, e_dev.max(), e_32.max(), np.max(e_dev / np.maximum(e_32, 1e-300) * (e_dev > 2.0 ** -24))))
    assert np.all(e_dev <= K_SOFTMAX * e_32 + 2.0 ** -24), (c, e_dev.max(), e_32.max())


# ------------------------------------------------------------------------------------------ 3. below-conv models on float inputs
@pytest.mark.parametrize('c', R.BELOW, ids=[c.tag for c in R.BELOW])
def test_below_conv_vs_fp64(sess, c):
    import torch
    ld = R.below_model(c)
    in_shape = tuple(c.size) + (1,)
    seed = 600 + R.BELOW.index(c)
    pars = netspec.he_init(ld, in_shape, seed=seed, bias_std=0.05)
    x = np.random.RandomState(seed + 1000).randn(N, *in_shape).astype(np.float32)
    F, sp = R.below_F(c)
    shape = sp + (c.C,)
    W, b = pars['fc']
    fc, prev = len(ld) - 1, len(ld) - 2
    relu_below = 'A' in c.ops and not c.pool      # the layer right below the fc layer masks its cotangent
    labels = (np.arange(N) % c.c).astype(np.int32)
    m = _mk(sess, ld, in_shape, pars, 4)
    t = _dev(sess, x)
    bad = []
    for a, e in _passes(N, 4):
        n = e - a
        _, k = _fc_launches(sess, lambda: m.forward_device(t[a:e], n))
        assert k == 2, k
        variants = OrderedDict([('mode 0 class %d' % (c.c - 1), dict(mode=0, cls=c.c - 1)), ('mode 0 class 0', dict(mode=0, cls=0)),
                                ('mode 1 rows', dict(mode=1, labels=labels[a:e], loss_scale=1. / N))])
        for vname, kw in list(variants.items()) + ([('Fisher pass', None)] if c.c == 2 else []):
            tag = '%s | %s | patches %d..%d' % (c.tag, vname, a, e - 1)
            if kw is None:
                _, k = _fc_launches(sess, lambda: _fisher(m, t[a:e], n))
            else:
                (rows, _, _), k = _fc_launches(sess, lambda: m.param_grads_device(t[a:e], n, **kw))
                rows = rows.cpu().numpy()
            assert k == 3, (tag, k)
            act = _copy(sess, m, prev, 0, n, (n,) + shape)
            z = _copy(sess, m, fc, 0, n, (n, c.c))
            delta = _copy(sess, m, fc, 1, n, (n, c.c))
            dlow = _copy(sess, m, prev, 1, n, (n, F))
            assert np.count_nonzero(act) and np.count_nonzero(delta), tag
            if 'A' in c.ops:
                assert (act >= 0).all() and np.count_nonzero(act == 0), tag
            if kw is None:
                _equal(delta, np.tile([[1., -1.]], (n, 1)), tag + ', the unit cotangent')
            _figure(bad, tag, 'logits', z, R.logits64(act, W, b, shape), R.logits_torch(act, W, b, shape, torch.float32))
            mask = act if relu_below else None
            d64, d32 = R.din64(delta, W, shape, act=mask), R.din_torch(delta, W, shape, mask, torch.float32)
            _figure(bad, tag, 'cotangent below', dlow, d64, d32)
            if relu_below:
                assert not dlow[act.reshape(n, -1) == 0].any(), tag
            if kw is None and not c.pool:      # the channel-sum field of the conv below (behind a pool the pool's backward writes it)
                _figure(bad, tag, 'channel sums', _copy(sess, m, prev, 3, n, (n, F // c.C)), R.chansum64(d64, c.C), R.chansum_torch(d32, c.C, torch.float32))
            if kw is not None:
                dW64, db64 = R.wgrad64(act, delta, shape)
                dW32, db32 = R.wgrad_torch(act, delta, shape, torch.float32)
                gW = np.stack([m.unflatten(r)[-2] for r in rows])
                gb = np.stack([m.unflatten(r)[-1] for r in rows])
                _figure(bad, tag, 'dW', gW, dW64, dW32)
                _figure(bad, tag, 'db', gb, db64, db32)
    m.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 4. the two-class bits head
def _five(v, nd):
    v = np.asarray(v)
    return v.reshape((len(v),) + (1,) * (3 - nd) + v.shape[1:])


def _conv_geometry(W, size):
    nd = len(size)
    W = np.asarray(W)
    W5 = W.reshape((1,) * (3 - nd) + W.shape)
    lo = [tfops.same_pads(s, k, 1)[1] for s, k in zip((1,) * (3 - nd) + tuple(size), W5.shape[:3])]
    return W5, lo


def _pre64(a_in, W, b, size):
    """The head conv's pre-activation in fp64 from its input activation (taken as given) and the units whose sign another
    arithmetic may see differently: |pre| <= ref64.DEFAULT_EPS x the sample's rms (tests/test_gpu_hvp.fragile_units' rule)."""
    from nnal_amd import ref64
    nd = len(size)
    W5, lo = _conv_geometry(W, size)
    pre = conv_ref.forward64(_five(a_in, nd).astype(np.float64), W5, b, lo).reshape((len(a_in),) + tuple(size) + (W5.shape[-1],))
    rms = np.sqrt((pre ** 2).mean(axis=tuple(range(1, pre.ndim)), keepdims=True))
    return pre, np.abs(pre) <= ref64.DEFAULT_EPS * rms


def _unpack(sb, shape):
    """Sign bytes [n, F / 4] -> bool [n, *shape]."""
    return (((sb[:, :, None] >> np.arange(4)) & 1) > 0).reshape((len(sb),) + tuple(shape))


def _head_refs(pars, a0, a1, mask, torch, Wcv=None):
    """fp64 / fp32 statements of a head over a ReLU conv from the activations a0 (the conv's input) and a1 (its output) and the
    signs `mask` of a1: logits, b0 - b1, the channel sums fc_small_dsum_bits_kernel owes, the masked cotangent of the conv and the
    cotangent of the layer below it under the unit cotangent (+1, -1)."""
    nd = a1.ndim - 2
    shape = a1.shape[1:]
    Wf, bf = pars['fc']
    wm = R.w_mem(np.asarray(Wf, np.float64), shape)
    wv = wm[0] - wm[1]
    dcv = mask * wv.reshape((1,) + shape)      # exact in fp32: one product by 0 or 1 (wv itself is one fp32 subtraction)
    dcv32 = torch.tensor(mask.astype(np.float32)) * (torch.tensor(R.w_mem(np.asarray(Wf, np.float32), shape)[0]) - torch.tensor(R.w_mem(np.asarray(Wf, np.float32), shape)[1])).reshape((1,) + shape)
    out = dict(z=R.logits64(a1, Wf, bf, shape), z32=R.logits_torch(a1, Wf, bf, shape, torch.float32), bdiff=float(bf[0, 0]) - float(bf[1, 0]), ds=dcv.sum(-1), dcv=dcv,
               dcv32=dcv32.numpy(), ds32=dcv32.sum(-1).numpy())
    if a0 is not None:
        W5, lo = _conv_geometry(pars['cv'][0] if Wcv is None else Wcv, shape[:-1])
        out['dl64'] = conv_ref.bwd_data64(_five(dcv, nd), W5, lo, act=_five(a0, nd)).reshape(a0.shape)
        out['dl32'] = conv_ref.bwd_data_torch(_five(dcv, nd).astype(np.float32), W5.astype(np.float32), _five(a0, nd), torch.float32).reshape(a0.shape)
    return out


def _assert_bits_form(sess, m, route, gtag, n, k, tag, fc=2):
    """The form of the last Fisher pass: fused head or not (debug index 5, its element count, the fc_small launches), sign bytes
    or not (debug index 14)."""
    fused = PARTIALS[gtag] is not None and route not in NOT_FUSED
    c5 = _try_copy(sess, m, 0, 5, n)
    assert (c5 is not None) == fused, (tag, c5)
    if fused:      # (a 16-channel input gives the conv another plan: its tile count is held to the class the case is there for)
        assert c5 % (4 * n) == 0 and (4 <= c5 // n <= 64 if PARTIALS[gtag] == 'at most 64' else c5 == n * PARTIALS[gtag]), (tag, c5)
    assert (_try_copy(sess, m, fc, 14, n) is not None) == (route != 'no_fc_bits'), tag
    assert k == (2 if fused else 3), (tag, k)      # finish_diff + dsum_bits | fwd + finish + (dsum_bits or fc_small_bwd)
    assert sess.lib.alq_model_engine_info(m._m, 1) == 0 and sess.lib.alq_model_engine_info(m._m, 5) == 0, tag
    return c5 // n if fused else 0


def _check_bits_buffers(sess, m, gtag, n, fused, bits, r, exact, bad, tag):
    """Every buffer of the last Fisher pass of a bits-head model against the statements `r` (_head_refs); `fused`: the partials
    per patch of the fused head, 0 where the head ran as its own kernels."""
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)      # noqa: E731
    cmp = (lambda what, dev, r64, r32: _equal(dev, r64, tag + ', ' + what)) if exact else (lambda what, dev, r64, r32: _figure(bad, tag, what, dev, r64, r32))
    shape = r['dcv'].shape[1:]
    F, vox = int(np.prod(shape)), int(np.prod(shape[:-1]))
    z = _copy(sess, m, 2, 0, n, (n, 2))
    diff64, diff32 = (r['z'][:, 0] - r['z'][:, 1])[:, None], (r['z32'][:, 0] - r['z32'][:, 1])[:, None]      # ref32: the same sums in fp32 torch
    if fused:
        part = _copy(sess, m, 0, 5, n, (n, fused))
        got = (part.astype(np.float64).sum(axis=1) + r['bdiff'])[:, None]
        cmp('sum of the partials + b0 - b1', f32(got), diff64, diff32)
        cmp('logit difference', z[:, :1], diff64, diff32)
        assert not z[:, 1].any(), tag
    else:
        cmp('logits', z, r['z'], r['z32'])
    if not bits:
        cmp('masked cotangent of the head conv', _copy(sess, m, 1, 1, n, (n, F)), r['dcv'].reshape(n, F), r['dcv32'].reshape(n, F))
    cmp('channel sums of the head conv', _copy(sess, m, 1, 3, n, (n, vox)), r['ds'].reshape(n, vox), r['ds32'].reshape(n, vox))
    cmp('cotangent below the head conv', _copy(sess, m, 0, 1, n, (n,) + r['dl64'].shape[1:]), r['dl64'], r['dl32'])


@pytest.mark.parametrize('negative', [False, True], ids=['mixed', 'all_negative'])
@pytest.mark.parametrize('gtag', ['4x4x8', '8x16', '8x12x12'])
def test_bits_head_exact_on_integers(sess, gtag, negative):
    """Integer x, conv weights and head: every buffer of a Fisher pass EQUALS the fp64 statement, on every route and for N in
    {1, 7, 8, 9} (patch groups of 8 in fc_small_dsum_bits_kernel; 8x12x12 gives it two workgroups with a ragged second).  Patch 0
    is all zero behind both convs (sign bytes 0, logits = bias), `all_negative` makes every pre-activation of every patch negative
    (sign bytes 0 everywhere; default, no_fc_fuse and no_fc_bits), the other patches are mixed (every nibble value occurs)."""
    import torch
    size = R.BITS_GEOMS[gtag]
    nmax = max(R.BITS_N)
    x, pars = R.bits_exact_inputs(nmax, size, seed=40 + len(gtag), negative=negative)
    a0, a1 = R.bits_exact_acts(x, pars)
    F = int(np.prod(size)) * 8
    refs = _head_refs(pars, a0, a1, a1 > 0, torch)
    sb_want = R.sign_bytes(a1)
    in_shape = tuple(size) + (1,)
    t = _dev(sess, x)
    p1 = {}
    for route, (_, knob) in ROUTES.items():
        if negative and route not in ('default', 'no_fc_fuse', 'no_fc_bits'):
            continue
        m = _mk(sess, R.bits_model(len(size)), in_shape, pars, nmax, route)
        with _knob(sess, knob):
            for n in R.BITS_N:
                tag = 'bits %s%s | %s | %d patches' % (gtag, ' all negative' if negative else '', route, n)
                r, k = _fc_launches(sess, lambda: _fisher(m, t[:n], n))
                p1[(route, n)] = r['p1'].cpu().numpy()
                fused = _assert_bits_form(sess, m, route, gtag, n, k, tag)
                if route == 'no_fc_bits':      # the activation itself: what the other routes' sign bytes are the signs of
                    _equal(_copy(sess, m, 1, 0, n, (n,) + tuple(size) + (8,)), a1[:n], tag + ', activation of the head conv')
                else:
                    sb = _sign_bytes(sess, m, 2, n, F)
                    assert np.array_equal(sb, sb_want[:n]), (tag, np.count_nonzero(sb != sb_want[:n]))      # bits 4 - 7 clear
                rn = {key: (v[:n] if isinstance(v, np.ndarray) else v) for key, v in refs.items()}
                _check_bits_buffers(sess, m, gtag, n, fused, route != 'no_fc_bits', rn, True, None, tag)
        m.close()
    for (route, n), p in p1.items():
        assert np.abs(p - p1[('no_fc_bits', n)]).max() <= 2e-6, (route, n)
        assert np.abs(p.astype(np.float64) - R.softmax64(refs['z'][:n])[0][:, 1]).max() <= 2e-6, (route, n)


BITS_FLOAT = OrderedDict([('8x16', (8, 16, 8)), ('8x12x12', (8, 12, 12, 8)), ('8x12x12-Ci16', (8, 12, 12, 16)), ('16x16x16', (16, 16, 16, 8)),
                          ('32x32x32', (32, 32, 32, 8))])


@pytest.mark.parametrize('name', list(BITS_FLOAT))
def test_bits_head_on_float_inputs(sess, name):
    """Float inputs: the activations of both convs are read under ALQ_NO_FC_BITS and taken as given.  On every route the sign bytes
    equal the sign of the head conv's fp64 pre-activation (from its given input) wherever that is not within ref64.DEFAULT_EPS x
    rms of zero - and the patches are the first N of a stream without such a unit, so the bytes equal act > 0 of the
    ALQ_NO_FC_BITS arm everywhere; the partials' sum + b0 - b1, the channel sums and the cotangent below follow in fp64 from the
    route's own signs under _bar; the posteriors lie within 2e-6 of that arm's; FLIP_OVERFLOW stays 0.  `-Ci16`: a 16-channel conv
    below the head conv - flip_fix_kernel<16, 3, 3, 3>; the others run <0, 0, 0, 0>.  32^3 (more than 64 partials per patch): 2
    patches as they come - half a million units leave no patch without a unit that close to zero, the units that are may differ
    and are counted - and the routes thinned to default, no_fc_fuse and no_fc_bits."""
    import torch
    from oracle.model import OracleModel
    from tests import convt_ref
    from tests.test_gpu_hvp import fragile_units
    size, Ci = BITS_FLOAT[name][:-1], BITS_FLOAT[name][-1]
    gtag = name
    big = gtag == '32x32x32'
    n = 2 if big else N
    nd = len(size)
    ld = R.bits_model(nd)
    ld['low'] = ['conv', [Ci, [3] * nd], 'MA']
    in_shape = tuple(size) + (1,)
    seed = 700 + list(BITS_FLOAT).index(name)
    pars = netspec.he_init(ld, in_shape, seed=seed, bias_std=0.05)
    if big:
        x = np.random.RandomState(seed + 1000).randn(n, *in_shape).astype(np.float32)
    else:
        x, chosen = convt_ref.first_stable_patches(OracleModel(ld, in_shape, pars, dtype=torch.float64), in_shape, seed + 1000, n, 4 * n, fragile_units)
        assert len(chosen) == n, 'too few patches without a fragile decision: pick another seed'
    shape = tuple(size) + (8,)
    F = int(np.prod(shape))
    t = _dev(sess, x)
    routes = ['no_fc_bits'] + [r for r in ROUTES if r != 'no_fc_bits' and (not big or r in ('default', 'no_fc_fuse'))]
    bad, p1 = [], {}
    for route in routes:
        m = _mk(sess, ld, in_shape, pars, n, route)
        with _knob(sess, ROUTES[route][1]):
            tag = 'bits %s float | %s' % (name, route)
            r, k = _fc_launches(sess, lambda: _fisher(m, t, n))
            p1[route] = r['p1'].cpu().numpy()
            fused = _assert_bits_form(sess, m, route, gtag, n, k, tag)
            if route == 'no_fc_bits':
                a0 = _copy(sess, m, 0, 0, n, (n,) + tuple(size) + (Ci,))
                a1 = _copy(sess, m, 1, 0, n, (n,) + shape)
                pre, fragile = _pre64(a0, pars['cv'][0], pars['cv'][1], size)
                print('%s: %d of %d units within DEFAULT_EPS x rms of zero' % (tag, np.count_nonzero(fragile), fragile.size))
                assert big or not fragile.any(), tag
                assert np.array_equal((a1 > 0)[~fragile], (pre > 0)[~fragile]) and 0.2 < np.mean(a1 > 0) < 0.8, tag
                mask = a1 > 0
            else:
                sb = _sign_bytes(sess, m, 2, n, F)
                assert not (sb & 0xE0).any() and (route == 'no_flipfix' or not (sb & 0x10).any()), tag
                mask = _unpack(sb & 15, shape)
                assert np.array_equal(mask[~fragile], (pre > 0)[~fragile]), (tag, np.count_nonzero(mask != (pre > 0)))
            _check_bits_buffers(sess, m, gtag, n, fused, route != 'no_fc_bits', _head_refs(pars, a0, a1, mask, torch), False, bad, tag)
        m.close()
    for route, p in p1.items():
        assert np.abs(p - p1['no_fc_bits']).max() <= 2e-6, (route, np.abs(p - p1['no_fc_bits']).max())
    assert not bad, bad


@pytest.mark.parametrize('case', R.NO_BITS, ids=[t[0] for t in R.NO_BITS])
def test_heads_that_must_not_take_the_bits(sess, case):
    """F % 1024 != 0, a 16-channel conv, three classes, the head conv as the first parameter layer: no sign bytes (debug index 14
    refused), no fused head (index 5 refused), the plain launches (forward 2; Fisher pass 3) - and the logits, the masked cotangent
    and the channel sums still follow from the activation in fp64 under _bar."""
    import torch
    tag, size, Cc, c, first = case
    nd = len(size)
    ld = R.bits_model(nd, Cc, c, first)
    in_shape = tuple(size) + (1,)
    pars = netspec.he_init(ld, in_shape, seed=800 + len(tag), bias_std=0.05)
    x = np.random.RandomState(900 + len(tag)).randn(N, *in_shape).astype(np.float32)
    fc, prev = len(ld) - 1, len(ld) - 2
    shape = tuple(size) + (Cc,)
    F = int(np.prod(shape))
    W, b = pars['fc']
    m = _mk(sess, ld, in_shape, pars, 4)
    t = _dev(sess, x)
    bad = []
    for a, e in _passes(N, 4):
        n = e - a
        _, k = _fc_launches(sess, lambda: m.forward_device(t[a:e], n))
        assert k == 2 and _try_copy(sess, m, 0, 5, n) is None, (tag, k)
        _, k = _fc_launches(sess, lambda: _fisher_or_refusal(m, t[a:e], n, c))
        assert k == (3 if c == 2 else 2) and _try_copy(sess, m, 0, 5, n) is None and _try_copy(sess, m, fc, 14, n) is None, (tag, k)
        lab = 'no bits %s | patches %d..%d' % (tag, a, e - 1)
        act = _copy(sess, m, prev, 0, n, (n,) + shape)
        _figure(bad, lab, 'logits', _copy(sess, m, fc, 0, n, (n, c)), R.logits64(act, W, b, shape), R.logits_torch(act, W, b, shape, torch.float32))
        if c == 2:
            delta = np.tile([[1., -1.]], (n, 1)).astype(np.float32)
            d64, d32 = R.din64(delta, W, shape, act=act), R.din_torch(delta, W, shape, act, torch.float32)
            if not first:      # (the first parameter layer's cotangent is only summed)
                _figure(bad, lab, 'cotangent below', _copy(sess, m, prev, 1, n, (n, F)), d64, d32)
            _figure(bad, lab, 'channel sums', _copy(sess, m, prev, 3, n, (n, F // Cc)), R.chansum64(d64, Cc), R.chansum_torch(d32, Cc, torch.float32))
    m.close()
    assert not bad, bad


def test_netc_32cube_plane_sweep_head(sess):
    """NET-C at 32^3, 2 patches: the plane-sweep engine (alq_model_engine_info(1) == 1) leaves 4 partials per patch, summed by
    fc_small_finish_diff_kernel.  dec2's output (after the Fisher pass) and input (enc1 | up2, after a general sweep, which keeps
    every activation) are read under ALQ_NO_FC_BITS and taken as given: the sum
    of the partials + b0 - b1 and the logits against the fp64 statement (_bar), the sign bytes against the sign of dec2's fp64
    pre-activation wherever that is not within DEFAULT_EPS x rms of zero, posteriors within 2e-6 of that arm's."""
    import torch
    ld, sk = netspec.net_c()
    names = list(ld)
    in_shape = (32, 32, 32, 1)
    n = 2
    pars = netspec.he_init(ld, in_shape, seed=14, skips=sk, bias_std=0.05)
    x = np.random.RandomState(1004).randn(n, 32 ** 3).astype(np.float32)
    t = _dev(sess, x)
    fc = len(ld) - 1
    shape = (32, 32, 32, 8)
    F = 32 ** 3 * 8
    W, b = pars['fc']
    out, bad = {}, []
    for route in ('no_fc_bits', 'default'):
        m = _make(sess, ld, in_shape, sk, pars, n, route, routes=ROUTES)
        r, k = _fc_launches(sess, lambda: _fisher(m, t, n))
        out[route] = r['p1'].cpu().numpy()
        if route == 'no_fc_bits':
            assert sess.lib.alq_model_engine_info(m._m, 1) == 0 and k == 3 and _try_copy(sess, m, 0, 5, n) is None
            act = _copy(sess, m, fc - 1, 0, n, (n,) + shape)
            z_dev = _copy(sess, m, fc, 0, n, (n, 2))
            m.param_grads_device(t, n, 0, cls=1)      # the general sweep keeps every activation: dec2's input (enc1 | up2)
            a_in = np.concatenate([_copy(sess, m, names.index('enc1'), 0, n, (n,) + shape), _copy(sess, m, names.index('up2'), 0, n, (n,) + shape)], axis=-1)
            pre, fragile = _pre64(a_in, pars['dec2'][0], pars['dec2'][1], shape[:-1])
            assert np.array_equal((act > 0)[~fragile], (pre > 0)[~fragile])
            z64, z32 = R.logits64(act, W, b, shape), R.logits_torch(act, W, b, shape, torch.float32)
            _figure(bad, 'NET-C 32^3 | no_fc_bits', 'logits', z_dev, z64, z32)
        else:
            assert sess.lib.alq_model_engine_info(m._m, 1) == 1 and k == 2 and sess.lib.alq_model_engine_info(m._m, 5) == 0
            part = _copy(sess, m, 0, 5, n, (n, 4))
            diff, diff32 = (z64[:, 0] - z64[:, 1])[:, None], (z32[:, 0] - z32[:, 1])[:, None]      # ref32: the same sums in fp32 torch
            got = (part.astype(np.float64).sum(axis=1) + float(b[0, 0]) - float(b[1, 0]))[:, None].astype(np.float32)
            _figure(bad, 'NET-C 32^3 | default', 'sum of the 4 partials + b0 - b1', got, diff, diff32)
            z = _copy(sess, m, fc, 0, n, (n, 2))
            _figure(bad, 'NET-C 32^3 | default', 'logit difference', z[:, :1], diff, diff32)
            assert not z[:, 1].any()
            sb = _sign_bytes(sess, m, fc, n, F)
            mask = _unpack(sb & 15, shape)
            print('NET-C 32^3: %d of %d units within DEFAULT_EPS x rms of zero, %d signs differ from the ALQ_NO_FC_BITS arm'
                  % (np.count_nonzero(fragile), fragile.size, np.count_nonzero(mask != (act > 0))))
            assert not (sb & 0xF0).any() and np.array_equal(mask[~fragile], (pre > 0)[~fragile])
        m.close()
    assert np.abs(out['default'] - out['no_fc_bits']).max() <= 2e-6
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 5. whole models
WHOLE = OrderedDict([
    ('hidden', (OrderedDict([('cv', ['conv', [4, [3, 3]], 'MA']), ('hid', ['fc', [8], 'MA']), ('fc', ['fc', [2]])]), (5, 6, 1), 2)),      # (the oracle flattens behind a conv)
    ('c5_on_conv12', (OrderedDict([('low', ['conv', [8, [3, 3, 3]], 'MA']), ('cv', ['conv', [12, [3, 3, 3]], 'MA']), ('fc', ['fc', [5]])]), (3, 5, 6, 1), 5)),
    ('bits_F1024', (R.bits_model(3), (4, 4, 8, 1), 2)),
])
_WHOLE = {}


def whole(name):
    if name not in _WHOLE:
        ld, in_shape, c = WHOLE[name]
        _WHOLE[name] = whole_record(name, ld, (), in_shape, 950 + list(WHOLE).index(name), None)
    return _WHOLE[name]


def _mkw(sess, d, route='default', **kw):
    return _make(sess, d['ld'], d['in_shape'], d['sk'], d['pars'], 4, route, routes=ROUTES, **kw)


@pytest.mark.parametrize('name', list(WHOLE))
def test_whole_model_param_grads_vs_fp64(sess, name):
    if WHOLE[name][2] != 2:      # check_param_grads' references are two-class: the same comparisons over every class
        return _check_param_grads_multiclass(sess, whole(name), WHOLE[name][2])
    check_param_grads(sess, whole(name), _mkw, ('default', 'no_fc_bits') if name == 'bits_F1024' else ('default',))


def _check_param_grads_multiclass(sess, d, c):
    """tests/test_gpu_convt.check_param_grads for a head of c classes: every W and b array of alq_param_grads against
    OracleModel(dtype=float64) under _bar - mode 0 for every class, mode 1 rows with labels over all classes - and the
    posteriors within 2e-6."""
    name, x = d['name'], d['x']
    lab = (np.arange(N) % c).astype(np.int32)
    onehot = np.eye(c)[lab].T
    refs = OrderedDict(('mode 0 class %d' % j, [[[np.asarray(a) for a in om.grad_log_post(j, x[[i]])] for i in range(N)] for om in (d['om64'], d['om32'])])
                       for j in range(c))
    refs['mode 1 rows'] = [[[np.asarray(a) / N for a in om.loss_and_grads(x[[i]], onehot[:, [i]])[1]] for i in range(N)] for om in (d['om64'], d['om32'])]
    p64 = d['om64'].forward(x)['posteriors']
    t = _dev(sess, x)
    m = _mkw(sess, d)
    got = {k: [] for k in refs}
    for a, e in _passes(N, 4):
        for j in range(c):
            g, post, _ = m.param_grads_device(t[a:e], e - a, 0, cls=j, want_post=True)
            got['mode 0 class %d' % j] += [m.unflatten(r) for r in g.cpu().numpy()]
            assert np.abs(post.cpu().numpy().astype(np.float64) - p64[:, a:e]).max() <= 2e-6
        g = m.param_grads_device(t[a:e], e - a, 1, labels=lab[a:e], loss_scale=1. / N)[0]
        got['mode 1 rows'] += [m.unflatten(r) for r in g.cpu().numpy()]
    m.close()
    bad = []
    for what, (r64, r32) in refs.items():
        for k, arr in enumerate(d['arrays']):
            _figure(bad, '%s | default | %s' % (name, what), arr, np.stack([r[k] for r in got[what]]), np.stack([r[k] for r in r64]).astype(np.float64),
                    np.stack([r[k] for r in r32]).astype(np.float32))
    assert not bad, bad


@pytest.mark.parametrize('name', [w for w in WHOLE if WHOLE[w][2] == 2])
def test_whole_model_other_entry_points_vs_fp64(sess, name):
    """alq_grad_sqnorms, alq_class_layer_sums, alq_diag_fisher, alq_hess_vecp (two-class bodies: the five-class model runs the
    parameter gradients only)."""
    check_other_entry_points(sess, whole(name), _mkw)


@pytest.mark.parametrize('name', [w for w in WHOLE if WHOLE[w][2] == 2])
def test_whole_model_fisher_pass_vs_fp64(sess, name):
    check_fisher_pass(sess, whole(name), _mkw, ROUTES)


@pytest.mark.parametrize('name', [w for w in WHOLE if WHOLE[w][2] == 2])
def test_device_weight_packing_same_bits(sess, name):
    check_packing(sess, whole(name), _mkw)
