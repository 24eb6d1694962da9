"""The kernels of the 1x1 conv head on their own (csrc/dense.hip: dense_head_fwd_kernel, dense_head_bwd_kernel,
dense_head_reduce_kernel through alq_dense_head_fwd / alq_dense_head_bwd; GPU box) against the fp64 statement of
tests/dense_head_ref.py (itself checked against triple loops by tests/test_dense_head_host.py).

  * Exact cases: integer inputs whose every product and partial sum stays below 2^24, so the fp32 chains, the fp64 folds and the
    rounding to float are exact: dX, dW, db and the prediction must equal the reference bit for bit; posteriors of exact logits
    within (4 + c) 2^-24 relative (tests.dense_head_ref.post_rel_bound).
  * Float cases: seeded randn inputs against running-error bounds computed per element (dense_head_ref.grad_bounds, logit_bound).
  * Every output of every call lies in the middle of a larger pattern-filled device tensor (_Framed): the margins must keep
    their bits, float payloads must hold no NaN.
  * Every case asserts from alq_dense_head_bwd_geometry - the launch's own arithmetic - that it is in the regime it names.

Nothing here is fitted to what the device returns: the bounds follow from the arithmetic, the inputs from their seeds."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dense_head_ref as ref  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -4
CIS = [4, 8, 12, 20, 28, 52, 60, 64]
CS = [2, 3, 4, 5, 6, 7, 8]
FWD_R = [1, 3, 4, 5, 1020, 1024, 1028, 1030, 4100]
FLOAT_CELLS = [(12, 5), (64, 8), (4, 2)]
GUARD = 64          # elements of margin on either side of an output (256 bytes of floats: 16-byte alignment is kept)
EXACT = 2 ** 24


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(sess, a):
    return a if isinstance(a, sess.torch.Tensor) else sess.to_device(a, sess.torch.float32)


class _Framed(object):
    """n elements `off` elements past an aligned address, in the middle of a pattern-filled device tensor."""

    def __init__(self, sess, n, dtype, off=0):
        torch = self.torch = sess.torch
        self.fill = {torch.float32: float('nan'), torch.int64: -7, torch.uint8: 0xA5}[dtype]
        self.buf = torch.full((n + 2 * GUARD + off,), self.fill, dtype=dtype, device=sess.device)
        self.lo, self.n, self.dtype = GUARD + off, n, dtype
        self.view = self.buf[self.lo:self.lo + n]
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.lo * self.buf.element_size())

    def _is_fill(self, t):
        torch = self.torch
        if self.dtype == torch.float32:          # by bits: another NaN is a write too
            pat = torch.full((1,), self.fill, dtype=torch.float32, device=t.device).view(torch.int32)
            return bool((t.view(torch.int32) == pat).all())
        return bool((t == self.fill).all())

    def margins_intact(self):
        return self._is_fill(self.buf[:self.lo]) and self._is_fill(self.buf[self.lo + self.n:])

    def untouched(self):
        return self._is_fill(self.buf)


def _geometry(sess, R, Ci):
    blocks, sweep, flush, per = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    assert sess.lib.alq_dense_head_bwd_geometry(R, Ci, C.byref(blocks), C.byref(per), C.byref(sweep), C.byref(flush)) == 0
    return dict(blocks=blocks.value, rows_per_block=per.value, rows_per_sweep=sweep.value, flush_rows=flush.value)


def _fwd(sess, x, W, b, post_off=0, pred_off=0, want_pred=True):
    """alq_dense_head_fwd into framed outputs: (post [c, R], pred [R] or None) as device tensors; the margins are asserted."""
    from nnal_amd._lib import check
    torch = sess.torch
    xd, Wd, bd = (_dev(sess, a) for a in (x, W, b))
    (R, Ci), c = xd.shape, Wd.shape[1]
    post = _Framed(sess, c * R, torch.float32, post_off)
    pred = _Framed(sess, R, torch.int64, pred_off) if want_pred else None
    sess.bind_stream()
    check(sess.lib.alq_dense_head_fwd(sess.ctx, P(xd), R, Ci, c, P(Wd), P(bd), post.ptr, pred.ptr if pred else None))
    assert post.margins_intact(), 'post: a store outside [c, R] (R=%d Ci=%d c=%d)' % (R, Ci, c)
    assert pred is None or pred.margins_intact(), 'pred: a store outside [R] (R=%d Ci=%d c=%d)' % (R, Ci, c)
    p = post.view.reshape(c, R)
    assert not bool(torch.isnan(p).any()), 'post: NaN or unwritten (R=%d Ci=%d c=%d)' % (R, Ci, c)
    return p, (pred.view if pred else None)


def _bwd(sess, x, delta, W, want_dx=True):
    """alq_dense_head_bwd into framed outputs, through a framed work buffer of exactly alq_dense_head_work_bytes: (dX [R, Ci] or
    None, [dW, db]) as device tensors; the margins are asserted."""
    from nnal_amd._lib import check
    torch = sess.torch
    xd, dd, Wd = (_dev(sess, a) for a in (x, delta, W))
    (R, Ci), c = xd.shape, Wd.shape[1]
    nbytes = int(sess.lib.alq_dense_head_work_bytes(Ci, c))
    assert nbytes == 2048 * (Ci * c + c) * 8
    work = _Framed(sess, nbytes, torch.uint8)
    g = _Framed(sess, Ci * c + c, torch.float32)
    dx = _Framed(sess, R * Ci, torch.float32) if want_dx else None
    sess.bind_stream()
    check(sess.lib.alq_dense_head_bwd(sess.ctx, P(dd), P(xd), R, Ci, c, P(Wd), dx.ptr if dx else None, work.ptr, g.ptr))
    tag = '(R=%d Ci=%d c=%d)' % (R, Ci, c)
    assert work.margins_intact(), 'work buffer: a store outside its %d bytes %s' % (nbytes, tag)
    assert g.margins_intact(), '[dW, db]: a store outside %s' % tag
    assert not bool(torch.isnan(g.view).any()), '[dW, db]: NaN or unwritten %s' % tag
    if dx is not None:
        assert dx.margins_intact(), 'dX: a store outside [R, Ci] %s' % tag
        assert not bool(torch.isnan(dx.view).any()), 'dX: NaN or unwritten %s' % tag
    return (dx.view.reshape(R, Ci) if dx else None), g.view


def _same(name, got, want):
    """Bit equality with the exact reference; a mismatch names the elements (integer inputs: readable)."""
    got = np.asarray(got.cpu().numpy() if hasattr(got, 'cpu') else got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError('%s: %d of %d elements differ; first at %s: device %s, reference %s' % (
            name, len(bad), got.size, [tuple(i) for i in bad[:6]], [got[tuple(i)] for i in bad[:6]], [want[tuple(i)] for i in bad[:6]]))


def _backward_rows(rpi):
    return [1, 2, rpi - 1, rpi, rpi + 1, 4 * rpi + 1, 8 * rpi, 8 * rpi + 1, 24 * rpi + 5]


# ------------------------------------------------------------------------------------------ exact: backward
@pytest.mark.parametrize('Ci', CIS)
def test_backward_exact_on_integers(sess, Ci):
    """x in [-4, 4], delta in [-3, 3], W in [-4, 4]: dX, dW and db equal the fp64 reference bit for bit, for every c in 2 .. 8 and
    R in 1, 2, rpi - 1, rpi, rpi + 1 (one sweep of the workgroup and its neighbours), 4 rpi + 1 (the second trip of lane 0 has
    its three later rows past the end), 8 rpi (one full workgroup), 8 rpi + 1 (two workgroups) and 24 rpi + 5 (four), with
    rpi = 256 / (Ci / 4) rows a sweep: 85, 51, 36, 19, 17 for Ci = 12, 20, 28, 52, 60 - lanes idle, the closing tree is ragged."""
    rpi = _geometry(sess, 1, Ci)['rows_per_sweep']
    assert rpi == 256 // (Ci // 4) and ((rpi & (rpi - 1)) != 0) == (Ci in (12, 20, 28, 52, 60))
    cells = 0
    for R in _backward_rows(rpi):
        geo = _geometry(sess, R, Ci)
        want_blocks = {8 * rpi + 1: 2, 24 * rpi + 5: 4}.get(R, 1)
        assert geo['blocks'] == want_blocks and geo['rows_per_block'] * geo['blocks'] >= R
        assert geo['rows_per_block'] <= geo['flush_rows'] * rpi          # one fold into fp64 per lane
        for c in CS:
            x, d, W = ref.backward_ints(R, Ci, c, 1000 * Ci + 10 * c + R % 7)
            want = ref.backward(x, d, W)
            assert max(np.abs(want[k]).max() for k in ('dX', 'dW', 'db')) < EXACT
            dX, g = _bwd(sess, x, d, W)
            tag = 'Ci=%d c=%d R=%d' % (Ci, c, R)
            _same('dX ' + tag, dX, want['dX'])
            _same('[dW, db] ' + tag, g, ref.flat_grad(want))
            cells += 1
    print('backward exact Ci=%d: rows_per_sweep %d, R in %s x c in 2..8 = %d cells, all bit-equal' % (Ci, rpi, _backward_rows(rpi), cells))


def _device_ints(sess, R, Ci, c, seed):
    torch = sess.torch
    gen = torch.Generator(device=sess.device).manual_seed(seed)
    x = torch.randint(-4, 5, (R, Ci), generator=gen, device=sess.device).float()
    d = torch.randint(-3, 4, (R, c), generator=gen, device=sess.device).float()
    W = torch.randint(-4, 5, (Ci, c), generator=gen, device=sess.device).float()
    return x, d, W


def _exact_large(sess, R, Ci, c, seed, twice):
    """Inputs drawn on the device, reference by torch fp64 matmuls on the device (exact for these integers)."""
    torch = sess.torch
    x, d, W = _device_ints(sess, R, Ci, c, seed)
    x64, d64, W64 = x.double(), d.double(), W.double()
    want_g = torch.cat([(x64.t() @ d64).reshape(-1), d64.sum(0)])
    want_dX = d64 @ W64.t()
    del x64
    biggest = max(float(want_g.abs().max()), float(want_dX.abs().max()))
    assert biggest < EXACT, biggest
    torch.cuda.synchronize()
    t0 = time.time()
    dX, g = _bwd(sess, x, d, W)
    torch.cuda.synchronize()
    dt = time.time() - t0
    if not torch.equal(g.double(), want_g):
        _same('[dW, db] Ci=%d c=%d R=%d' % (Ci, c, R), g, want_g.cpu().numpy())
    if not torch.equal(dX.double(), want_dX):
        rows = torch.nonzero((dX.double() != want_dX).any(1)).reshape(-1)
        raise AssertionError('dX Ci=%d c=%d R=%d: %d rows differ, first %s' % (Ci, c, R, rows.numel(), rows[:8].tolist()))
    del want_dX
    _, g0 = _bwd(sess, x, d, W, want_dx=False)
    assert torch.equal(g0, g), 'd_dx = NULL changes [dW, db]'
    if twice:
        dX2, g2 = _bwd(sess, x, d, W)
        assert torch.equal(dX2, dX) and torch.equal(g2, g), 'two identical calls differ'
    return biggest, dt


@pytest.mark.parametrize('c', [2, 7])
def test_backward_exact_beyond_the_capped_grid(sess, c):
    """Ci = 64, R = 3 * 262,144 + 5: the grid stops at 2048 workgroups and each owns 385 rows, more than the 8 sweeps (128 rows)
    of every uncapped launch; the last five workgroups own no row.  Also: two calls give the same bits, d_dx = NULL the same
    [dW, db], and no store leaves dX, the work buffer or [dW, db]."""
    R, Ci = 3 * 262144 + 5, 64
    geo = _geometry(sess, R, Ci)
    assert geo['blocks'] == 2048 and geo['rows_per_block'] > 8 * geo['rows_per_sweep']
    assert geo['rows_per_block'] <= geo['flush_rows'] * geo['rows_per_sweep']
    t0 = time.time()
    biggest, dt = _exact_large(sess, R, Ci, c, 11 + c, twice=True)
    print('capped grid Ci=64 c=%d R=%d: %s, largest |sum| %.0f < 2^24, bit-equal; call + checks %.3f s, test %.2f s'
          % (c, R, geo, biggest, dt, time.time() - t0))


def test_backward_exact_second_flush(sess):
    """Ci = 64, c = 3, R = 2048 * 16 * 68 + 3 = 2,228,227: a workgroup owns 1089 rows, more than flush_rows * rows_per_sweep =
    64 * 16 = 1024, so its lanes fold their fp32 sums into fp64 a second time (the outer loop of the kernel runs twice).  The
    path starts at R = 2,097,153; this R also leaves workgroups of different trip counts.  x is 0.57 GB."""
    R, Ci, c = 2048 * 16 * 68 + 3, 64, 3
    geo = _geometry(sess, R, Ci)
    assert geo['blocks'] == 2048 and geo['rows_per_block'] > 64 * 16
    assert geo['rows_per_block'] > geo['flush_rows'] * geo['rows_per_sweep']
    t0 = time.time()
    biggest, dt = _exact_large(sess, R, Ci, c, 5, twice=False)
    print('second flush Ci=64 c=3 R=%d: %s, largest |sum| %.0f < 2^24, bit-equal; call + checks %.3f s, test %.2f s'
          % (R, geo, biggest, dt, time.time() - t0))


# ------------------------------------------------------------------------------------------ exact: forward
def _check_forward(sess, x, W, b, tag, **kw):
    """pred equal on every voxel; posteriors within (4 + c) 2^-24 p64 wherever the voxel's logit spread is at most 80 (every
    p64 a normal float).  Returns (worst error / bound, the device's post, pred, the reference)."""
    want = ref.forward(x, W, b)
    assert np.array_equal(want['z'], np.round(want['z'])) and np.abs(want['z']).max() < EXACT          # exact logits
    post, pred = _fwd(sess, x, W, b, **kw)
    post = post.cpu().numpy()
    if pred is not None:
        _same('pred ' + tag, pred, want['pred'])
    firm = want['spread'] <= 80
    tol = ref.post_rel_bound(W.shape[1]) * want['post'][:, firm]
    ratio = np.abs(post.astype(np.float64)[:, firm] - want['post'][:, firm]) / tol
    assert post.min() >= 0 and post.max() <= 1
    return (ratio.max() if ratio.size else 0.), post, pred, want


@pytest.mark.parametrize('Ci', CIS)
def test_forward_exact_logits(sess, Ci):
    """Integer x, W, b (exact logits) for every c in 2 .. 8 and R in 1, 3, 4, 5, 1020, 1024, 1028, 1030, 4100: the 16-byte path
    (R % 4 == 0), the guarded path, under one workgroup and five.  Rows of x = 0 (logits b = [0, 1, 1, ...]: classes 1 and 2 tie)
    sit at both ends and in between.  The accuracy family keeps every voxel's logit spread at most 73 by construction
    (asserted at most 80); the wide family (W in [-4, 4]; R = 5, 1028, 4100) asserts pred everywhere and the posteriors of
    the voxels within that spread."""
    worst, cells = 0., 0
    for R in FWD_R:
        for c in CS:
            for wide in ((False, True) if R in (5, 1028, 4100) else (False,)):
                x, W, b = ref.forward_ints(R, Ci, c, 77 * Ci + 5 * c + R, wide)
                tag = 'Ci=%d c=%d R=%d wide=%d' % (Ci, c, R, wide)
                ratio, post, pred, want = _check_forward(sess, x, W, b, tag)
                assert wide or want['spread'].max() <= 80
                assert ratio <= 1., '%s: posterior error %.3f of its bound' % (tag, ratio)
                worst, cells = max(worst, ratio), cells + 1
    print('forward exact Ci=%d: %d cells (R in %s, c in 2..8), pred equal everywhere, worst posterior error / bound %.3f' % (Ci, cells, FWD_R, worst))


@pytest.mark.parametrize('Ci', [4, 12, 64])
def test_forward_first_maximum_on_ties(sess, Ci):
    """Logits made exactly equal through the weights: classes j and j + 1 tie above the rest for every j (prediction j), all
    classes equal (0), the last class alone (c - 1), and z = b; at R = 24 (16-byte path) and R = 23 (guarded path).  Tied
    classes get the same posterior bits."""
    for c in CS:
        for j in range(c - 1):
            for R in (24, 23):
                x, W, b, want = ref.tie_case(Ci, c, j, R)
                post, pred = _fwd(sess, x, W, b)
                _same('pred Ci=%d c=%d j=%d R=%d' % (Ci, c, j, R), pred, want)
                post = post.cpu().numpy()
                assert np.array_equal(post[j, 1::4], post[j + 1, 1::4])
                assert (post[:, 2::4] == post[0, 2::4]).all() and np.abs(post[:, 2::4] - 1. / c).max() <= ref.post_rel_bound(c) / c
    print('ties Ci=%d: c in 2..8, every pair (j, j + 1), all equal, R = 24 and 23: first maximum everywhere' % Ci)


@pytest.mark.parametrize('Ci', [4, 20, 64])
def test_forward_saturation(sess, Ci):
    """One class at least 200 above the others (the reference's spread is asserted): its posterior is exactly 1, the others
    exactly 0, no NaN, the right prediction; every class in turn, both store paths."""
    for c in CS:
        for top in range(c):
            for R in (16, 13):
                rs = np.random.RandomState(Ci + 10 * c + top)
                W = rs.randint(-4, 5, size=(Ci, c)).astype(np.float32)
                b = rs.randint(-3, 4, size=c).astype(np.float32)
                W[0, top] = 4096          # the top logit >= 4096 - 3 - 63 * 16, the others <= 3 + 64 * 16: 2058 apart at least
                x = rs.randint(-4, 5, size=(R, Ci)).astype(np.float32)
                x[:, 0] = 1 + np.arange(R) % 4
                want = ref.forward(x, W, b)
                gap = want['z'][:, top] - np.delete(want['z'], top, axis=1).max(1)
                assert gap.min() >= 200 and want['spread'].min() >= 200
                post, pred = _fwd(sess, x, W, b)
                _same('pred', pred, np.full(R, top))
                _same('post', post, (np.arange(c)[:, None] == top) * np.ones((1, R)))


def test_forward_buffer_variants(sess):
    """R = 1024 (R % 4 == 0): a post buffer one float off 16-byte alignment, a pred buffer one int64 off, and pred = NULL give
    the bits of the aligned call - the first two through the guarded path, the last on the 16-byte path.  At a
    non-power-of-two Ci and at Ci = 64; a second identical call gives the same bits."""
    torch = sess.torch
    for Ci, c in ((12, 5), (64, 8), (4, 2)):
        x, W, b = ref.forward_ints(1024, Ci, c, 3)
        xd = sess.to_device(x, torch.float32)
        post, pred = _fwd(sess, xd, W, b)
        assert post.data_ptr() % 16 == 0 and pred.data_ptr() % 16 == 0
        for kw in (dict(post_off=1), dict(pred_off=1), dict(want_pred=False), dict(post_off=3, pred_off=1), {}):
            p2, q2 = _fwd(sess, xd, W, b, **kw)
            assert (p2.data_ptr() % 16 != 0) == ('post_off' in kw) and (q2 is None or (q2.data_ptr() % 16 != 0) == ('pred_off' in kw))
            assert torch.equal(p2, post) and (q2 is None or torch.equal(q2, pred)), (Ci, c, kw)


# ------------------------------------------------------------------------------------------ float cases
@pytest.mark.parametrize('Ci,c', FLOAT_CELLS)
def test_float_inputs_within_running_error_bounds(sess, Ci, c):
    """Full-mantissa randn inputs (a 16-bit conversion anywhere would show) at R = 5000 and R = 24 rpi + 5: dW and db within
    65 * 2^-24 sum_r |x_r||delta_r| + 2^-24 |ref|, dX within (c + 1) 2^-24 sum_j |delta_j||W_j|, posteriors within
    p64 (2 max_j |dz_j| + (4 + c) 2^-24) with dz the bound on the fp32 logits, (Ci + 1) 2^-24 (|b| + sum |x||W|)."""
    rpi = _geometry(sess, 1, Ci)['rows_per_sweep']
    for R in (5000, 24 * rpi + 5):
        geo = _geometry(sess, R, Ci)
        assert geo['blocks'] >= 2 and geo['rows_per_block'] <= geo['flush_rows'] * rpi
        rs = np.random.RandomState(Ci * c + R)
        x, d = rs.randn(R, Ci).astype(np.float32), (rs.randn(R, c) / R).astype(np.float32)
        W, b = (0.5 * rs.randn(Ci, c)).astype(np.float32), (0.05 * rs.randn(c)).astype(np.float32)
        bw = ref.backward(x, d, W)
        bound = ref.grad_bounds(x, d, W, bw)
        dX, g = _bwd(sess, x, d, W)
        r_dx = (np.abs(dX.cpu().numpy().astype(np.float64) - bw['dX']) / bound['dX']).max()
        r_g = (np.abs(g.cpu().numpy().astype(np.float64) - ref.flat_grad(bw)) / bound['g']).max()
        fw = ref.forward(x, W, b)
        assert fw['spread'].max() <= 80
        dz = ref.logit_bound(x, W, b).max(1)
        tol = fw['post'] * (2 * dz + ref.post_rel_bound(c))[None, :]
        post, pred = _fwd(sess, x, W, b)
        r_p = (np.abs(post.cpu().numpy().astype(np.float64) - fw['post']) / tol).max()
        top2 = np.sort(fw['z'], axis=1)
        firm = top2[:, -1] - top2[:, -2] > 2 * dz
        print('float Ci=%d c=%d R=%d %s: error / bound dX %.3f, [dW, db] %.3f, posteriors %.3f; %d of %d predictions firm'
              % (Ci, c, R, geo, r_dx, r_g, r_p, firm.sum(), R))
        assert r_dx <= 1. and r_g <= 1. and r_p <= 1.
        assert np.array_equal(pred.cpu().numpy()[firm], fw['pred'][firm])


@pytest.mark.parametrize('Ci,c', FLOAT_CELLS)
def test_logits_through_a_model(sess, Ci, c):
    """The logits the forward kernel stores when the last layer is the requested feature layer (alq_forward ->
    dense_forward_head(..., want_logits)): conv(Ci, 3x3, ReLU) + head, the head's input read back through a second model whose
    feature layer is the conv (same weights, same bits), within (Ci + 1) 2^-24 (|b| + sum |x||W|) of fp64.  10x10 with N = 50:
    5000 voxels on the 16-byte path; 5x7 with N = 3: 105 voxels on the guarded path."""
    from nnal_amd import device, netspec
    from tests.test_gpu_dense import _head_net
    torch = sess.torch
    for in_shape, N in (((10, 10, 1), 50), ((5, 7, 1), 3)):
        ld, sk = _head_net(Ci, c, 2)
        pars = netspec.he_init(ld, in_shape, seed=40 + Ci + c, skips=sk, bias_std=0.05)
        xin = np.random.RandomState(Ci + c).randn(N, *in_shape).astype(np.float32)
        t = sess.to_device(xin.reshape(N, -1), torch.float32)
        feats = []
        for layer in (0, 1):
            m = device.DeviceModel(sess, ld, in_shape, sk, feature_layer=layer, max_batch=64)
            m.set_weights(pars)
            post, pred, feat = m.forward_device(t, N, want_pred=True, want_feat=True)
            feats.append((feat.cpu().numpy(), post.cpu().numpy(), pred.cpu().numpy()))
            m.close()
        R = N * in_shape[0] * in_shape[1]
        x, z = feats[0][0].reshape(R, Ci), feats[1][0].reshape(R, c)
        assert feats[0][1].tobytes() == feats[1][1].tobytes() and (x >= 0).all() and (x > 0).mean() > 0.1
        W, b = pars['last'][0].reshape(Ci, c), pars['last'][1]
        fw = ref.forward(x, W, b)
        bound = ref.logit_bound(x, W, b)
        r_z = (np.abs(z.astype(np.float64) - fw['z']) / bound).max()
        tol = fw['post'] * (2 * bound.max(1) + ref.post_rel_bound(c))[None, :]
        r_p = (np.abs(feats[1][1].astype(np.float64) - fw['post']) / tol).max()
        print('logits Ci=%d c=%d R=%d: error / bound logits %.3f, posteriors %.3f' % (Ci, c, R, r_z, r_p))
        assert r_z <= 1. and r_p <= 1.
        # the stored logits and the stored prediction agree: the first maximum of the device's own logits
        assert np.array_equal(feats[1][2], ref.first_argmax(z))


# ------------------------------------------------------------------------------------------ stores, identity
def test_stores_stay_inside_their_buffers(sess):
    """Every call of this file goes through _Framed outputs; here one small and one large shape per kernel, named: backward
    at R = 341 (Ci = 12) and beyond the capped grid (Ci = 64, R = 786,437; work buffer of exactly alq_dense_head_work_bytes),
    forward at R = 341 and at 786,436 / 786,437 voxels (3073 workgroups, both store paths)."""
    torch = sess.torch
    lib = sess.lib
    for Ci in CIS:
        for c in CS:
            assert lib.alq_dense_head_work_bytes(Ci, c) == 2048 * (Ci * c + c) * 8
    assert lib.alq_dense_head_work_bytes(0, 2) == 0 and lib.alq_dense_head_work_bytes(8, 0) == 0 and lib.alq_dense_head_work_bytes(-8, -2) == 0
    f = _Framed(sess, 10, torch.float32, 1)
    assert f.margins_intact() and f.untouched()
    f.buf[f.lo - 1] = 0.
    assert not f.margins_intact()          # the check sees a single store
    x, d, W = ref.backward_ints(341, 12, 5, 0)
    _bwd(sess, x, d, W)
    _fwd(sess, x, W, ref.tie_bias(5))
    R = 3 * 262144 + 5
    assert _geometry(sess, R, 64)['blocks'] == 2048
    x, d, W = _device_ints(sess, R, 64, 7, 1)
    b = sess.to_device(ref.tie_bias(7), torch.float32)
    _bwd(sess, x, d, W)
    p1, q1 = _fwd(sess, x, W, b)
    p0, q0 = _fwd(sess, x[:R - 1], W, b)
    assert torch.equal(p0, p1[:, :R - 1]) and torch.equal(q0, q1[:R - 1])          # the two store paths: the same bits
    print('stores: margins of %d elements intact around post, pred, dX, [dW, db] and the work buffer at R = 341 (Ci = 12, %s) and R = %d '
          '(Ci = 64, %s)' % (GUARD, _geometry(sess, 341, 12), R, _geometry(sess, R, 64)))


@pytest.mark.parametrize('Ci,c,R', [(12, 5, 5000), (52, 7, 24 * 19 + 5), (20, 3, 1)])
def test_identical_calls_and_optional_outputs(sess, Ci, c, R):
    """Two identical calls: the same bits of post, pred, dX and [dW, db] (no atomics); d_dx = NULL: the same [dW, db];
    pred = NULL: the same post.  At non-power-of-two head widths (the capped-grid shape: test_backward_exact_beyond_the_capped_grid)."""
    torch = sess.torch
    rs = np.random.RandomState(R + Ci)
    x, d, W, b = (sess.to_device(rs.randn(*s).astype(np.float32), torch.float32) for s in ((R, Ci), (R, c), (Ci, c), (c,)))
    dX, g = _bwd(sess, x, d, W)
    dX2, g2 = _bwd(sess, x, d, W)
    _, g3 = _bwd(sess, x, d, W, want_dx=False)
    assert torch.equal(dX, dX2) and torch.equal(g, g2) and torch.equal(g, g3)
    post, pred = _fwd(sess, x, W, b)
    post2, pred2 = _fwd(sess, x, W, b)
    post3, none = _fwd(sess, x, W, b, want_pred=False)
    assert torch.equal(post, post2) and torch.equal(pred, pred2) and torch.equal(post, post3) and none is None
    print('identical calls Ci=%d c=%d R=%d %s: the same bits' % (Ci, c, R, _geometry(sess, R, Ci)))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(sess):
    """Every refusal returns its status before a launch (dense_check and the null / alignment checks of k_dense_head_* precede
    hipLaunchKernelGGL): the pre-filled outputs keep their bits, alq_last_error names the entry point."""
    torch, lib = sess.torch, sess.lib
    R, Ci, c = 40, 8, 3
    x, d, W = (sess.to_device(a, torch.float32) for a in ref.backward_ints(R + 1, Ci, c, 0))
    b = sess.to_device(ref.tie_bias(c), torch.float32)
    post, pred = _Framed(sess, c * R, torch.float32), _Framed(sess, R, torch.int64)
    dx, g = _Framed(sess, (R + 1) * Ci, torch.float32), _Framed(sess, Ci * c + c, torch.float32)
    work = _Framed(sess, int(lib.alq_dense_head_work_bytes(64, 8)), torch.uint8)
    sess.bind_stream()
    fwd = (sess.ctx, P(x), R, Ci, c, P(W), P(b), post.ptr, pred.ptr)
    bwd = (sess.ctx, P(d), P(x), R, Ci, c, P(W), dx.ptr, work.ptr, g.ptr)

    def put(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    off4 = lambda p: C.c_void_p(p.value + 4)          # noqa: E731
    for name, fn, ok, i_x, i_R, i_Ci, i_c, nulls in (('dense_head_fwd', lib.alq_dense_head_fwd, fwd, 1, 2, 3, 4, (0, 1, 5, 6, 7)),
                                                     ('dense_head_bwd', lib.alq_dense_head_bwd, bwd, 2, 3, 4, 5, (0, 1, 2, 6, 8, 9))):
        cases = [(put(ok, i_Ci, v), EUNSUPPORTED) for v in (0, 2, 6, 68)] + [(put(ok, i_c, v), EUNSUPPORTED) for v in (1, 9)]
        cases += [(put(ok, i_R, 0), EINVAL), (put(ok, i_R, -3), EINVAL)]
        # R * max(Ci, c) >= 2^31 on the small buffers: refused by the sizes alone
        cases += [(put(put(ok, i_R, 2 ** 31 // 64), i_Ci, 64), EUNSUPPORTED), (put(put(put(ok, i_R, 2 ** 28), i_Ci, 4), i_c, 8), EUNSUPPORTED),
                  (put(ok, i_R, 2 ** 40), EUNSUPPORTED)]
        cases += [(put(ok, i_x, off4(P(x))), EINVAL)] + [(put(ok, i, None), EINVAL) for i in nulls]
        if name == 'dense_head_bwd':
            cases.append((put(ok, 7, off4(dx.ptr)), EINVAL))
        for args, status in cases:
            assert fn(*args) == status, (name, args, status)
            assert name.encode() in lib.alq_last_error(), lib.alq_last_error()
    torch.cuda.synchronize()
    for f in (post, pred, dx, g, work):
        assert f.untouched()
    # the calls these were derived from are accepted
    assert lib.alq_dense_head_fwd(*fwd) == 0 and lib.alq_dense_head_bwd(*bwd) == 0
    assert lib.alq_dense_head_fwd(*put(fwd, 8, None)) == 0 and lib.alq_dense_head_bwd(*put(bwd, 7, None)) == 0
    torch.cuda.synchronize()
    assert all(f.margins_intact() for f in (post, pred, dx, g, work)) and not post.untouched() and not g.untouched()
