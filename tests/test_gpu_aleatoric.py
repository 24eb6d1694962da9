"""The aleatoric-uncertainty head (AU_4U) on the device (GPU box): dense_head_fwd_au_kernel against alq_dense_head_fwd and the fp64
statement of tests/aleatoric_ref.py, mt_cotangent_au_kernel against nnal_amd.mteach.evaluate_au and alq_mt_cotangent, whole nets
against the fp64 torch graph of tests/dense_ref.py, sess.run of AU_vals / output, one optimiser step and the refusals.

Bars: rows 4 * 2^-24 * (|labelled term| + |consistency term|), the log-variance column against au_scale (kappa / 2 + div e) - one
fp32 rounding of a sum formed in fp64, the factor of tests.test_gpu_mteach._kernel_case; statistics 1e-12 relative; the raw
channel of the head within tests.dense_head_ref.logit_bound; whole nets as tests/test_gpu_mteach.py (loss 1e-6 relative,
gradients through tests.test_gpu_train._close); `output` within 4 times the fp32 torch graph's own error to fp64."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import aleatoric_ref, dense_head_ref, dense_ref  # noqa: E402
from tests.test_gpu_losses import _objective  # noqa: E402
from tests.test_gpu_mteach import CW, EINVAL, EUNSUPPORTED, P, _dense_model, _mt_call, _posteriors  # noqa: E402
from tests.test_gpu_train import _close  # noqa: E402

GUARD = 64          # floats of NaN on either side of an output
SHAPES = {'R140': (140, 0), 'R105': (105, 0), 'R1': (1, 0), 'R140_unaligned': (140, 1)}
KAPPA = 0.1


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


class _Framed(object):
    """n elements `off` elements past an aligned address, between two margins of a fill value that must keep their bits."""

    def __init__(self, sess, n, dtype, off=0):
        torch = self.torch = sess.torch
        self.int = dtype == torch.int64
        self.buf = torch.full((n + 2 * GUARD + off,), -7 if self.int else float('nan'), dtype=dtype, device=sess.device)
        self.lo, self.n = GUARD + off, n
        self.view = self.buf[self.lo:self.lo + n]
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.lo * self.buf.element_size())

    def _fill(self, t):
        return bool((t == -7).all()) if self.int else bool((t.view(self.torch.int32) == 0x7FC00000).all())

    def margins_intact(self):
        return self._fill(self.buf[:self.lo]) and self._fill(self.buf[self.lo + self.n:])

    def untouched(self):
        return self._fill(self.buf)


# ------------------------------------------------------------------------------------------ the head's forward kernel
def _head_au(sess, x, W, b, off):
    """alq_dense_head_fwd_au into framed outputs `off` elements past an aligned address: post [c, R], pred, au [R], logits [R, c + 1]."""
    from nnal_amd._lib import check
    torch = sess.torch
    xd, Wd, bd = (sess.to_device(a, torch.float32) for a in (x, W, b))
    (R, Ci), c = x.shape, W.shape[1] - 1
    post, pred = _Framed(sess, c * R, torch.float32, off), _Framed(sess, R, torch.int64, off)
    au, z = _Framed(sess, R, torch.float32, off), _Framed(sess, R * (c + 1), torch.float32, off)
    sess.bind_stream()
    check(sess.lib.alq_dense_head_fwd_au(sess.ctx, P(xd), R, Ci, c, P(Wd), P(bd), post.ptr, pred.ptr, au.ptr, z.ptr))
    for f in (post, pred, au, z):
        assert f.margins_intact(), 'a store outside an output (R=%d Ci=%d c=%d off=%d)' % (R, Ci, c, off)
    outs = [f.view.cpu().numpy() for f in (post, pred, au, z)]
    assert not any(np.isnan(o).any() for o in (outs[0], outs[2], outs[3]))
    return outs[0].reshape(c, R), outs[1], outs[2], outs[3].reshape(R, c + 1)


def _head_plain(sess, x, W, b, off):
    from nnal_amd._lib import check
    torch = sess.torch
    xd, Wd, bd = (sess.to_device(np.ascontiguousarray(a), torch.float32) for a in (x, W, b))
    (R, Ci), c = x.shape, W.shape[1]
    post, pred = _Framed(sess, c * R, torch.float32, off), _Framed(sess, R, torch.int64, off)
    sess.bind_stream()
    check(sess.lib.alq_dense_head_fwd(sess.ctx, P(xd), R, Ci, c, P(Wd), P(bd), post.ptr, pred.ptr))
    return post.view.cpu().numpy().reshape(c, R), pred.view.cpu().numpy()


@pytest.mark.parametrize('c', [2, 3, 7])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_head_forward_kernel(sess, shape, c):
    """140 voxels: the 16-byte path; 105 and 1: R % 4 != 0, the guarded path; 140 with every output one element into its buffer:
    unaligned bases, the guarded path again.  Ci 4, 12, 64: one, three and sixteen 16-byte pieces a voxel."""
    R, off = SHAPES[shape]
    for Ci in (4, 12, 64):
        # float case: the classes carry the bits of alq_dense_head_fwd on the sliced weights, au is the ReLU of the raw channel
        rs = np.random.RandomState(1000 * c + Ci + R)
        x = rs.randn(R, Ci).astype(np.float32)
        W, b = (rs.randn(Ci, c + 1) * 0.5).astype(np.float32), rs.randn(c + 1).astype(np.float32)
        post, pred, au, z = _head_au(sess, x, W, b, off)
        post0, pred0 = _head_plain(sess, x, W[:, :c], b[:c], off)
        assert post.tobytes() == post0.tobytes() and pred.tobytes() == pred0.tobytes(), (shape, Ci, c)
        assert np.array_equal(au, np.maximum(z[:, c], np.float32(0.)))
        ref = aleatoric_ref.forward_au(x, W, b)
        err, bound = np.abs(z - ref['z']), dense_head_ref.logit_bound(x, W, b)
        print('%s Ci=%d c=%d: worst logit error / running-error bound %.3f' % (shape, Ci, c, (err / bound).max()))
        assert (err <= bound).all()
        # integer case: exact logits; the raw channel holds negatives, exact zeros (the rows of x = 0: its bias is 0) and positives
        xi, Wi, bi = dense_head_ref.forward_ints(R, Ci, c + 1, seed=Ci + c)
        bi[c] = 0
        refi = aleatoric_ref.forward_au(xi, Wi, bi)
        raw = refi['z'][:, c]
        assert (raw == 0).any() and (R == 1 or ((raw < 0).any() and (raw > 0).any()))
        post, pred, au, z = _head_au(sess, xi, Wi, bi, off)
        assert np.array_equal(z.astype(np.float64), refi['z']) and np.array_equal(au.astype(np.float64), refi['au'])
        assert not au[raw <= 0].any() and np.array_equal(pred, refi['pred'])
        post0, pred0 = _head_plain(sess, xi, Wi[:, :c], bi[:c], off)
        assert post.tobytes() == post0.tobytes() and pred.tobytes() == pred0.tobytes()


# ------------------------------------------------------------------------------------------ the cotangent kernel
def _au_plane(rs, R):
    """max(randn, 0) * 2 - about half exact zeros - with 80, 800 (exp(-a) underflows towards and to zero) and 0 planted."""
    au = (np.maximum(rs.randn(R), 0.) * 2.).astype(np.float32)
    for i, v in zip(rs.permutation(R)[:3], (80., 800., 0.)):
        au[i] = v
    return au


def _au_call(sess, p, q, au, lab, measure, s, k, kau, kappa, cw=None, sw=None, gamma=None, off=0, rows=True):
    """alq_mt_cotangent_au (or alq_mt_stats_au) on host arrays; `off`: the planes, au and the rows start that many floats into
    their buffers."""
    from nnal_amd._lib import LossT, check
    torch = sess.torch
    c, R = p.shape

    def up(a, dt=torch.float32):
        buf = sess.empty((a.size + off,), dt)
        buf[off:] = sess.to_device(a.reshape(-1), dt)
        return buf
    pd, qd, ad, ld = up(p), up(q), up(au), sess.to_device(lab.astype(np.int32), torch.int32)
    cwd = sess.to_device(np.asarray(cw, np.float32), torch.float32) if cw is not None else None
    swd = sess.to_device(sw.astype(np.float32), torch.float32) if sw is not None else None
    L = LossT(0, -1. if gamma is None else gamma, 0.7, 1., cwd.data_ptr() if cwd is not None else None,
              swd.data_ptr() if swd is not None else None, None, None)
    out = _Framed(sess, R * (c + 1), torch.float32, off)
    st = torch.full((3,), float('nan'), dtype=torch.float64, device=sess.device)
    sess.bind_stream()
    if rows:
        check(sess.lib.alq_mt_cotangent_au(sess.ctx, P(pd, 4 * off), P(qd, 4 * off), P(ad, 4 * off), c, R, P(ld), C.byref(L), float(s), float(k),
                                           float(kau), float(kappa), measure, out.ptr, P(st)))
        assert out.margins_intact()
    else:
        check(sess.lib.alq_mt_stats_au(sess.ctx, P(pd, 4 * off), P(qd, 4 * off), P(ad, 4 * off), c, R, P(ld), C.byref(L), float(kappa), measure,
                                       P(st)))
        assert out.untouched()
    return out.view.cpu().numpy().reshape(R, c + 1), st.cpu().numpy()


def _au_case(sess, R, c, measure, weighted, off=0, seed=0):
    from nnal_amd import mteach
    rs = np.random.RandomState(seed + 7 * c + R % 1000)
    p, q = _posteriors(rs, c, R), _posteriors(rs, c, R)
    au = _au_plane(rs, R) if R >= 3 else np.asarray([1.5] * R, np.float32)
    lab = rs.randint(0, c, size=R)
    cw = sw = gamma = None
    if weighted:
        lab[rs.rand(R) < 0.3] = -1
        sw = (0.25 + rs.rand(R)).astype(np.float32)
        sw[rs.rand(R) < 0.05] = 0
        if c == 2:
            cw, gamma = np.asarray(CW, np.float32), 2.
    s, k, kau = np.float32(3. / max(R, 1)), np.float32(0.8 * 2. / (c * 35)), np.float32(0.8 / 35)
    args = (p, q, au, lab, measure, s, k, kau, np.float32(KAPPA), cw, sw, gamma, off)
    rows, st = _au_call(sess, *args)
    rows2, st2 = _au_call(sess, *args)
    assert rows.tobytes() == rows2.tobytes() and st.tobytes() == st2.tobytes()          # no atomics: the same bits
    ref = mteach.evaluate_au(p, q, au, lab, measure, float(s), float(k), float(kau), KAPPA, cw, sw, gamma)
    mag = np.abs(ref['labelled_rows']) + np.abs(ref['cons_rows'])
    mag[:, c] = float(kau) * (0.5 * float(np.float32(KAPPA)) + ref['div'] * np.exp(-au.astype(np.float64)))
    tol = 4 * 2. ** -24 * mag
    err = np.abs(rows.astype(np.float64) - ref['rows'])
    print('R=%d c=%d measure=%d weighted=%d off=%d: worst row error / bound %.3f, stats %s' % (R, c, measure, weighted, off,
          (err / np.maximum(tol, 1e-300)).max(), st))
    assert not np.isnan(rows).any() and (err <= tol).all()
    assert not rows[au == 0, c].any()          # ReluGrad at x <= 0: exactly 0
    assert R < 3 or (rows[au > 0, c] != 0).any()
    for a, b in zip(st, ref['stats']):
        assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300) or a == b
    _, st3 = _au_call(sess, *args, rows=False)
    assert st3.tobytes() == st.tobytes()
    if measure == mteach.CE:          # TF does not differentiate the labels: no consistency term below column c, one in column c
        rows0 = _au_call(sess, p, q, au, lab, measure, s, np.float32(0.), kau, np.float32(KAPPA), cw, sw, gamma, off)[0]
        assert np.array_equal(rows, rows0) and (R < 3 or rows[:, c].any())


@pytest.mark.parametrize('measure', [0, 1])
@pytest.mark.parametrize('c', [2, 3, 7])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_cotangent_kernel_vs_fp64_statement(sess, shape, c, measure):
    R, off = SHAPES[shape]
    for weighted in (False, True):
        _au_case(sess, R, c, measure, weighted, off)


@pytest.mark.parametrize('measure', [0, 1])
@pytest.mark.parametrize('c', [2, 3, 7])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_zero_variance_writes_the_bits_of_the_mean_teacher_kernel(sess, shape, c, measure):
    R, off = SHAPES[shape]
    rs = np.random.RandomState(11 * c + R)
    p, q = _posteriors(rs, c, R), _posteriors(rs, c, R)
    lab = rs.randint(-1, c, size=R)
    sw = (0.25 + rs.rand(R)).astype(np.float32)
    s, k = np.float32(3. / R), np.float32(0.8 * 2. / (c * 35))
    rows, st = _au_call(sess, p, q, np.zeros(R, np.float32), lab, measure, s, k, np.float32(0.7), np.float32(0.), sw=sw, off=off)
    rows0, st0 = _mt_call(sess, p, q, lab, measure, s, k, sw=sw, off=off)
    assert rows[:, :c].tobytes() == rows0.tobytes() and not rows[:, c].any()
    assert st[:2].tobytes() == st0[:2].tobytes() and (st[2] == st0[2] or abs(st[2] - st0[2]) <= 1e-12 * abs(st0[2]))


@pytest.mark.parametrize('measure', [0, 1])
def test_cotangent_kernel_beyond_one_trip_of_the_grid(sess, measure):
    """Four voxels more than one sweep of the capped grid covers (the kernel's exported figure): one lane grid-strides."""
    R = int(sess.lib.alq_mt_au_trip_voxels()) + 4
    assert R % 4 == 0 and R < 2 ** 22
    _au_case(sess, R, 2, measure, True)


# ------------------------------------------------------------------------------------------ whole nets
# net -> (netspec function, classes, input shape, N, max_batch, weight seed, input seed).  The seeds were searched on the CPU, from 44
# / 53 and 1000 up: the first weights with a quarter of the raw log-variances on either side of 0, then the first inputs whose fp64
# graph - plain and under the dropout of the test - keeps every raw log-variance 1e-3 away from 0 (asserted below, from that graph)
NETS = {'2d': ('net_c_2d_dense', 2, (16, 16, 1), 4, 3, 47, 1001), '3d': ('net_c_dense', 2, (8, 8, 8, 1), 2, 8, 53, 1005)}
DROP = dict(layers=[0], keep_prob=0.5, seed=20251, first_sample=0)


def _au_reference(g, gt, hy, x, px, ycols, vw, measure, coeff, N, c, kappa):
    """(value, what the optimiser differentiates, raw log-variances) of loss = L + coeff * cons read as the vector [N]: the
    labelled loss on the c clean logits, cons_v = div_v exp(-a_v) + kappa a_v / 2, the teacher's clean posteriors constants."""
    import torch
    z = g._graph(g._as_input(x))['output']
    L, _ = _objective(hy, z[:c], ycols, vw)
    with torch.no_grad():
        zt = gt._graph(gt._as_input(px))['output'][:c]
    p, a = torch.softmax(z[:c], 0), torch.relu(z[c])
    if measure == 'L2':
        div = ((p - torch.softmax(zt, 0)) ** 2).mean(0)
    else:
        div = -(p.detach() * torch.log_softmax(zt, 0)).sum(0)          # TF: no gradient into the labels
    cons = (div * torch.exp(-a) + 0.5 * kappa * a).reshape(N, -1).mean(1)
    return L + coeff * cons.mean(), N * L + coeff * cons.sum(), z[c].detach().numpy()


def _raw_is_clear(raw):
    return np.abs(raw).min() > 1e-3 and (raw > 0).mean() >= 0.1 and (raw < 0).mean() >= 0.1


def _net_inputs(net):
    """The model's weights, the teacher's, and their inputs; the fp64 graph alone - plain and under the dropout of the test - must
    satisfy _raw_is_clear.  CPU only."""
    import torch
    from nnal_amd import netspec, ref64
    fn, c, in_shape, N, mb, wseed, xseed = NETS[net]
    ld, sk = getattr(netspec, fn)(c + 1)
    pars = netspec.he_init(ld, in_shape, seed=wseed, skips=sk, bias_std=0.05)
    tpars = netspec.he_init(ld, in_shape, seed=wseed + 1, skips=sk, bias_std=0.05)
    g64 = dense_ref.DenseGraph(ld, in_shape, pars, sk, torch.float64)
    t64 = dense_ref.DenseGraph(ld, in_shape, tpars, sk, torch.float64)
    x, _ = dense_ref.select_inputs(g64, in_shape, N, xseed, ref64.DEFAULT_EPS)
    for drop in (None, DROP):
        g64.drop = drop
        with torch.no_grad():
            raw = g64._graph(g64._as_input(x))['output'][c].numpy()
        g64.drop = None
        assert _raw_is_clear(raw), (net, drop, np.abs(raw).min(), (raw > 0).mean())
    px, _ = dense_ref.select_inputs(t64, in_shape, N, xseed + 5000, ref64.DEFAULT_EPS)
    return ld, sk, pars, tpars, x, px, xseed


@pytest.mark.parametrize('measure', ['L2', 'CE'])
@pytest.mark.parametrize('net', sorted(NETS))
def test_whole_nets_vs_fp64(sess, net, measure):
    """Student and a teacher of different weights through tests/dense_ref.DenseGraph; the 2-D net at max_batch 3: two cuts."""
    import torch
    from nnal_amd import NN_extended, mteach
    fn, c, in_shape, N, mb, wseed, _ = NETS[net]
    ld, sk, pars, tpars, x, px, xseed = _net_inputs(net)
    max_coeff, ramp = 150., 1.          # cons_coeff = 150 exp(-5) = 1.01 at step 0
    m = NN_extended.CNN(in_shape, ld, 'au ' + net, list(sk), dropout=[[0], 0.5], sess=sess, max_batch=mb, MT_SSL=True, AU_4U=True,
                        AU_log_rel_coeff=KAPPA, output_perturbation_measure=measure, max_cons_coeff=max_coeff, rampup_length=ramp,
                        learning_rate=0.01)
    m.set_weights(pars)
    assert m.AU_4U and not m.AU_4L and m.class_num == c == m.nclass and m.num_params == sum(W.size + b.size for W, b in pars.values())
    m.get_optimizer()
    m.teacher.set_weights(tpars)
    assert m.teacher.AU_4U and m.teacher.nclass == c
    coeff = mteach.cons_coeff(0, ramp, max_coeff)
    g64, g32 = (dense_ref.DenseGraph(ld, in_shape, pars, sk, dt) for dt in (torch.float64, torch.float32))
    t64, t32 = (dense_ref.DenseGraph(ld, in_shape, tpars, sk, dt) for dt in (torch.float64, torch.float32))
    tpost = sess.run(m.teacher.posteriors, feed_dict={m.teacher.x: px})
    t_ref = torch.softmax(t64.maps(t64._as_input(px))[..., :c], -1).detach().numpy()
    assert tpost.shape == t_ref.shape and np.abs(tpost - t_ref).max() <= 2e-6          # the teacher's clean posteriors
    rs = np.random.RandomState(wseed + 7)
    shape = (N,) + tuple(in_shape[:-1])
    variants = [('plain', {}, 0., False, 1.), ('weighted', dict(bin_class_weights=CW, focal_gamma=2.), 0.3, True, 1.), ('dropout', {}, 0., False, 0.5)]
    for name, hy, unl, weights, kp in variants:
        lab = rs.randint(0, c, size=shape)
        y = (lab[..., None] == np.arange(c)).astype(np.float32)
        y[rs.rand(*shape) < unl] = 0
        vw = (0.25 + rs.rand(*shape)).astype(np.float32) if weights else None
        if weights:
            vw[rs.rand(*shape) < 0.05] = 0
        ycols = np.ascontiguousarray(y.reshape(-1, c).T)
        hyf = dict(loss_name='CE', **hy)
        m.set_hypers(dict(NN_extended.CNN.DEFAULT_HYPERS, **hyf))
        refs = []
        for g, gt in ((g64, t64), (g32, t32)):
            g.drop = dict(DROP) if kp < 1. else None
            val, diff, raw = _au_reference(g, gt, hyf, x, px, ycols, None if vw is None else vw.reshape(-1), measure, coeff, N, c, KAPPA)
            refs.append((float(val.detach()), dense_ref.flat_grads(g, diff), raw))
            g.drop = None
        (l64, gr64, raw64), (_, gr32, _) = refs
        assert _raw_is_clear(raw64), (net, name, xseed)
        t, n = m._as_device_batch(x)
        gsum, l_dev = m._objective_pass(t, n, ycols, kp, DROP['seed'], None if vw is None else vw.reshape(-1), None, mt_feed=dict(kp=1., px=px))
        gdev = m.unflatten(gsum.cpu().numpy())
        rel = lambda a, b: max(np.abs(np.asarray(u, np.float64) - v).max() / (np.abs(v).max() + 1e-30) for u, v in zip(a, b))
        e_dev, e_32 = rel(gdev, gr64), rel(gr32, gr64)
        print('%s %s %s (input seed %d): loss %.9g vs %.9g, labelled %.6g cons %.6g, gradients e_dev %.3e e_32 %.3e e_dev / e_32 = %.2f'
              % (net, measure, name, xseed, l_dev, l64, m._mt['last'][0], m._mt['last'][1], e_dev, e_32, e_dev / max(e_32, 1e-30)))
        assert abs(l_dev - l64) <= 1e-6 * abs(l64), (name, l_dev, l64)
        _close(gdev, gr64, name='%s %s %s' % (net, measure, name))
        assert np.abs(gdev[-2][..., c]).max() > 0 and np.abs(gdev[-1][c]) > 0          # the log-variance channel has a gradient
        if kp == 1.:          # the same figures through the reference's call shapes
            fd = {m.x: x, m.y_: y, m.keep_prob: 1., m.perturbed_x: px}
            if vw is not None:
                fd[m.input_vox_weights] = vw
            assert sess.run(m.loss, feed_dict=fd) == l_dev
            lab_l, cons_l = sess.run(m.labeled_loss, feed_dict=fd), sess.run(m.cons_loss, feed_dict=fd)
            assert lab_l + coeff * cons_l == l_dev
    m.teacher.close()
    m.close()


def _au_model(sess, tag, mt=True, **kw):
    from nnal_amd import NN_extended
    ld, sk, pars, tpars, x, px, _ = _net_inputs('2d')
    hy = dict(MT_SSL=True, output_perturbation_measure='L2', max_cons_coeff=150., rampup_length=1., learning_rate=0.01) if mt else {}
    m = NN_extended.CNN((16, 16, 1), ld, tag, list(sk), dropout=[[0], 0.5], sess=sess, max_batch=3, AU_4U=True, AU_log_rel_coeff=KAPPA,
                        **dict(hy, **kw))
    m.set_weights(pars)
    return m, ld, sk, pars, tpars, x, px


def test_sess_run_of_au_vals_and_output(sess):
    import torch
    from nnal_amd import eval_utils
    m, ld, sk, pars, _, x, _ = _au_model(sess, 'au run', mt=False)          # without MT_SSL the model builds and evaluates
    c, N = 2, x.shape[0]
    with pytest.raises(NotImplementedError):
        m.get_optimizer()
    au = sess.run(m.AU_vals, feed_dict={m.x: x, m.keep_prob: 1.})
    out = sess.run(m.output, feed_dict={m.x: x, m.keep_prob: 1.})
    assert au.shape == (N, 16, 16) and out.shape == (N, 16, 16, c + 1) and au.dtype == np.float32
    assert np.array_equal(au, np.maximum(out[..., c], np.float32(0.))) and (au == 0).any() and (au > 0).any()
    post = sess.run(m.posteriors, feed_dict={m.x: x, m.keep_prob: 1.})
    assert post.shape == (N, 16, 16, c)
    z64, z32 = (dense_ref.DenseGraph(ld, (16, 16, 1), pars, sk, dt) for dt in (torch.float64, torch.float32))
    with torch.no_grad():
        r64, r32 = (g.maps(g._as_input(x)).numpy().astype(np.float64) for g in (z64, z32))
    e_dev, e_32 = np.abs(out - r64).max(), np.abs(r32 - r64).max()
    print('output against the fp64 graph: device %.3e, fp32 torch %.3e, ratio %.2f' % (e_dev, e_32, e_dev / e_32))
    assert e_dev <= 4 * e_32
    mc = sess.run(m.output, feed_dict={m.x: x, m.keep_prob: 0.5})          # dropout is allowed ('MC-sigma')
    assert mc.shape == out.shape and not np.array_equal(mc, out)
    vol = np.ascontiguousarray(np.moveaxis(np.random.RandomState(3).randn(6, 16, 16), 0, -1))          # (h, w, z)
    np.random.seed(1)
    seg = eval_utils.full_slice_segment(m, sess, [vol], None, 'AU_vals')
    per = np.stack([sess.run(m.AU_vals, feed_dict={m.x: vol[None, :, :, k, None], m.keep_prob: 1.})[0] for k in range(6)], axis=-1)
    assert seg.shape == (16, 16, 6) and np.array_equal(seg, per)
    sig = eval_utils.full_slice_segment(m, sess, [vol], None, 'sigma')
    assert sig.shape == (c, 16, 16, 6) and np.array_equal(np.maximum(sig[0], 0.), seg) and np.array_equal(sig[0], sig[1])
    m.close()


def test_one_sgd_step_and_the_teacher(sess):
    from nnal_amd._lib import check
    torch = sess.torch
    m, ld, sk, pars, tpars, x, px = _au_model(sess, 'au step')
    m.get_optimizer()
    c, N = 2, x.shape[0]
    rs = np.random.RandomState(9)
    y = (rs.randint(0, c, size=(N, 16, 16))[..., None] == np.arange(c)).astype(np.float32)
    ycols = np.ascontiguousarray(y.reshape(-1, c).T)
    theta = sess.to_device(m.flat_params(), torch.float32)
    t, n = m._as_device_batch(x)
    g, l0 = m._objective_pass(t, n, ycols, 1., None, None, None, mt_feed=dict(kp=1., px=px))
    sess.bind_stream()
    check(sess.lib.alq_sgd_step(sess.ctx, P(theta), P(g), m.num_params, 0.01))          # theta - lr * g as the optimiser forms it
    l1 = sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1., m.perturbed_x: px})
    assert l1 == l0 and m.flat_params().tobytes() == theta.cpu().numpy().tobytes()
    moved = (m.unflatten(m.flat_params())[-2] - pars[list(pars)[-1]][0])[..., c]
    assert np.abs(moved).max() > 0          # the log-variance column of the head took a step
    sess.run(m.ema_apply)
    shapes = [a.shape for a in m.teacher.unflatten(m.teacher.flat_params())]
    assert shapes == [a.shape for a in m.unflatten(m.flat_params())] and shapes[-1] == (c + 1,) and shapes[-2][-1] == c + 1
    assert m.teacher.AU_4U and sess.run(m.teacher.posteriors, feed_dict={m.teacher.x: x}).shape == (N, 16, 16, c)
    m.teacher.close()
    m.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(sess):
    """ALQ_EINVAL / ALQ_EUNSUPPORTED before any launch: the pre-filled outputs are untouched."""
    from nnal_amd import device, netspec
    from nnal_amd._lib import LossT
    torch = sess.torch
    lib, R, c = sess.lib, 140, 2
    rs = np.random.RandomState(0)
    p, q = (sess.to_device(_posteriors(rs, c, R), torch.float32) for _ in range(2))
    au = sess.to_device(_au_plane(rs, R), torch.float32)
    lab = sess.to_device(rs.randint(0, c, size=R).astype(np.int32), torch.int32)
    rows = torch.full((R, 8), 7., dtype=torch.float32, device=sess.device)
    st = torch.full((3,), 7., dtype=torch.float64, device=sess.device)
    L, soft = LossT(0, -1., 0.7, 1., None, None, None, None), LossT(1, -1., 0.7, 1., None, None, P(p).value, None)
    sess.bind_stream()
    ok = (sess.ctx, P(p), P(q), P(au), c, R, P(lab), C.byref(L), 1., 1., 1., 0.1, 0, P(rows), P(st))
    calls = [ok[:i] + (None,) + ok[i + 1:] for i in (0, 1, 2, 3, 6, 7, 13, 14)]          # a null pointer; 3: the log-variance plane
    calls += [ok[:4] + (cc,) + ok[5:] for cc in (1, 8)] + [ok[:5] + (0,) + ok[6:], ok[:12] + (2,) + ok[13:], ok[:7] + (C.byref(soft),) + ok[8:]]
    for args in calls:
        assert lib.alq_mt_cotangent_au(*args) == EINVAL, args
    sok = (sess.ctx, P(p), P(q), P(au), c, R, P(lab), C.byref(L), 0.1, 0, P(st))
    for args in [sok[:i] + (None,) + sok[i + 1:] for i in (0, 1, 2, 3, 6, 7, 10)] + [sok[:4] + (8,) + sok[5:], sok[:5] + (0,) + sok[6:],
                                                                                 sok[:9] + (-1,) + sok[10:]]:
        assert lib.alq_mt_stats_au(*args) == EINVAL, args
    # the head's forward kernel
    Ci = 8
    x = sess.to_device(rs.randn(R, Ci).astype(np.float32), torch.float32)
    W, b = sess.to_device(rs.randn(Ci, 8).astype(np.float32), torch.float32), sess.to_device(rs.randn(8).astype(np.float32), torch.float32)
    post = torch.full((8, R), 7., dtype=torch.float32, device=sess.device)
    aud = torch.full((R,), 7., dtype=torch.float32, device=sess.device)
    hok = (sess.ctx, P(x), R, Ci, c, P(W), P(b), P(post), None, P(aud), None)
    for args in [hok[:i] + (None,) + hok[i + 1:] for i in (0, 1, 5, 6, 7, 9)] + [hok[:2] + (0,) + hok[3:]]:
        assert lib.alq_dense_head_fwd_au(*args) == EINVAL, args
    for args in [hok[:4] + (cc,) + hok[5:] for cc in (1, 8)] + [hok[:3] + (6,) + hok[4:], hok[:3] + (68,) + hok[4:]]:
        assert lib.alq_dense_head_fwd_au(*args) == EUNSUPPORTED, args
    assert (rows == 7.).all() and (st == 7.).all() and (post == 7.).all() and (aud == 7.).all()
    # alq_model_set_aleatoric: an fc head, a 2-channel conv head
    ldf, skf = netspec.net_c_2d(2)
    mf = device.DeviceModel(sess, ldf, (16, 16, 1), skf, max_batch=2)
    assert lib.alq_model_set_aleatoric(mf._m, 1) == EUNSUPPORTED and lib.alq_model_set_aleatoric(None, 1) == EINVAL
    mf.close()
    m2, _, _, _ = _dense_model(sess, 'au refuse 2')
    assert lib.alq_model_set_aleatoric(m2._m, 1) == EUNSUPPORTED
    V = m2.out_voxels
    xm = sess.to_device(rs.randn(2, 256).astype(np.float32), torch.float32)
    labd = sess.to_device(rs.randint(0, 2, size=2 * V).astype(np.int32), torch.int32)
    tq = sess.to_device(_posteriors(rs, 2, 2 * V), torch.float32)
    g2 = torch.full((m2.num_params,), 7., dtype=torch.float32, device=sess.device)
    aum = torch.full((2 * V,), 7., dtype=torch.float32, device=sess.device)
    # a model without the flag: the _au entry points are unsupported
    assert lib.alq_param_grads_loss_mt_au(m2._m, P(xm), 2, P(labd), C.byref(L), 1., P(tq), 0, 1., 1., 0.1, 1., 0, 0, None, 0, P(g2), None,
                                          P(st)) == EUNSUPPORTED
    assert lib.alq_forward_au(m2._m, P(xm), 2, 1., 0, 0, None, 0, None, None, P(aum), None) == EUNSUPPORTED
    assert (g2 == 7.).all() and (aum == 7.).all()
    m2.close()
    # an aleatoric model: the plain gradient entry points are unsupported, the checks of alq_mt_cotangent_au hold
    m3, _, _, _ = _dense_model(sess, 'au refuse 3', c=3)
    assert lib.alq_model_set_aleatoric(m3._m, 1) == 0
    g3 = torch.full((m3.num_params,), 7., dtype=torch.float32, device=sess.device)
    assert lib.alq_param_grads_loss(m3._m, P(xm), 2, P(labd), C.byref(L), 1., 0., 1., 0, 0, None, 0, P(g3), None, P(st)) == EUNSUPPORTED
    assert lib.alq_param_grads_loss_mt(m3._m, P(xm), 2, P(labd), C.byref(L), 1., P(tq), 0, 1., 1., 0, 0, None, 0, P(g3), None, P(st)) == EUNSUPPORTED
    dok = (m3._m, P(xm), 2, P(labd), C.byref(L), 1., P(tq), 0, 1., 1., 0.1, 1., 0, 0, None, 0, P(g3), None, P(st))
    for args in [dok[:i] + (None,) + dok[i + 1:] for i in (0, 1, 3, 4, 6, 16)] + [dok[:2] + (0,) + dok[3:], dok[:2] + (99,) + dok[3:],
                                                                                 dok[:7] + (5,) + dok[8:], dok[:4] + (C.byref(soft),) + dok[5:]]:
        assert lib.alq_param_grads_loss_mt_au(*args) == EINVAL, args
    fok = (m3._m, P(xm), 2, 1., 0, 0, None, 0, None, None, P(aum), None)
    for args in [fok[:i] + (None,) + fok[i + 1:] for i in (0, 1, 10)] + [fok[:2] + (99,) + fok[3:]]:
        assert lib.alq_forward_au(*args) == EINVAL, args
    assert (g3 == 7.).all() and (st == 7.).all() and (aum == 7.).all()
    m3.close()
