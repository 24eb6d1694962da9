"""The fused diagonal Fisher (alq_diag_fisher, csrc/dfisher.hip), the masks of partial fine-tuning (alq_topk_mask,
alq_threshold_mask) and masked train steps on the device, against the fp64 oracle, the rows arm and NumPy (GPU box)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests.test_gpu_egl import _mk, _nets  # noqa: E402

N_S = 9            # samples: three passes of max_batch = 4, the last partial


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _data(in_shape, n=N_S, seed=7):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, *in_shape).astype(np.float32)
    lab = rs.randint(0, 2, size=n)
    if n > 1:
        lab[0], lab[1] = 0, 1      # both classes, whatever the draw
    return x, lab


_cache = {}


def _case(sess, name):
    """Per net, computed once and left unchanged: the fp64 oracle, the fused arm and the rows arm (max_batch = 4)."""
    if name not in _cache:
        import torch
        _, ld, in_shape, sk = [c for c in _nets() if c[0] == name][0]
        m, pars = _mk(sess, ld, in_shape, sk, 71, max_batch=4)
        x, lab = _data(in_shape)
        om = OracleModel(ld, in_shape, pars, skips=sk, dtype=torch.float64)
        ref = None
        for i in range(N_S):
            g = [np.asarray(a, dtype=np.float64) ** 2 for a in om.grad_log_post(int(lab[i]), x[[i]])]
            ref = g if ref is None else [a + b for a, b in zip(ref, g)]
        ref = [a / N_S for a in ref]
        fused = m.diagonal_fisher(x, lab)
        rows = m.diagonal_fisher(x, lab, fused=False)
        names = [n_ + p for n_ in m.var_names for p in ('/W', '/b')]
        m.close()
        _cache[name] = dict(ref=ref, fused=fused, rows=rows, names=names)
    return _cache[name]


NET_NAMES = [c[0] for c in _nets()]


@pytest.mark.parametrize('name', NET_NAMES)
def test_diag_fisher_vs_fp64_oracle(sess, name):
    """Per variable in TF shape (a misplaced or transposed tile fails): |d - ref| <= 2e-3 ref + 1e-6 max(ref of the variable),
    the bound of test_gpu_train.test_diagonal_fisher_vs_oracle."""
    c = _case(sess, name)
    assert len(c['fused']) == len(c['ref'])
    for nme, d, r in zip(c['names'], c['fused'], c['ref']):
        assert d.shape == r.shape and d.dtype == np.float64, nme
        err = np.abs(d - r)
        bound = 2e-3 * r + 1e-6 * r.max()
        print('%s %s: max err / max ref = %.3e' % (name, nme, err.max() / r.max()))
        assert np.all(err <= bound), (name, nme, float((err - bound).max()))


@pytest.mark.parametrize('name', NET_NAMES)
def test_diag_fisher_error_against_rows_arm(sess, name):
    """Per variable E = max|d - ref| / max|ref| of both arms against the fp64 oracle; the bar is E_fused <= max(2 E_rows, 1e-6):
    both arms accumulate in fp32 in different orders and squaring doubles a relative error."""
    c = _case(sess, name)
    bad = []
    for nme, f, w, r in zip(c['names'], c['fused'], c['rows'], c['ref']):
        ef = np.abs(f - r).max() / np.abs(r).max()
        er = np.abs(w - r).max() / np.abs(r).max()
        print('%s %s: E_fused = %.3e  E_rows = %.3e' % (name, nme, ef, er))
        if not ef <= max(2 * er, 1e-6):
            bad.append((nme, ef, er))
    assert not bad, (name, bad)


@pytest.mark.parametrize('name', NET_NAMES)
def test_diag_fisher_pass_cuts(sess, name):
    """max_batch 4 (three passes) against 16 (one pass): the per-sample terms are the same numbers, so the sums differ by
    the fp64 reassociation of n non-negative terms only, |a - b| <= n 2^-52 a per entry."""
    _, ld, in_shape, sk = [c for c in _nets() if c[0] == name][0]
    x, lab = _data(in_shape)
    a = _case(sess, name)['fused']
    m16, _ = _mk(sess, ld, in_shape, sk, 71, max_batch=16)
    b = m16.diagonal_fisher(x, lab)
    m16.close()
    for nme, u, v in zip(_case(sess, name)['names'], a, b):
        assert np.all(np.abs(u - v) <= N_S * 2.0 ** -52 * u), (name, nme, np.abs(u - v).max())


def test_diag_fisher_two_runs_bit_equal(sess):
    ld, sk = netspec.net_c()
    in_shape = (12, 8, 16, 1)
    m, _ = _mk(sess, ld, in_shape, sk, 71, max_batch=4)
    x, lab = _data(in_shape)
    a = m.diagonal_fisher(x, lab)
    b = m.diagonal_fisher(x, lab)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    m.close()


def test_diag_fisher_mid_size_vs_rows_arm(sess):
    """netc at 16^3, 37 samples in passes of 16 (several sample groups per launch, a partial last pass), on the device:
    |fused - rows| <= 2e-5 rows or rows < 1e-12 sum, the bound of test_grad_sqnorms_vs_materialised_gradients."""
    ld, sk = netspec.net_c()
    in_shape = (16, 16, 16, 1)
    m, _ = _mk(sess, ld, in_shape, sk, 63, max_batch=16)
    x, lab = _data(in_shape, n=37, seed=9)
    f = np.concatenate([a.ravel() for a in m.diagonal_fisher(x, lab)])
    r = np.concatenate([a.ravel() for a in m.diagonal_fisher(x, lab, fused=False)])
    err = np.abs(f - r)
    ok = (err <= 2e-5 * r) | (r < 1e-12 * r.sum())
    assert np.all(ok), (err[~ok].max(), int((~ok).sum()))
    m.close()


def test_diag_fisher_argument_errors(sess):
    torch = sess.torch
    in_shape = (20, 20, 1)
    m, _ = _mk(sess, netspec.net_a(), in_shape, (), 71, max_batch=4)
    x, lab = _data(in_shape)
    t = sess.to_device(x.reshape(N_S, -1), torch.float32)
    cls = sess.to_device(lab.astype(np.int32), torch.int32)
    acc = torch.full((m.num_params,), 3.0, dtype=torch.float64, device=sess.device)
    p = lambda q: C.c_void_p(q.data_ptr())       # noqa: E731
    f = m.lib.alq_diag_fisher
    sess.bind_stream()
    assert f(None, p(t), 4, p(cls), p(acc)) != 0
    assert f(m._m, None, 4, p(cls), p(acc)) != 0
    assert f(m._m, p(t), 4, None, p(acc)) != 0
    assert f(m._m, p(t), 4, p(cls), None) != 0
    assert f(m._m, p(t), 0, p(cls), p(acc)) != 0
    assert f(m._m, p(t), 5, p(cls), p(acc)) != 0          # N > max_batch
    bad = cls.clone()
    bad[2] = 2                                             # a class of c: refused before anything is written
    assert f(m._m, p(t), 4, p(bad), p(acc)) != 0
    assert b'class' in m.lib.alq_last_error()
    assert bool((acc == 3.0).all())
    assert f(m._m, p(t), 4, p(cls), p(acc)) == 0           # the call adds to what it finds
    assert bool((acc >= 3.0).all()) and bool((acc > 3.0).any())
    m.close()


def test_diag_fisher_default_labels_are_predictions(sess):
    in_shape = (20, 20, 1)
    m, _ = _mk(sess, netspec.net_a(), in_shape, (), 71, max_batch=4)
    x, _ = _data(in_shape)
    pred = m.forward(x, want=('prediction',))['prediction']
    a = m.diagonal_fisher(x)
    b = m.diagonal_fisher(x, labels=pred)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    m.close()


@pytest.mark.parametrize('name', ['netb_small', 'netc_12'])
def test_diag_fisher_sums_match_grad_sqnorms(sess, name):
    """One sample: the per-variable sums of the fused diagonal are the squared norms alq_grad_sqnorms gives for that class,
    to the 1e-4 relative that kernel holds against fp64."""
    torch = sess.torch
    _, ld, in_shape, sk = [c for c in _nets() if c[0] == name][0]
    m, _ = _mk(sess, ld, in_shape, sk, 71, max_batch=4)
    x, _ = _data(in_shape, n=1)
    t = sess.to_device(x.reshape(1, -1), torch.float32)
    for cls in (0, 1):
        d = m.diagonal_fisher(x, [cls])
        sq = m.grad_sqnorms_device(t, 1, cls=cls).cpu().numpy()[0]
        got = np.array([a.sum() for a in d])
        assert np.all(np.abs(got - sq) <= 1e-4 * sq), (name, cls, np.abs(got - sq) / sq)
    m.close()


# ------------------------------------------------------------------------------------------ masks
def _topk_mask(sess, v, k):
    torch = sess.torch
    sess.bind_stream()
    n = v.size
    dv = sess.to_device(v, torch.float64)
    mask = torch.full((n,), -1.0, dtype=torch.float32, device=sess.device)
    work = sess.empty((sess.lib.alq_topk_mask_work_bytes(n),), torch.uint8)
    rc = sess.lib.alq_topk_mask(sess.ctx, C.c_void_p(dv.data_ptr()), n, int(k), C.c_void_p(mask.data_ptr()), C.c_void_p(work.data_ptr()))
    return rc, mask.cpu().numpy()


def _stable_mask(v, k):
    want = np.zeros(v.size, dtype=np.float32)
    want[np.argsort(-v, kind='stable')[:k]] = 1
    return want


@pytest.mark.parametrize('k', [0, 1, 17, 999, 1000])
def test_topk_mask_small_with_duplicates(sess, k):
    rs = np.random.RandomState(5)
    v = rs.randint(0, 40, size=1000).astype(np.float64) / 8.0       # many duplicates, zeros among them
    v[::97] = -v[::97]                                               # either sign, -0.0 included
    rc, mask = _topk_mask(sess, v, k)
    assert rc == 0
    np.testing.assert_array_equal(mask, _stable_mask(v, k))


def test_topk_mask_large(sess):
    rs = np.random.RandomState(6)
    n = (1 << 20) + 3
    v = np.abs(rs.randn(n))
    rep = rs.choice(n, size=n // 100, replace=False)
    k = n // 10
    v[rep] = np.sort(v)[n - k]                                       # 1 % exact repeats, of the value where the cut falls
    rc, mask = _topk_mask(sess, v, k)
    assert rc == 0
    assert int(mask.sum()) == k
    want = _stable_mask(v, k)
    assert 0 < want[rep].sum() < rep.size                            # the cut runs through the tied entries
    np.testing.assert_array_equal(mask, want)


def test_topk_mask_rejects_k_above_n(sess):
    rc, _ = _topk_mask(sess, np.arange(10, dtype=np.float64), 11)
    assert rc != 0
    rc, _ = _topk_mask(sess, np.arange(10, dtype=np.float64), -1)
    assert rc != 0


def test_threshold_mask_exact_at_ties(sess):
    torch = sess.torch
    rs = np.random.RandomState(8)
    v = rs.randint(0, 50, size=5003).astype(np.float64) / 16.0
    thr = 1.25
    assert (v == thr).any()
    m, _ = _mk(sess, netspec.net_a(), (20, 20, 1), (), 71, max_batch=4)
    dv = sess.to_device(v, torch.float64)
    np.testing.assert_array_equal(m.pft_mask_device(dv, thr=thr).cpu().numpy(), (v >= thr).astype(np.float32))
    np.testing.assert_array_equal(m.pft_mask_device(dv, k=100).cpu().numpy(), _stable_mask(v, 100))
    with pytest.raises(ValueError):
        m.pft_mask_device(dv)
    m.close()


# ------------------------------------------------------------------------------------------ masked steps
def _train_setup(sess, opt, seed=71):
    in_shape = (20, 20, 1)
    m, pars = _mk(sess, netspec.net_a(), in_shape, (), seed, max_batch=8)
    m.get_optimizer(0.05 if opt == 'SGD' else 1e-3, optimizer_name=opt)
    x, lab = _data(in_shape, n=12, seed=11)
    y = np.zeros((2, 12))
    y[lab, np.arange(12)] = 1
    return m, x, lab, y


def _top_mask(m, sess, x, lab, share=0.1):
    torch = sess.torch
    t = sess.to_device(x.reshape(len(x), -1), torch.float32)
    dF = m.diagonal_fisher_device(t, len(x), lab.astype(np.int32))
    assert dF.dtype == torch.float64 and tuple(dF.shape) == (m.num_params,)
    k = int(share * m.num_params)
    mask = m.pft_mask_device(dF, k=k)
    assert int(mask.sum().item()) == k
    return mask


def test_masked_sgd_steps(sess):
    """Top 10 % of the diagonal Fisher.  After two masked steps the masked-out parameters are bit-equal to the start.  The
    masked-in ones are compared with an unmasked run after the FIRST step only: the second step's gradient depends on the
    weights the mask froze, so from there on the two runs differ by design."""
    m, x, lab, y = _train_setup(sess, 'SGD')
    start = m.flat_params().copy()
    mask = _top_mask(m, sess, x, lab)
    mh = mask.cpu().numpy() > 0
    m.set_PFT_mask(mask)
    assert m.PFT_bflag
    m.train_on_batch(x, y)
    one = m.flat_params().copy()
    m.train_on_batch(x, y)
    two = m.flat_params().copy()
    np.testing.assert_array_equal(two[~mh], start[~mh])
    assert np.any(two[mh] != one[mh]) and np.any(one[mh] != start[mh])
    m.close()
    u, _, _, _ = _train_setup(sess, 'SGD')
    np.testing.assert_array_equal(u.flat_params(), start)
    u.train_on_batch(x, y)
    free = u.flat_params()
    np.testing.assert_array_equal(one[mh], free[mh])
    assert np.any(free[~mh] != start[~mh])
    u.close()


def test_masked_adam_steps(sess):
    """A mask in force from the optimiser's first step: m = v = 0 on the masked-out parameters, which do not move."""
    m, x, lab, y = _train_setup(sess, 'Adam')
    start = m.flat_params().copy()
    mask = _top_mask(m, sess, x, lab)
    mh = mask.cpu().numpy() > 0
    m.set_PFT_mask(m.unflatten(mask.cpu().numpy()))          # the list form
    for _ in range(3):
        m.train_on_batch(x, y)
    end = m.flat_params()
    np.testing.assert_array_equal(end[~mh], start[~mh])
    assert np.any(end[mh] != start[mh])
    m.set_PFT_mask(None)
    assert not m.PFT_bflag
    m.close()


def test_all_zero_layer_mask_skips_the_repack(sess):
    """A layer whose mask is all zero is left out of the `only=` list of the repack and keeps its weights; the posteriors of
    a fixed input are those of a model holding the start weights of that layer and the stepped weights of the others."""
    m, x, lab, y = _train_setup(sess, 'SGD')
    start = [a.copy() for a in m.unflatten(m.flat_params())]
    mask = [np.ones_like(a) for a in start]
    t_off = m.var_names.index('conv2')
    mask[2 * t_off][:] = 0
    mask[2 * t_off + 1][:] = 0
    seen = []
    orig = m.set_weights_device

    def spy(theta, only=None):
        seen.append(None if only is None else list(only))
        return orig(theta, only=only)
    m.set_weights_device = spy
    m.set_PFT_mask(mask)
    m.train_on_batch(x, y)
    assert seen == [[t for t in range(m.L) if t != t_off]]
    end = m.unflatten(m.flat_params())
    np.testing.assert_array_equal(end[2 * t_off], start[2 * t_off])
    np.testing.assert_array_equal(end[2 * t_off + 1], start[2 * t_off + 1])
    assert all(np.any(e != s) for q, (e, s) in enumerate(zip(end, start)) if q // 2 != t_off)
    post = m.forward(x)['posteriors']
    m.close()
    f, _, _, _ = _train_setup(sess, 'SGD')
    f.set_weights({nme: [end[2 * q], end[2 * q + 1]] for q, nme in enumerate(f.var_names)})
    np.testing.assert_array_equal(f.forward(x)['posteriors'], post)
    f.close()


def test_adam_mask_after_unmasked_steps_keeps_model_and_optimiser_in_step(sess):
    """Adam's moments persist: a layer masked to zero AFTER unmasked steps still moves on them (the mask multiplies the
    gradient only), so it must be repacked.  The posteriors of the stepped model equal those of a fresh model loaded from its
    flat_params(); once the same mask holds from the first step, the layer is left out of the repack and does not move."""
    m, x, lab, y = _train_setup(sess, 'Adam')
    for _ in range(2):
        m.train_on_batch(x, y)
    before = [a.copy() for a in m.unflatten(m.flat_params())]
    mask = [np.ones_like(a) for a in before]
    t_off = m.var_names.index('conv2')
    mask[2 * t_off][:] = 0
    mask[2 * t_off + 1][:] = 0
    seen = []
    orig = m.set_weights_device

    def spy(theta, only=None):
        seen.append(None if only is None else list(only))
        return orig(theta, only=only)
    m.set_weights_device = spy
    m.set_PFT_mask(mask)
    m.train_on_batch(x, y)
    assert seen == [list(range(m.L))]                         # nonzero moments: every layer is repacked
    end = m.unflatten(m.flat_params())
    assert np.any(end[2 * t_off] != before[2 * t_off])        # the masked layer moved on its moments
    post = m.forward(x)['posteriors']
    flat = m.flat_params().copy()
    m.close()
    f, _, _, _ = _train_setup(sess, 'Adam')
    f.set_flat_params(flat)
    np.testing.assert_array_equal(f.forward(x)['posteriors'], post)
    # the same mask from the first step of a new optimiser: zero moments, no move, no repack of that layer
    f.get_optimizer(1e-3, optimizer_name='Adam')
    seen2 = []
    orig2 = f.set_weights_device

    def spy2(theta, only=None):
        seen2.append(None if only is None else list(only))
        return orig2(theta, only=only)
    f.set_weights_device = spy2
    f.set_PFT_mask(mask)
    f.train_on_batch(x, y)
    assert seen2 == [[t for t in range(f.L) if t != t_off]]
    np.testing.assert_array_equal(f.unflatten(f.flat_params())[2 * t_off], end[2 * t_off])
    f.close()


def test_par_placeholders_feed_equals_set_PFT_mask(sess):
    a, x, lab, y = _train_setup(sess, 'SGD')
    mask = _top_mask(a, sess, x, lab, share=0.3)
    a.set_PFT_mask(mask)
    a.train_on_batch(x, y)
    want = a.flat_params().copy()
    a.close()
    b, _, _, _ = _train_setup(sess, 'SGD')
    ph = b.get_par_placeholders()
    assert ph is b.par_placeholders and len(ph) == 2 * b.L
    feed = {b.x: x, b.y_: y, b.keep_prob: 1.}
    feed.update(dict(zip(ph, b.unflatten(mask.cpu().numpy()))))
    sess.run(b.train_step, feed_dict=feed)
    np.testing.assert_array_equal(b.flat_params(), want)
    assert not b.PFT_bflag                                   # a fed mask holds for its step only
    b.close()
