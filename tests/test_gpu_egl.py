"""Per-sample squared gradient norms (alq_grad_sqnorms, csrc/gnorm.hip) and the expected-gradient-length query
(NNAL.py:234-285) on the device, against the fp64 oracle and against materialised gradients (GPU box)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from oracle.model import OracleModel  # noqa: E402
from tests.test_oracle_golden import Expr  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _nets():
    ld_c, sk_c = netspec.net_c()
    ld_c2, sk_c2 = netspec.net_c_2d()
    return [('neta', netspec.net_a(), (20, 20, 1), ()),
            ('netb_small', netspec.net_b_small(), (25, 25, 2), ()),
            ('netc2d', ld_c2, (16, 16, 2), sk_c2),
            ('netc', ld_c, (8, 8, 8, 1), sk_c),
            ('netc_12', ld_c, (12, 8, 16, 1), sk_c)]


def _mk(sess, ld, in_shape, sk, seed, max_batch=16, nclass_scale=1.):
    from nnal_amd import device
    pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    last = list(pars.keys())[-1]
    pars[last][0] = (pars[last][0] * nclass_scale).astype(np.float32)
    m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
    m.set_weights(pars)
    return m, pars


def _sq(arrs):
    return np.array([np.sum(np.asarray(a, dtype=np.float64) ** 2) for a in arrs])


def _sqnorms(m, sess, x, **kw):
    t = sess.to_device(np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1), sess.torch.float32)
    return m.grad_sqnorms_device(t, len(x), **kw).cpu().numpy()


@pytest.mark.parametrize('name,ld,in_shape,sk', _nets())
def test_grad_sqnorms_vs_fp64_oracle(sess, name, ld, in_shape, sk):
    """||d log p_j / d theta_t||^2 per variable against torch autograd in fp64, classes 0 and 1, and the unit-cotangent
    form (cls = -1) as ||g_0||^2 / p1^2 on inputs whose posteriors are moderate."""
    m, pars = _mk(sess, ld, in_shape, sk, 61, nclass_scale=0.2)
    om = OracleModel(ld, in_shape, pars, skips=sk, dtype=__import__('torch').float64)
    x = np.random.RandomState(7).randn(4, *in_shape).astype(np.float32)
    p1 = om.forward(x)['posteriors'][1].astype(np.float64)
    assert np.all((p1 > 0.05) & (p1 < 0.95)), p1
    ref = {j: np.stack([_sq(om.grad_log_post(j, x[[i]])) for i in range(len(x))]) for j in (0, 1)}
    for cls in (0, 1, -1):
        got = _sqnorms(m, sess, x, cls=cls)
        assert got.shape == (len(x), 2 * m.L)
        r = ref[cls] if cls >= 0 else ref[0] / (p1[:, None] ** 2)
        tot = r.sum(axis=1, keepdims=True)
        err = np.abs(got - r)
        assert np.all(err <= 1e-4 * r + 1e-12 * tot), (name, cls, np.max(err / (r + 1e-300)))
    m.close()


def test_grad_sqnorms_per_sample_classes(sess):
    """d_cls overrides the class per sample (the ten-pass form of a c >= 20 net): rows equal the one-class passes."""
    ld = netspec.net_a(nclass=21)
    m, _ = _mk(sess, ld, (20, 20, 1), (), 62)
    x = np.random.RandomState(8).randn(9, 20, 20, 1).astype(np.float32)
    cls = np.array([0, 20, 3, 3, 7, 11, 19, 2, 5], dtype=np.int32)
    got = _sqnorms(m, sess, x, cls_per_sample=cls)
    for j in np.unique(cls):
        one = _sqnorms(m, sess, x, cls=int(j))
        np.testing.assert_array_equal(got[cls == j], one[cls == j])
    with pytest.raises(Exception):
        _sqnorms(m, sess, x, cls=-1)                        # the unit cotangent needs a two-class net
    m.close()


@pytest.mark.parametrize('name,shape,n', [('netc_16', (16, 16, 16, 1), 96), ('netc_32', (32, 32, 32, 1), 200),
                                          ('netb_small', (25, 25, 2), 200)])
def test_grad_sqnorms_vs_materialised_gradients(sess, name, shape, n):
    """Against alq_param_grads(per_sample = 1) rows, squared and summed per variable on the device in fp64."""
    torch = sess.torch
    if name.startswith('netc'):
        ld, sk = netspec.net_c()
    else:
        ld, sk = netspec.net_b_small(), ()
    m, _ = _mk(sess, ld, shape, sk, 63, max_batch=50)
    x = np.random.RandomState(9).randn(n, *shape).astype(np.float32)
    t = sess.to_device(x.reshape(n, -1), torch.float32)
    sizes = [int(np.prod(s)) for _, w, b in m.param_shapes for s in (w, b)]
    off = np.cumsum([0] + sizes)
    for cls in (1, -1):
        got = m.grad_sqnorms_device(t, n, cls=cls).cpu().numpy()
        ref = np.zeros_like(got)
        for a in range(0, n, 50):
            b = min(n, a + 50)
            if cls >= 0:
                g, _, _ = m.param_grads_device(t[a:b], b - a, 0, cls=cls)
            else:   # u = d(z0 - z1): d log p0 = p1 u
                g, post, _ = m.param_grads_device(t[a:b], b - a, 0, cls=0, want_post=True)
                g = g / post[1][:, None]
            g = g.double()
            for v in range(len(sizes)):
                ref[a:b, v] = (g[:, off[v]:off[v + 1]] ** 2).sum(dim=1).cpu().numpy()
            del g
        err = np.abs(got - ref) / (ref + 1e-300)
        assert np.all((err <= 2e-5) | (ref < 1e-12 * ref.sum(axis=1, keepdims=True))), (name, cls, err.max())
    m.close()


def test_grad_sqnorms_independent_of_pass_cut_and_run(sess):
    ld, sk = netspec.net_c()
    shape = (16, 16, 16, 1)
    x = np.random.RandomState(10).randn(37, *shape).astype(np.float32)
    m16, _ = _mk(sess, ld, shape, sk, 64, max_batch=16)
    m64, _ = _mk(sess, ld, shape, sk, 64, max_batch=64)
    a = _sqnorms(m16, sess, x, cls=-1)
    b = _sqnorms(m64, sess, x, cls=-1)
    c = _sqnorms(m64, sess, x, cls=-1)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(b, c)
    d = _sqnorms(m64, sess, x[5:9], cls=-1)
    np.testing.assert_array_equal(d, b[5:9])
    m16.close()
    m64.close()


def _assert_same_top(Q, ref_scores, k):
    """Q equals the top k of ref_scores (stable); where two scores lie within 1e-5 relative, their gap is asserted
    instead of their order."""
    ref_Q = np.argsort(-ref_scores, kind='stable')[:k]
    Q = np.asarray(Q)
    assert len(Q) == len(ref_Q)
    for r in range(len(Q)):
        if Q[r] != ref_Q[r]:
            a, b = ref_scores[Q[r]], ref_scores[ref_Q[r]]
            assert abs(a - b) <= 1e-5 * max(abs(a), abs(b)), (r, Q, ref_Q, a, b)


# ------------------------------------------------------------------------------------------------ image level
@pytest.mark.parametrize('tag', ['c3', 'c12'])
def test_image_level_egl(golden_dir, tmp_path, tag):
    import torch
    from nnal_amd import NN, NNAL, NNAL_tools, device
    sess_ = device.default_session()
    g = np.load(os.path.join(golden_dir, 'r3_imgfi.npz'))
    c, wseed, seed, k, B = [int(v) for v in g[tag + '_meta']]
    imgs = g['imgs']
    pfile = tmp_path / 'paths.txt'
    with open(pfile, 'w') as f:
        for i in range(len(imgs)):
            np.save(tmp_path / ('img_%d.npy' % i), imgs[i])
            f.write(str(tmp_path / ('img_%d.npy' % i)) + '\n')
    hw = imgs.shape[1]
    ld = netspec.net_a(nclass=c)
    in_shape = (hw, hw, 3)
    pars = netspec.he_init(ld, in_shape, seed=wseed, bias_std=0.05)
    last = list(pars.keys())[-1]
    pars[last][0] = (pars[last][0] * float(g[tag + '_logit_scale'])).astype(np.float32)
    model = NN.CNN(in_shape, ld, 'egl', len(ld) - 2, None, sess=sess_, max_batch=5)
    model.set_weights(pars)
    expr = Expr({'k': k, 'B': B, 'lambda_': 0.5, 'batch_size': 8, 'target_shape': (hw, hw), 'mean': 100.})
    expr.imgs_path_file = str(pfile)
    pool_inds = np.asarray(g[tag + '_pool_inds'])
    np.random.seed(seed)
    Q = NNAL.CNN_query(model, expr, pool_inds, 'egl', sess_, col=True)
    # the reference's loop on fp64 oracle gradients, over the same candidates and posteriors
    np.random.seed(seed)
    post = NNAL_tools.idxBatch_posteriors(model, pool_inds, expr, sess_, True)
    sel = NNAL_tools.uncertainty_filtering(post, B) if B < post.shape[1] else np.arange(post.shape[1])
    sel_post = post[:, sel].astype(np.float64)
    X, _ = NN.load_winds(pool_inds[sel], expr.imgs_path_file, (hw, hw), 100.)
    om = OracleModel(ld, in_shape, pars, dtype=torch.float64)
    scores = np.zeros(len(sel))
    T = 2 * len(pars)
    for i in range(len(sel)):
        for j in range(c):
            gr = om.grad_log_post(j, X[i:i + 1].astype(np.float32))
            class_score = 0.
            for tt in range(T):
                class_score += np.sum(gr[tt] ** 2)
                scores[i] += class_score * sel_post[j, i]
    _assert_same_top([list(sel).index(q) for q in Q], scores, k)
    model.close()


# ------------------------------------------------------------------------------------------------ patch-wise
def _pw_setup(sess):
    from nnal_amd import NN
    rs = np.random.RandomState(18)
    patch_shape = (5, 5, 3)
    vols = []
    for s_ in range(2):
        shp = (9 + s_, 10, 8)
        mods = [np.pad(rs.randn(*shp), [(2, 2), (2, 2), (1, 1)], 'constant') for _ in range(2)]
        vols.append(mods + [rs.randint(0, 2, size=shp)])
    pools = [np.sort(rs.permutation(9 * 10 * 8)[:170]), np.sort(rs.permutation(10 * 10 * 8)[:110])]
    stats = np.array([[0., 1., 0.1, 0.9], [0.05, 1.1, 0., 1.]])
    expr = Expr({'patch_shape': patch_shape, 'ntb': 64, 'k': 9, 'B': 40,
                 'stats': [[0., 1.], [0.1, 0.9]]}, train_stats=stats)
    expr.train_paths = [['a'], ['b']]
    ld = netspec.net_b_small()
    in_shape = (5, 5, 6)
    model = NN.CNN(in_shape, ld, 'egl', len(ld) - 2, None, sess=sess, max_batch=16)
    pars = netspec.he_init(ld, in_shape, seed=48, bias_std=0.1)
    last = list(pars.keys())[-1]
    pars[last][0] = (pars[last][0] * 0.3).astype(np.float32)
    model.set_weights(pars)
    return expr, model, pars, ld, in_shape, vols, pools


def _binary_reference(om, X, p1):
    """NNAL.py:264-283 for c = 2 on fp64 oracle gradients, posteriors (1 - p1, p1)."""
    T = 2 * om.nlayers_par
    p = np.stack([1. - p1, p1])
    scores = np.zeros(len(X))
    for i in range(len(X)):
        for j in range(2):
            gr = om.grad_log_post(j, X[i:i + 1])
            class_score = 0.
            for tt in range(T):
                class_score += np.sum(gr[tt] ** 2)
                scores[i] += class_score * p[j, i]
    return scores


def test_pw_cnn_query_egl(sess):
    import torch
    from nnal_amd import PW_NN, PW_NNAL, patch_utils
    expr, model, pars, ld, in_shape, vols, pools = _pw_setup(sess)
    imgs, pool = vols[0][:-1], pools[0]
    Q = PW_NNAL.CNN_query(expr, model, sess, imgs, pool, [], 'egl')
    posts = PW_NN.batch_eval(model, sess, imgs, pool, expr.pars['patch_shape'], expr.pars['ntb'], expr.pars['stats'],
                             'posteriors')[0]
    sel = PW_NNAL.binary_uncertainty_filter(posts, expr.pars['B'])
    dv = patch_utils.DeviceVolumes(sess, imgs)
    X = dv.gather(pool[sel], expr.pars['patch_shape'], np.asarray(expr.pars['stats'], dtype=np.float64)[:2], quirk=1)
    X = X.cpu().numpy().reshape(len(sel), *in_shape)
    om = OracleModel(ld, in_shape, pars, dtype=torch.float64)
    scores = _binary_reference(om, X, posts[sel].astype(np.float64))
    _assert_same_top([list(sel).index(q) for q in Q], scores, expr.pars['k'])
    model.close()


def test_pw_query_multimg_egl(sess):
    import torch
    from nnal_amd import PW_NNAL, patch_utils
    expr, model, pars, ld, in_shape, vols, pools = _pw_setup(sess)
    Q = PW_NNAL.query_multimg(expr, model, sess, vols, pools, None, 'egl')
    sel, sel_posts = PW_NNAL.bin_uncertainty_filter_multimg(expr, model, sess, vols, pools, expr.pars['B'])
    Xs, ps = [], []
    for i in range(2):
        dv = patch_utils.DeviceVolumes(sess, vols[i][:-1])
        X = dv.gather(np.asarray(pools[i])[np.asarray(sel[i])], expr.pars['patch_shape'], expr.train_stats[i, :4], quirk=0)
        Xs.append(X.cpu().numpy().reshape(len(sel[i]), *in_shape))
        ps.append(np.asarray(sel_posts[i], dtype=np.float64))
    om = OracleModel(ld, in_shape, pars, dtype=torch.float64)
    scores = _binary_reference(om, np.concatenate(Xs), np.concatenate(ps))
    n0 = len(sel[0])
    glob = [list(sel[0]).index(q) for q in Q[0]] + [n0 + list(sel[1]).index(q) for q in Q[1]]
    ref_Q = np.argsort(-scores, kind='stable')[:expr.pars['k']]
    got = np.sort(glob)
    want = np.sort(ref_Q)
    if not np.array_equal(got, want):      # only candidates tied to 1e-5 with the k-th score may differ
        kth = scores[ref_Q[-1]]
        for q in set(got) ^ set(want):
            assert abs(scores[q] - kth) <= 1e-5 * abs(kth), (q, scores[q], kth)
    model.close()
