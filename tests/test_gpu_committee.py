"""The committee queries `ensemble` and `QBC-JS` (PW_NNAL.py:453-545) on the device: alq_committee_update against NumPy,
query_multimg against a restatement through the project's own bin_uncertainty_filter_multimg, the fine-tuned members,
the pass cut and run_method (GPU box)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from tests.test_committee_host import Expr, _reference  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _ent(x):
    a, b = x.copy(), 1 - x
    a[a == 0] += 1e-6
    b[b == 0] += 1e-6
    return -a * np.log(a) - b * np.log(b)


def _member_p1(rs, n, i):
    p = rs.rand(n).astype(np.float32)
    special = np.array([0., 1., .5, 1e-30, 1e-20, 1e-8, 2. ** -24, 1. - 2. ** -24, 0., 1.], dtype=np.float32)
    p[:len(special)] = np.roll(special, i)                  # the specials meet each other across members
    p[rs.rand(n) < .05] = 0.
    p[rs.rand(n) < .05] = 1.
    p[-50:] = 0.25                                          # rows where every member agrees (score 0)
    return p


@pytest.mark.parametrize('M', [1, 2, 3, 4, 5, 6, 7])
def test_committee_update_against_numpy(sess, M):
    torch = sess.torch
    rs = np.random.RandomState(40 + M)
    n = 70001
    members = [_member_p1(rs, n, i) for i in range(M)]
    for mode in (0, 1):
        mp = sess.empty((n,), torch.float64)
        mh = sess.empty((n,), torch.float64) if mode else None
        keys = sess.empty((n,), torch.float64)
        av, avh = 0, 0
        for i, p32 in enumerate(members):
            p = p32.astype(np.float64)
            sess.committee_update(sess.to_device(p32, torch.float32), i, mode, mp, mh, keys if i == M - 1 else None)
            av = (p + i * av) / (i + 1)
            np.testing.assert_array_equal(mp.cpu().numpy(), av)          # bit-exact running mean, both modes
            if mode:
                avh = (_ent(p) + i * avh) / (i + 1)
                np.testing.assert_allclose(mh.cpu().numpy(), avh, rtol=0, atol=1e-14)
        k = keys.cpu().numpy()
        if mode == 0:
            np.testing.assert_array_equal(k, np.abs(av - .5))
        else:
            score = _ent(av) - avh
            np.testing.assert_allclose(k, -score, rtol=0, atol=1e-14)
            assert not np.any((k == 0) & np.signbit(k))                      # never -0.0
            if M == 1:
                np.testing.assert_array_equal(k[-50:], 0.)


def test_topk_orders_signed_keys(sess):
    """alq_topk_uncertain on keys of either sign (QBC-JS keys are 0.0 - score): numeric order, ties -> lower position."""
    torch = sess.torch
    rs = np.random.RandomState(3)
    k = np.round(rs.randn(5000), 2)
    k[:20] = 0.
    got = sess.topk_smallest(sess.to_device(k, torch.float64), 700).cpu().numpy()
    np.testing.assert_array_equal(got, np.lexsort((np.arange(len(k)), k))[:700])


# ------------------------------------------------------------------------------------------------ query_multimg
def _pw(sess, tmp_path, M, max_batch=128, seed=5):
    from nnal_amd import NN
    rs = np.random.RandomState(seed)
    patch_shape = (5, 5, 3)
    imgs, pools = [], []
    for s_, shp in enumerate([(16, 14, 6), (9, 9, 4), (14, 15, 5)]):
        mods = [np.pad(rs.randn(*shp) * (1 + j), [(2, 2), (2, 2), (1, 1)], 'constant') for j in range(2)]
        imgs.append(mods + [rs.randint(0, 2, size=shp).astype(np.float64)])
        nv = int(np.prod(shp))
        pools.append([] if s_ == 1 else list(np.sort(rs.permutation(nv)[:nv // 2])))
    stats = np.array([[0., 1., 0.1, 1.9], [0., 1., 0., 1.], [0.05, 1.1, 0., 2.1]])
    expr = Expr({'patch_shape': patch_shape, 'ntb': 64, 'k': 25, 'B': 40, 'epochs': 2, 'b': 8}, stats)
    ld = netspec.net_a()
    in_shape = (5, 5, 6)

    def mk(pars_seed=90, mb=max_batch):
        m = NN.CNN(in_shape, ld, 'committee', None, None, sess=sess, max_batch=mb)
        m.set_weights(netspec.he_init(ld, in_shape, seed=pars_seed, bias_std=0.2))
        m.get_optimizer(0.05, [], 'SGD')
        return m
    paths = []
    for i in range(M):
        m = mk(70 + i)
        p = str(tmp_path / ('member_%d.npz' % i))
        m.save_weights(p)
        m.close()
        paths.append(p)
    expr.pretrained_paths = paths
    return expr, imgs, pools, mk


def _keys(members, method):
    av, avh = 0, 0
    for i, p in enumerate(members):
        av = (p + i * av) / (i + 1)
        avh = (_ent(p) + i * avh) / (i + 1)
    return np.abs(av - .5) if method == 'ensemble' else -(_ent(av) - avh)


def _check(got, want, members, method, sizes, exact):
    """Same picks; with `exact` False, swaps only among keys within 1e-13 of the k-th key (device log against NumPy's)."""
    offs = np.cumsum([0] + sizes)
    if exact:
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
        return
    g = set(int(q + offs[i]) for i in range(len(got)) for q in got[i])
    w = [int(q + offs[i]) for i in range(len(want)) for q in want[i]]
    keys = _keys(members, method)
    kth = np.sort(keys[w])[-1]
    for q in g ^ set(w):
        assert abs(keys[q] - kth) <= 1e-13, (q, keys[q], kth)
    assert sum(len(a) for a in got) == len(w)


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
def test_query_multimg_pretrained_members(sess, tmp_path, method):
    from nnal_amd import PW_NNAL
    expr, imgs, pools, mk = _pw(sess, tmp_path, 4)
    model = mk()
    w0 = {n: [np.array(a) for a in wb] for n, wb in model.var_dict.items()}
    expr.model_holder = mk(91)
    got = PW_NNAL.query_multimg(expr, model, sess, imgs, pools, [[], [], []], method)
    ref_holder = mk(92)
    want, members = _reference(expr, ref_holder, sess, imgs, pools, [[], [], []], method)
    assert len(got[1]) == 0
    _check(got, want, members, method, [len(p) for p in pools], exact=(method == 'ensemble'))
    for n in w0:
        for a, b in zip(w0[n], model.var_dict[n]):
            np.testing.assert_array_equal(a, b)
    for m in (model, expr.model_holder, ref_holder):
        m.close()


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
def test_query_multimg_finetuned_members(sess, tmp_path, method):
    """Labels present: every member starts from prev_weights_path and is fine-tuned once on the device; the same seed gives
    the restatement's picks, the main model is untouched."""
    from nnal_amd import PW_NNAL
    expr, imgs, pools, mk = _pw(sess, tmp_path, 3)
    labeled = [list(pools[0][:12]), [], list(pools[2][:10])]
    pools = [pools[0][12:], pools[1], pools[2][10:]]
    model = mk()
    expr.prev_weights_path = str(tmp_path / 'prev.npz')
    model.save_weights(expr.prev_weights_path)
    w0 = {n: [np.array(a) for a in wb] for n, wb in model.var_dict.items()}
    expr.model_holder = mk(91)
    np.random.seed(11)
    got = PW_NNAL.query_multimg(expr, model, sess, imgs, pools, labeled, method)
    ref_holder = mk(92)
    np.random.seed(11)
    want, members = _reference(expr, ref_holder, sess, imgs, pools, labeled, method)
    assert not np.array_equal(members[0], members[1])
    _check(got, want, members, method, [len(p) for p in pools], exact=False)
    for n in w0:
        for a, b in zip(w0[n], model.var_dict[n]):
            np.testing.assert_array_equal(a, b)
    for m in (model, expr.model_holder, ref_holder):
        m.close()


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
def test_query_multimg_independent_of_pass_cut(sess, tmp_path, method):
    from nnal_amd import PW_NNAL
    expr, imgs, pools, mk = _pw(sess, tmp_path, 3)
    model = mk()
    out = []
    for mb in (64, 512):
        expr.model_holder = mk(91, mb)
        out.append(PW_NNAL.query_multimg(expr, model, sess, imgs, pools, [[], [], []], method))
        expr.model_holder.close()
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)
    model.close()


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
def test_run_method_two_rounds_on_the_device(sess, tmp_path, method):
    from nnal_amd import NN, PW_AL
    from tests.test_dist_gloo import VOL_PARS, _subject_paths, _write_subjects
    data = str(tmp_path / 'data')
    os.makedirs(data)
    _write_subjects(data)
    ld = netspec.net_a()
    paths = []
    for i in range(3):
        m = NN.CNN((5, 5, 6), ld, 'pre', None, None, sess=sess, max_batch=64)
        m.set_weights(netspec.he_init(ld, (5, 5, 6), seed=300 + i, bias_std=0.1))
        paths.append(str(tmp_path / ('pre_%d.npz' % i)))
        m.save_weights(paths[-1])
        m.close()
    pars = dict(VOL_PARS, pretrained_paths=paths)
    expr = PW_AL.Experiment_MultiImg(str(tmp_path / 'e'), pars, _subject_paths(data))

    def factory(e, in_shape, s):
        m = NN.CNN(in_shape, ld, 'net', None, None, sess=s, max_batch=64)
        m.set_weights(netspec.he_init(ld, in_shape, seed=61, bias_std=0.05))
        m.get_optimizer(e.pars['learning_rate'], [], 'SGD')
        return m
    expr.model_factory = factory
    expr.add_method(method)
    np.random.seed(17)
    k = pars['k']
    log = expr.run_method(method, 2 * k, sess=sess)
    assert len(log) == 2 and all(len(l['Q_mat']) == k for l in log)
    root = os.path.join(str(tmp_path / 'e'), method)
    for it in range(2):
        np.testing.assert_array_equal(np.loadtxt(os.path.join(root, 'queries', '%d' % it), ndmin=2).astype(np.int64),
                                      log[it]['Q_mat'])
        assert os.path.exists(os.path.join(root, 'curr_weights_%d.npz' % (it + 1)))
    allq = np.concatenate([l['Q_mat'] for l in log])
    assert len(np.unique(allq, axis=0)) == len(allq)
    expr.model.close()
    expr.model_holder.close()
