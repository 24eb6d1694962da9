"""The committee queries `ensemble` and `QBC-JS` of query_multimg (PW_NNAL.py:453-545), host side: the member loop, the
holder, the RNG stream, run_method and the sharded sweep against a literal restatement of the reference, on the
oracle-backed CPU fakes of tests/fake_device.py (extended here), and the new C symbol (no GPU needed)."""
import os
import re
import subprocess
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import select_ref
from tests.fake_device import FakeModel, FakeSession, FakeVolumes


# ------------------------------------------------------------------------------------------------ fakes
class CommitteeSession(FakeSession):
    """FakeSession + the committee update (NumPy float64, the reference's formulas in its order), the top-k in numeric key
    order for either sign (alq_topk_uncertain) and a train_step routed to the model that owns it."""

    def __init__(self):
        self.members = []                   # every member's p1 as handed to committee_update (what the device sweep gave)

    def committee_update(self, p1, member, mode, mean_p, mean_h=None, keys=None):
        p = p1.numpy().astype(np.float64)
        self.members.append(p.copy())
        i = member
        mp_ = mean_p.numpy() if i else 0
        av = (p + i * mp_) / (i + 1)
        mean_p.copy_(torch.as_tensor(av))
        if mode == 1:
            h = _ent(p)
            mh = mean_h.numpy() if i else 0
            avh = (h + i * mh) / (i + 1)
            mean_h.copy_(torch.as_tensor(avh))
            if keys is not None:
                keys.copy_(torch.as_tensor(0.0 - (_ent(av) - avh)))
        elif keys is not None:
            keys.copy_(torch.as_tensor(np.abs(av - .5)))

    def topk_smallest(self, keys, B):
        return torch.as_tensor(select_ref.topk_ref(keys.numpy(), B))

    def run(self, fetch, feed_dict=None):
        m = fetch.model
        return m.train_on_batch(torch.as_tensor(np.asarray(feed_dict[m.x], dtype=np.float32)), feed_dict[m.y_])


class _Handle(object):
    def __init__(self, name, model):
        self.name, self.model = name, model


class MemberModel(FakeModel):
    """FakeModel with its own train_step handle, set_weights / var_dict (the holder is loaded from the model's weights in
    memory) and nclass."""
    nclass = 2

    def __init__(self, *a, **kw):
        FakeModel.__init__(self, *a, **kw)
        self.train_step = _Handle('train_step', self)

    @property
    def var_dict(self):
        return OrderedDict((n, wb) for n, wb in self.weights().items())

    def set_weights(self, pars):
        with torch.no_grad():
            for n, (w, b) in self.om.params.items():
                w.copy_(torch.as_tensor(np.asarray(pars[n][0])))
                b.copy_(torch.as_tensor(np.asarray(pars[n][1])))


def _ent(x):
    """-x log x - (1-x) log(1-x) with the reference's lifting (PW_NNAL.py:524-529), x not modified."""
    a, b = x.copy(), 1 - x
    a[a == 0] += 1e-6
    b[b == 0] += 1e-6
    return -a * np.log(a) - b * np.log(b)


# ------------------------------------------------------------------------------------------------ restatement
def _reference(expr, holder, sess, imgs, pool_inds, labeled_inds, method_name):
    """PW_NNAL.py:453-545 as written (stable sorts: ties -> lower position), through the project's
    bin_uncertainty_filter_multimg on the fakes; expr.prev_weights_path is the members' start."""
    from nnal_amd import PW_AL, PW_NNAL, patch_utils
    k = expr.pars['k']
    img_ind_sizes = [len(p) for p in pool_inds]
    n_labels = np.sum([len(labeled_inds[i]) for i in range(len(labeled_inds))])
    av_posts = 0
    av_ents = 0
    x_feed_dict = {holder.keep_prob: 1.}
    members = []
    for i in range(len(expr.pretrained_paths)):
        if n_labels == 0:
            holder.perform_assign_ops(expr.pretrained_paths[i], sess)
        else:
            holder.perform_assign_ops(expr.prev_weights_path, sess)
            PW_AL.finetune_multimg(expr, holder, sess, imgs, labeled_inds)
        posts = PW_NNAL.bin_uncertainty_filter_multimg(expr, holder, sess, imgs, pool_inds, k, x_feed_dict)
        members.append(posts.copy())
        av_posts = (posts + i * av_posts) / (i + 1)
        if method_name == 'QBC-JS':
            neg_posts = 1 - posts
            posts[posts == 0] += 1e-6
            neg_posts[neg_posts == 0] += 1e-6
            ents = -posts * np.log(posts) - neg_posts * np.log(neg_posts)
            av_ents = (ents + i * av_ents) / (i + 1)
    if method_name == 'ensemble':
        inds = np.argsort(np.abs(av_posts - .5), kind='stable')[:k]
    else:
        av_neg_posts = 1 - av_posts
        av_posts[av_posts == 0] += 1e-6
        av_neg_posts[av_neg_posts == 0] += 1e-6
        ent_av_posts = -av_posts * np.log(av_posts) - av_neg_posts * np.log(av_neg_posts)
        scores = ent_av_posts - av_ents
        inds = np.argsort(-scores, kind='stable')[:k]
    return patch_utils.global2local_inds(inds, img_ind_sizes), members


# ------------------------------------------------------------------------------------------------ set-up
class Expr(object):
    def __init__(self, pars, train_stats):
        self.pars = pars
        self.train_stats = train_stats


def _setup(tmp_path, M, saturate=(), same=False, k=9, rs_seed=3):
    """3 subjects (the middle one with an empty pool), NET-A on 5x5x(2x3) patches, M member weight files."""
    from oracle import netspec
    rs = np.random.RandomState(rs_seed)
    patch_shape = (5, 5, 3)
    imgs, pools = [], []
    for s_, shp in enumerate([(8, 9, 5), (7, 7, 4), (9, 8, 4)]):
        mods = [np.pad(rs.randn(*shp) * (1 + j), [(2, 2), (2, 2), (1, 1)], 'constant') for j in range(2)]
        imgs.append(mods + [rs.randint(0, 2, size=shp).astype(np.float64)])
        nv = int(np.prod(shp))
        pools.append([] if s_ == 1 else list(np.sort(rs.permutation(nv)[:60 + 10 * s_])))
    stats = np.array([[0., 1., 0.1, 1.9], [0., 1., 0., 1.], [0.05, 1.1, 0., 2.1]])
    expr = Expr({'patch_shape': patch_shape, 'ntb': 32, 'k': k, 'B': 40, 'epochs': 2, 'b': 4}, stats)
    ld = netspec.net_a()
    in_shape = (5, 5, 6)
    paths = []
    for i in range(M):
        pars = netspec.he_init(ld, in_shape, seed=0 if same else 70 + i, bias_std=0.2)
        if i in saturate:
            pars['fc1'][0] = (pars['fc1'][0] * 400.).astype(np.float32)
        m = MemberModel(ld, in_shape, pars)
        p = str(tmp_path / ('member_%d.npz' % i))
        m.save_weights(p)
        paths.append(p)
    expr.pretrained_paths = paths

    def mk(seed=90):
        return MemberModel(ld, in_shape, netspec.he_init(ld, in_shape, seed=seed, bias_std=0.1), lr=0.05)
    return expr, imgs, pools, mk


@pytest.fixture
def fakes(monkeypatch):
    from nnal_amd import patch_utils
    from oracle import alpath
    monkeypatch.setattr(patch_utils, 'DeviceVolumes', FakeVolumes)
    monkeypatch.setattr(patch_utils, 'get_patches_multimg', alpath.get_patches_multimg)


def _run(expr, model, sess, imgs, pools, labeled, method):
    from nnal_amd import PW_NNAL
    return PW_NNAL.query_multimg(expr, model, sess, imgs, pools, labeled, method)


def _eq(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64))


# ------------------------------------------------------------------------------------------------ tests
def test_committee_symbol_is_declared_and_exported():
    from nnal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'alq.h')).read()
    assert re.search(r'\bint alq_committee_update\(alq_ctx \*ctx, const float \*d_p1, int64_t n, int member, int mode, '
                     r'double \*d_mean_p,', hdr)
    assert '#define ALQ_COMMITTEE_ENSEMBLE 0' in hdr and '#define ALQ_COMMITTEE_QBC_JS 1' in hdr
    assert 'alq_committee_update' in _lib.exported_names()
    _lib.build()
    nm = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert re.search(r'\bT alq_committee_update\b', nm)
    L = _lib.lib()
    assert L.alq_prof_class_name(10) == b'committee'
    assert L.alq_prof_class_name(9) == b'gnorm' and L.alq_prof_class_name(0) == b'igemm_fwd'


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
@pytest.mark.parametrize('M', [1, 3, 7])
def test_pretrained_members_match_the_reference(tmp_path, fakes, method, M):
    expr, imgs, pools, mk = _setup(tmp_path, M)
    sess = CommitteeSession()
    model = mk()
    w0 = model.weights()
    expr.model_holder = mk(91)
    got = _run(expr, model, sess, imgs, pools, [[], [], []], method)
    want, members = _reference(expr, mk(92), sess, imgs, pools, [[], [], []], method)
    _eq(got, want)
    assert len(got[1]) == 0 and sum(len(g) for g in got) == expr.pars['k']
    assert len(sess.members) == M
    for a, b in zip(sess.members, members):
        np.testing.assert_array_equal(a, b)
    for n in w0:                                             # the main model is not touched
        for a, b in zip(w0[n], model.weights()[n]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
def test_k_at_least_the_pool(tmp_path, fakes, method):
    expr, imgs, pools, mk = _setup(tmp_path, 3, k=500)
    sess = CommitteeSession()
    expr.model_holder = mk(91)
    got = _run(expr, mk(), sess, imgs, pools, [[], [], []], method)
    want, _ = _reference(expr, mk(92), sess, imgs, pools, [[], [], []], method)
    _eq(got, want)
    assert [len(g) for g in got] == [len(p) for p in pools]


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
def test_saturated_members_are_lifted(tmp_path, fakes, method):
    """Members whose posteriors are exactly 0 and 1 in places: the 1e-6 lifting of x and of 1 - x."""
    expr, imgs, pools, mk = _setup(tmp_path, 4, saturate=(1, 2))
    sess = CommitteeSession()
    expr.model_holder = mk(91)
    got = _run(expr, mk(), sess, imgs, pools, [[], [], []], method)
    want, members = _reference(expr, mk(92), sess, imgs, pools, [[], [], []], method)
    _eq(got, want)
    sat = np.concatenate(members[1:3])
    assert np.any(sat == 0.) and np.any(sat == 1.)


@pytest.mark.parametrize('M', [2, 3])
def test_agreeing_members_tie_at_score_zero(tmp_path, fakes, M):
    """Every member the same net: with M = 2 every QBC-JS score is exactly 0 (the reference's keys -0.0, ours +0.0):
    all rows tie and the lowest pool positions win; with M = 3 rounding leaves tiny scores of either sign."""
    expr, imgs, pools, mk = _setup(tmp_path, M, same=True)
    sess = CommitteeSession()
    expr.model_holder = mk(91)
    got = _run(expr, mk(), sess, imgs, pools, [[], [], []], 'QBC-JS')
    want, _ = _reference(expr, mk(92), sess, imgs, pools, [[], [], []], 'QBC-JS')
    _eq(got, want)
    if M == 2:
        k = expr.pars['k']
        _eq(got, [np.arange(min(k, len(pools[0]))), [], []])


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
@pytest.mark.parametrize('from_file', [True, False])
def test_labelled_members_are_finetuned_like_the_reference(tmp_path, fakes, method, from_file):
    """With labels every member starts from prev_weights_path - or, without one, from the model's weights in memory -
    and is fine-tuned once: the same members, picks and NumPy stream as the restatement; the main model is untouched."""
    expr, imgs, pools, mk = _setup(tmp_path, 3)
    labeled = [list(pools[0][:5]), [], list(pools[2][:4])]
    pools = [pools[0][5:], pools[1], pools[2][4:]]
    model = mk()
    prev = str(tmp_path / 'prev.npz')
    model.save_weights(prev)
    if from_file:
        expr.prev_weights_path = prev
    w0 = model.weights()
    sess = CommitteeSession()
    expr.model_holder = mk(91)
    np.random.seed(5)
    got = _run(expr, model, sess, imgs, pools, labeled, method)
    st_got = np.random.get_state()
    expr.prev_weights_path = prev
    np.random.seed(5)
    want, members = _reference(expr, mk(92), sess, imgs, pools, labeled, method)
    st_want = np.random.get_state()
    _eq(got, want)
    for a, b in zip(sess.members, members):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(members[0], members[1])        # the members differ through the stream
    assert st_got[0] == st_want[0] and np.array_equal(st_got[1], st_want[1]) and st_got[2:] == st_want[2:]
    for n in w0:
        for a, b in zip(w0[n], model.weights()[n]):
            np.testing.assert_array_equal(a, b)


def test_missing_pretrained_paths_and_multiclass_raise(tmp_path, fakes):
    expr, imgs, pools, mk = _setup(tmp_path, 1)
    del expr.pretrained_paths
    expr.model_holder = mk(91)
    with pytest.raises(ValueError, match='pretrained_paths'):
        _run(expr, mk(), CommitteeSession(), imgs, pools, [[], [], []], 'ensemble')
    m = mk()
    m.nclass = 3
    with pytest.raises(ValueError, match='binary'):
        _run(expr, m, CommitteeSession(), imgs, pools, [[], [], []], 'QBC-JS')


# ------------------------------------------------------------------------------------------------ run_method
def _experiment(root, data, pars, sess, methods, rounds):
    """Experiment_MultiImg over the synthetic subjects of test_dist_gloo, NET-A fakes; returns {method: [Q_mat, ...]}."""
    from nnal_amd import PW_AL
    from oracle import netspec
    from tests.test_dist_gloo import _subject_paths
    expr = PW_AL.Experiment_MultiImg(root, pars, _subject_paths(data))

    def factory(e, in_shape, s):
        ld = netspec.net_a()
        return MemberModel(ld, in_shape, netspec.he_init(ld, in_shape, seed=61, bias_std=0.05), lr=e.pars['learning_rate'])
    expr.model_factory = factory
    out = {}
    for method in methods:
        expr.add_method(method)
        np.random.seed(17)
        out[method] = [l['Q_mat'] for l in expr.run_method(method, rounds, sess=sess)]
    return expr, out


def _committee_pars(tmp_path, M=3):
    from oracle import netspec
    from tests.test_dist_gloo import VOL_PARS
    ld = netspec.net_a()
    paths = []
    for i in range(M):
        p = str(tmp_path / ('pre_%d.npz' % i))
        MemberModel(ld, (5, 5, 6), netspec.he_init(ld, (5, 5, 6), seed=300 + i, bias_std=0.1)).save_weights(p)
        paths.append(p)
    return dict(VOL_PARS, pretrained_paths=paths)


@pytest.mark.parametrize('method', ['ensemble', 'QBC-JS'])
def test_run_method_two_rounds(tmp_path, fakes, method):
    """Round 0 (no labels) queries with the pretrained members, round 1 with members fine-tuned from curr_weights_1;
    the query files and weights are written, the holder and the member list are on the experiment."""
    from tests.test_dist_gloo import _write_subjects
    data = str(tmp_path / 'data')
    os.makedirs(data)
    _write_subjects(data)
    pars = _committee_pars(tmp_path)
    k = pars['k']
    expr, out = _experiment(str(tmp_path / 'e'), data, pars, CommitteeSession(), [method], 2 * k)
    Q = out[method]
    assert len(Q) == 2 and all(len(q) == k for q in Q)
    allq = np.concatenate(Q)
    assert len(np.unique(allq, axis=0)) == len(allq)
    root = os.path.join(str(tmp_path / 'e'), method)
    for it in range(2):
        np.testing.assert_array_equal(np.loadtxt(os.path.join(root, 'queries', '%d' % it), ndmin=2).astype(np.int64), Q[it])
        assert os.path.exists(os.path.join(root, 'curr_weights_%d.npz' % (it + 1)))
    assert expr.pretrained_paths == pars['pretrained_paths']
    assert expr.prev_weights_path == os.path.join(root, 'curr_weights_1.npz')
    assert expr.model_holder is not expr.model


def test_run_method_without_pretrained_paths_raises(tmp_path, fakes):
    from tests.test_dist_gloo import VOL_PARS, _write_subjects
    data = str(tmp_path / 'data')
    os.makedirs(data)
    _write_subjects(data)
    with pytest.raises(ValueError, match='pretrained_paths'):
        _experiment(str(tmp_path / 'e'), data, dict(VOL_PARS), CommitteeSession(), ['QBC-JS'], 5)


# ------------------------------------------------------------------------------------------------ sharded
def _committee_worker(rank, ws, port, q, root, data, pars):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    if ws > 1:
        dist.init_process_group('gloo', rank=rank, world_size=ws)
    import nnal_amd  # noqa: F401
    from nnal_amd import patch_utils
    from oracle import alpath
    patch_utils.DeviceVolumes = FakeVolumes
    patch_utils.get_patches_multimg = alpath.get_patches_multimg
    sess = CommitteeSession()
    expr, out = _experiment(root, data, pars, sess, ['ensemble', 'QBC-JS'], 2 * pars['k'])
    q.put((rank, out, [len(p) for p in sess.members]))
    if ws > 1:
        dist.barrier()
        dist.destroy_process_group()


def _run_committee(ws, root, data, pars):
    from tests.test_dist_gloo import _free_port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_committee_worker, args=(r, ws, port, q, root, data, pars)) for r in range(ws)]
    for p in procs:
        p.start()
    res = {r: (out, sizes) for r, out, sizes in (q.get(timeout=600) for _ in range(ws))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def test_committee_world2_equals_single_process(tmp_path):
    """Two gloo ranks, each sweeping its block of the concatenated pool for every member, the keys assembled with
    allgather_rows: both methods' queries of two rounds (pretrained, then fine-tuned members) equal one process bit for
    bit on both ranks."""
    from tests.test_dist_gloo import _write_subjects
    data = str(tmp_path / 'data')
    os.makedirs(data)
    _write_subjects(data)
    pars = _committee_pars(tmp_path)
    one = _run_committee(1, str(tmp_path / 'e1'), data, pars)
    two = _run_committee(2, str(tmp_path / 'e2'), data, pars)
    out1, sizes1 = one[0]
    for r in (0, 1):
        outr, sizesr = two[r]
        assert all(s < s1 for s, s1 in zip(sizesr, sizes1))       # each rank swept a part of the pool
        for method in ('ensemble', 'QBC-JS'):
            assert len(out1[method]) == len(outr[method]) == 2
            for a, b in zip(out1[method], outr[method]):
                np.testing.assert_array_equal(a, b)
