"""Test-set evaluation on the device (GPU box): alq_eval_counts against NumPy's get_preds_stats - exact integer equality over
sizes, mask types, chunkings and orders -, the uint8 scatter, the bad-index status, and eval_counts_device / test_eval /
full_model_eval / eval_MultimgAL against host recomputations from batch_eval(..., 'prediction'): the predictions come from
the same kernels, so every comparison is an equality."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from tests.test_oracle_golden import Expr, build_fisher_model  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _stats(preds, labels):
    from nnal_amd import PW_analyze_results as R
    return np.array(R.get_preds_stats(np.asarray(preds), np.asarray(labels)))


def _labels(rs, n, dtype):
    return rs.choice(np.array([np.nan, 0., 1., 2., -1.]), size=n, p=[.15, .35, .3, .1, .1]).astype(dtype)


def _counts(sess, pred, inds, mask, seg=None, counts=None):
    torch = sess.torch
    c = counts if counts is not None else torch.zeros(6, dtype=torch.int64, device=sess.device)
    sess.eval_counts(sess.to_device(pred, torch.int64), sess.to_device(inds, torch.int64) if inds is not None else None,
                     mask if isinstance(mask, torch.Tensor) else sess.to_device(mask, getattr(torch, str(mask.dtype))), c, seg)
    return c


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 8192, 300001])
def test_eval_counts_against_numpy(sess, n, dtype):
    torch = sess.torch
    rs = np.random.RandomState(100 + n % 97)
    pred = rs.randint(0, 2, size=n).astype(np.int64)
    # label-vector form (no indices)
    lab = _labels(rs, max(n, 1), dtype)
    got = _counts(sess, pred, None, lab[:n] if n else lab).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.float64), _stats(pred, lab[:n]))
    # volume form: indices into a larger mask
    elems = 2 * n + 77
    mask = _labels(rs, elems, dtype)
    inds = rs.permutation(elems)[:n].astype(np.int64)
    got = _counts(sess, pred, inds, mask).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.float64), _stats(pred, mask[inds]))
    if n >= 63:
        assert min(got) > 0                                   # every outcome occurs, NaN / negative labels were dropped
        assert got[0] + got[1] < n
    # a third class index is a positive prediction
    pred2 = rs.randint(0, 3, size=n).astype(np.int64)
    got = _counts(sess, pred2, inds, mask).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.float64), _stats(pred2, mask[inds]))


def test_eval_counts_accumulate_over_chunks_orders_and_runs(sess):
    torch = sess.torch
    rs = np.random.RandomState(5)
    n, elems = 300001, 400000
    mask = _labels(rs, elems, np.float64)
    dmask = sess.to_device(mask, torch.float64)
    inds = rs.permutation(elems)[:n].astype(np.int64)
    pred = rs.randint(0, 2, size=n).astype(np.int64)
    one = _counts(sess, pred, inds, dmask).cpu().numpy()
    np.testing.assert_array_equal(one.astype(np.float64), _stats(pred, mask[inds]))
    again = _counts(sess, pred, inds, dmask).cpu().numpy()
    np.testing.assert_array_equal(one, again)
    c = torch.zeros(6, dtype=torch.int64, device=sess.device)
    for a, b in ((0, 5), (5, 131072 + 9), (131072 + 9, n)):        # three unequal chunks into the same totals
        _counts(sess, pred[a:b], inds[a:b], dmask, counts=c)
    np.testing.assert_array_equal(c.cpu().numpy(), one)
    perm = rs.permutation(n)
    np.testing.assert_array_equal(_counts(sess, pred[perm], inds[perm], dmask).cpu().numpy(), one)
    # the totals are added to, never overwritten
    c2 = sess.to_device(np.array([7, 0, 1, 2, 3, 4], dtype=np.int64), torch.int64)
    _counts(sess, pred, inds, dmask, counts=c2)
    np.testing.assert_array_equal(c2.cpu().numpy(), one + np.array([7, 0, 1, 2, 3, 4]))


def test_eval_counts_scatter(sess):
    torch = sess.torch
    rs = np.random.RandomState(6)
    n, elems = 70001, 100000
    mask = _labels(rs, elems, np.float32)
    inds = rs.permutation(elems)[:n].astype(np.int64)
    pred = rs.randint(0, 3, size=n).astype(np.int64)
    seg0 = rs.randint(3, 250, size=elems).astype(np.uint8)
    seg = sess.to_device(seg0, torch.uint8)
    got = _counts(sess, pred, inds, mask, seg=seg).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.float64), _stats(pred, mask[inds]))
    want = seg0.copy()
    want[inds] = pred.astype(np.uint8)
    np.testing.assert_array_equal(seg.cpu().numpy(), want)          # bytes no index names are unchanged
    assert np.any(want == seg0)


def test_eval_counts_rejects_an_index_outside_the_volume(sess):
    """The mask tensor handed over has `elems` elements but is a view of a buffer twice as long, so the indices elems and
    elems + 5 are outside the declared volume yet inside memory this test owns: nothing can fault.  The call returns an
    error, the bad samples are neither read nor counted nor scattered (the memory behind the view holds a label that
    would count, and a seg byte that would change)."""
    from nnal_amd._lib import AlqError
    torch = sess.torch
    rs = np.random.RandomState(7)
    n, elems = 1000, 5000
    big = np.ones(2 * elems)                                          # behind the view: label 1 everywhere
    big[:elems] = _labels(rs, elems, np.float64)
    dbig = sess.to_device(big, torch.float64)
    seg_big = torch.full((2 * elems,), 200, dtype=torch.uint8, device=sess.device)
    inds = rs.permutation(elems)[:n].astype(np.int64)
    bad = inds.copy()
    bad[17], bad[900] = elems, elems + 5
    pred = np.ones(n, dtype=np.int64)
    c = torch.zeros(6, dtype=torch.int64, device=sess.device)
    with pytest.raises(AlqError, match='outside'):
        _counts(sess, pred, bad, dbig[:elems], seg=seg_big[:elems], counts=c)
    keep = np.ones(n, bool)
    keep[[17, 900]] = False
    np.testing.assert_array_equal(c.cpu().numpy().astype(np.float64), _stats(pred[keep], big[bad[keep]]))
    assert np.all(seg_big[elems:].cpu().numpy() == 200)
    neg = inds.copy()
    neg[3] = -1
    with pytest.raises(AlqError, match='outside'):
        _counts(sess, pred, neg, dbig[:elems])
    # and the context still works
    np.testing.assert_array_equal(_counts(sess, pred, inds, dbig[:elems]).cpu().numpy().astype(np.float64), _stats(pred, big[inds]))
    with pytest.raises((AlqError, AssertionError)):                   # more samples than labels, label-vector form
        _counts(sess, np.ones(10, dtype=np.int64), None, dbig[:5])


def test_eval_profile_class(sess):
    sess.prof_reset()
    sess.prof_enable(True)
    _counts(sess, np.ones(5000, dtype=np.int64), None, np.ones(5000))
    prof = sess.prof_read()
    sess.prof_enable(False)
    assert list(prof)[11] == 'eval' and prof['eval']['launches'] == 1 and prof['eval']['ms'] > 0
    assert prof['committee']['launches'] == 0


# ------------------------------------------------------------------------------------------------ through the nets
def _neta(sess, golden_dir, max_batch=64):
    from nnal_amd import device
    g = np.load(os.path.join(golden_dir, 'eval_neta.npz'))
    ld = netspec.net_a()
    pshape = tuple(int(v) for v in g['pshape'])
    in_shape = (pshape[0], pshape[1], 2 * pshape[2])
    m = device.DeviceModel(sess, ld, in_shape, (), max_batch=max_batch)
    pars = netspec.he_init(ld, in_shape, seed=int(g['wseed']), bias_std=0.05)
    m.set_weights(pars)
    return g, m, pshape, pars


def test_eval_counts_device_neta(sess, golden_dir):
    from nnal_amd import PW_NN, PW_analyze_results as R
    g, model, pshape, pars = _neta(sess, golden_dir)
    vols = [g['vol0'], g['vol1']]
    stats = g['stats'].tolist()
    pool = np.asarray(g['pool'], dtype=np.int64)
    mask = np.asarray(g['mask'], dtype=np.float64).copy()
    mask.reshape(-1)[pool[::7]] = np.nan
    labels = mask.reshape(-1)[pool]
    # the golden's weights as they are (they predict one class on this pool), then with the class-0 bias moved by the median
    # logit difference, so that both classes are predicted and all four outcomes occur
    p1 = PW_NN.batch_eval(model, sess, vols, pool, pshape, 64, stats, 'posteriors')[0]
    med = float(np.median(p1))
    assert 0. < med < 1.
    last = list(pars.keys())[-1]
    shifted = {k: [v[0].copy(), v[1].copy()] for k, v in pars.items()}
    shifted[last][1][0, 0] += np.float32(np.log(med / (1. - med)))
    for w, split in ((pars, False), (shifted, True)):
        model.set_weights(w)
        host = PW_NN.batch_eval(model, sess, vols, pool, pshape, 64, stats, 'prediction')[0]
        want = R.get_preds_stats(host, labels)
        assert want[0] > 0 and want[1] > 0 and want[0] + want[1] < len(pool)
        if split:
            assert min(want[2:]) > 0, want
        got = R.eval_counts_device(model, sess, vols, pool, pshape, 64, stats, labels)
        assert got == want and all(type(v) is float for v in got)
        assert R.eval_counts_device(model, sess, vols, pool, pshape, 64, stats, mask) == want              # volume form
        assert R.eval_counts_device(model, sess, vols, pool, pshape, 64, stats, mask.astype(np.float32)) == want
    model.close()


def test_eval_counts_device_netc_8cube(sess, golden_dir):
    """NET-C on 8^3 patches with the weights of fisher_netc_8cube.npz.  Its patches are even-sided, which the volume gather
    does not cut (patch_utils.py:1119-1121: odd sides), so the evaluated 'voxels' are rows of a patch pool handed in as the
    `_vols` object of batch_eval / eval_counts_device: the forward passes, the predictions and the counting are the same
    launches as for gathered patches."""
    from nnal_amd import PW_NN, PW_analyze_results as R, device
    torch = sess.torch
    g = np.load(os.path.join(golden_dir, 'fisher_netc_8cube.npz'))
    ld, skips, in_shape, pars = build_fisher_model(g, 'c')
    model = device.DeviceModel(sess, ld, in_shape, skips, max_batch=16)
    model.set_weights(pars)
    rs = np.random.RandomState(8)
    n = 150
    x = sess.to_device(rs.randn(n, *in_shape).astype(np.float32), torch.float32)

    class Pool(object):
        def gather(self, inds, patch_shape, stats=None, quirk=2, out_f64=False):
            return x.index_select(0, sess.to_device(np.asarray(inds, dtype=np.int64), torch.int64)).contiguous()
    inds = rs.permutation(n)
    labels = _labels(rs, n, np.float64)
    dummy = [np.zeros((1, 1, 1))]
    host = PW_NN.batch_eval(model, sess, dummy, inds, in_shape[:3], 16, [[0., 1.]], 'prediction', _vols=Pool())[0]
    want = R.get_preds_stats(host, labels)
    assert 0 < host.sum() < n, 'one-class predictions: the case shows nothing'
    assert R.eval_counts_device(model, sess, dummy, inds, in_shape[:3], 16, [[0., 1.]], labels, _vols=Pool()) == want
    model.close()


def _synthetic_subjects(tmp_path, shapes, seed=31):
    from nnal_amd import nrrd_io
    rs = np.random.RandomState(seed)
    paths = []
    os.makedirs(str(tmp_path), exist_ok=True)
    for s_, shp in enumerate(shapes):
        sub = []
        for j in range(2):
            p = str(tmp_path / ('sub%d_mod%d.nrrd' % (s_, j)))
            nrrd_io.write(p, rs.randn(*shp) * (1. + j) + 0.2 * s_)
            sub.append(p)
        mask = rs.randint(0, 2, size=shp).astype(np.float64)
        mask[rs.rand(*shp) < 0.1] = np.nan
        p = str(tmp_path / ('sub%d_mask.nrrd' % s_))
        nrrd_io.write(p, mask)
        sub.append(p)
        paths.append(sub)
    return paths


def _host_f1(model, sess, expr, paths, stats_rows):
    """test_eval recomputed on the host from batch_eval, the reference's lines."""
    from nnal_amd import PW_AL, PW_NN, PW_analyze_results as R
    inds, labels = PW_AL.gen_multimg_inds(paths, expr.pars['grid_spacing'])
    tP = tTP = tFP = 0
    rows = []
    for i in range(len(paths)):
        stats = [[stats_rows[i, 2 * j], stats_rows[i, 2 * j + 1]] for j in range(2)]
        preds = PW_NN.batch_eval(model, sess, paths[i][:-1], inds[i], expr.pars['patch_shape'], expr.pars['ntb'], stats, 'prediction')[0]
        st = R.get_preds_stats(preds, np.array(labels[i]))
        rows.append(st)
        tP, tTP, tFP = tP + st[0], tTP + st[2], tFP + st[3]
    if tTP + tFP == 0 or tP == 0:                  # where the reference's divisions raise, test_eval gives 0
        return 0, preds, np.array(rows)
    Pr, Rc = tTP / (tTP + tFP), tTP / tP
    return (2. / (1 / Pr + 1 / Rc) if Pr > 0 and Rc > 0 else 0), preds, np.array(rows)


def _neta_factory(sess, seed=61, lr=0.02):
    from nnal_amd import NN
    ld = netspec.net_a()

    def factory(e, in_shape, s):
        m = NN.CNN(in_shape, ld, 'net', None, None, sess=s, max_batch=64)
        m.set_weights(netspec.he_init(ld, in_shape, seed=seed, bias_std=0.3))
        m.get_optimizer(lr, [], 'SGD')
        return m
    return factory


def test_test_eval_on_the_device(sess, tmp_path):
    from nnal_amd import PW_AL
    from tests.test_dist_gloo import VOL_PARS
    paths = _synthetic_subjects(tmp_path / 'data', [(14, 12, 6), (12, 15, 5)])
    expr = PW_AL.Experiment_MultiImg(str(tmp_path / 'e'), dict(VOL_PARS), paths, test_paths=paths)
    expr.test_stats = PW_AL.get_stats(paths)
    model = _neta_factory(sess)(expr, (5, 5, 6), sess)
    want_F1, want_preds, want_rows = _host_f1(model, sess, expr, paths, expr.test_stats)
    assert np.all(want_rows[:, 2:] > 0), want_rows
    F1, preds = expr.test_eval(model, sess)
    assert F1 == want_F1 and preds.dtype == np.float64
    np.testing.assert_array_equal(preds, want_preds)
    np.testing.assert_array_equal(expr.test_counts, want_rows)
    model.close()


def test_full_model_eval_on_the_device(sess, tmp_path):
    from nnal_amd import PW_NN, PW_analyze_results as R, nrrd_io
    from tests.test_dist_gloo import VOL_PARS
    paths = _synthetic_subjects(tmp_path / 'data', [(20, 17, 6)])
    expr = Expr(dict(VOL_PARS, stats=[[0.1, 1.1], [0.2, 2.2]]))
    model = _neta_factory(sess)(expr, (5, 5, 6), sess)
    mask = nrrd_io.read(paths[0][-1])[0]
    slices = [1, 4, 5]
    out = str(tmp_path / 'full')
    preds, F1 = R.full_model_eval(expr, model, sess, paths[0][:-1], paths[0][-1], slices, save_dir=out)
    want = np.zeros(mask.shape)
    plane = np.arange(mask.shape[0] * mask.shape[1])
    for z in slices:
        ix = np.ravel_multi_index(np.unravel_index(plane, mask.shape[:2]) + (np.full(len(plane), z),), mask.shape)
        want.reshape(-1)[ix] = PW_NN.batch_eval(model, sess, paths[0][:-1], ix, expr.pars['patch_shape'], expr.pars['ntb'],
                                                expr.pars['stats'], 'prediction')[0]
    np.testing.assert_array_equal(preds, want)
    np.testing.assert_array_equal(preds, R.full_slice_eval(model, sess, paths[0][:-1], slices, expr.pars['patch_shape'],
                                                           expr.pars['ntb'], expr.pars['stats']))
    assert 0 < want[:, :, slices].sum() < want[:, :, slices].size
    assert F1 == R.F1_scores(want[:, :, slices], mask[:, :, slices])
    segs = nrrd_io.read(os.path.join(out, 'segs.nrrd'))[0]
    assert segs.dtype == np.uint8
    np.testing.assert_array_equal(segs, want.astype(np.uint8))
    assert float(np.loadtxt(os.path.join(out, 'F1_socre.txt'))) == F1
    model.close()


def test_run_method_then_eval_MultimgAL(sess, tmp_path):
    from nnal_amd import PW_AL, PW_analyze_results as R
    from tests.test_dist_gloo import VOL_PARS
    train = _synthetic_subjects(tmp_path / 'train', [(14, 12, 6), (12, 15, 5)], seed=4100)
    test = _synthetic_subjects(tmp_path / 'test', [(12, 12, 5), (10, 14, 4)], seed=77)
    expr = PW_AL.Experiment_MultiImg(str(tmp_path / 'e'), dict(VOL_PARS), train)
    expr.model_factory = _neta_factory(sess, lr=0.002)
    expr.add_method('entropy')
    np.random.seed(17)
    k = expr.pars['k']
    log = expr.run_method('entropy', 2 * k, sess=sess)
    assert len(log) == 2
    expr.model.close()
    scores = R.eval_MultimgAL(expr, 'entropy', test, sess=sess)
    sfile = os.path.join(expr.root_dir, 'entropy', 'test_scores.txt')
    on_disk = np.loadtxt(sfile, ndmin=2)
    assert on_disk.shape == (len(test), 2)
    np.testing.assert_array_equal(on_disk, scores)
    assert np.any(scores > 0), scores                  # not a curve of one-class models only
    state = PW_AL.LoopState(os.path.join(expr.root_dir, 'entropy'))
    model = expr.model_factory(expr, (5, 5, 6), sess)
    for i in range(2):
        model.perform_assign_ops(state.weights_path(i + 1), sess)
        for j in range(len(test)):
            sub = test[j:j + 1]
            mask = PW_AL._volume(sub[0][-1])
            st = np.array([[f(PW_AL._volume(sub[0][t])[~np.isnan(mask)]) for t in range(2) for f in (np.mean, np.std)]])
            want, _, rows = _host_f1(model, sess, expr, sub, st)
            assert scores[j, i] == want, (j, i, scores[j, i], want, rows)
    model.close()
