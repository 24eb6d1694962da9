"""Test-set evaluation, host side (no GPU): the metric functions of PW_analyze_results bit for bit against the reference's own
(tests/golden/eval_metrics.npz, made by tests/golden/make_golden_eval.py), Experiment_MultiImg.test_eval, eval_MultimgAL and
full_slice_eval against the reference's runs recorded there - with the golden's seeded predictor in the evaluator's place -
and on the oracle-backed CPU fakes of tests/fake_device.py (extended here with predictions and a NumPy eval_counts); the
sharded evaluation on two gloo ranks; the new C symbol."""
import importlib.util
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fake_device import FakeModel, FakeSession, FakeVolumes


# ------------------------------------------------------------------------------------------------ fakes
class EvalSession(FakeSession):
    """FakeSession + alq_eval_counts in NumPy (get_preds_stats' comparisons on mask[inds], the uint8 scatter)."""

    def __init__(self):
        self.eval_calls = 0

    def eval_counts(self, pred, inds, mask, counts, seg=None):
        self.eval_calls += 1
        assert pred.dtype == torch.int64 and counts.dtype == torch.int64 and int(counts.numel()) == 6
        assert mask.dtype in (torch.float32, torch.float64) and mask.dim() == 1
        p = pred.numpy()
        if inds is not None:
            ix = inds.numpy()
            assert ix.min() >= 0 and ix.max() < mask.numel()
            lab = mask.numpy()[ix]
        else:
            ix = np.arange(len(p))
            lab = mask.numpy()[:len(p)]
        add = [np.sum(lab > 0), np.sum(lab == 0), np.sum((p > 0) & (lab > 0)), np.sum((p > 0) & (lab == 0)),
               np.sum((p == 0) & (lab == 0)), np.sum((p == 0) & (lab > 0))]
        counts += torch.as_tensor(np.array(add, dtype=np.int64))
        if seg is not None:
            seg.numpy()[ix] = p.astype(np.uint8)


class PredModel(FakeModel):
    """FakeModel whose forward pass also returns the predictions (argmax of the posteriors, int64)."""
    nclass = 2

    def forward_device(self, t, n, want_pred=False, want_feat=False, rows=None):
        post, _, _ = FakeModel.forward_device(self, t, n, want_pred, want_feat, rows)
        return post, (torch.argmax(post, dim=0).to(torch.int64) if want_pred else None), None


class SaltModel(object):
    """The golden's model stand-in: remembers the iteration number of the weight file it was given."""
    dropout_rate = 1.
    dropout_layers = ()
    salt = 0

    def __init__(self):
        self.loaded = []

    def add_assign_ops(self):
        pass

    def perform_assign_ops(self, path, sess=None):
        self.loaded.append(path)
        self.salt = int(re.search(r'curr_weights_(\d+)', path).group(1))


def _generator(golden_dir):
    spec = importlib.util.spec_from_file_location('make_golden_eval', os.path.join(golden_dir, 'make_golden_eval.py'))
    gen = importlib.util.module_from_spec(spec)
    sys.path.insert(0, golden_dir)
    try:
        spec.loader.exec_module(gen)          # data + the seeded predictor only; main() (the reference run) is not called
    finally:
        sys.path.remove(golden_dir)
    return gen


def _write_subjects(gen, g, data):
    from nnal_amd import nrrd_io
    table, paths = gen.subjects(int(g['subject_seed']))
    os.makedirs(data, exist_ok=True)
    here = []
    for sub in paths:
        row = []
        for p in sub:
            q = os.path.join(data, os.path.basename(p))
            nrrd_io.write(q, table[p])
            row.append(q)
        here.append(row)
    return table, here


def _pars(g):
    return dict(grid_spacing=int(g['par_grid_spacing']), patch_shape=tuple(int(v) for v in g['par_patch_shape']), model_name='PW',
                dropout_rate=1., learning_rate=1e-3, grad_layers=[], train_layers=[], optimizer_name='SGD',
                init_weights_path='init', k=4, B=10, lambda_=0., ntb=int(g['par_ntb']), b=4, epochs=1,
                stats=g['par_stats'].tolist())


def _install_predictor(gen, g, calls, chunk=50):
    """Binds the golden's seeded predictor in the place of the device passes (PW_NN._eval_passes): what the golden run bound
    in the place of PW_NN.batch_eval.  Every walk is recorded with the subject, the indices and the statistics."""
    from nnal_amd import PW_NN
    shapes = [tuple(int(v) for v in s) for s in g['shapes']]

    def passes(model, sess, img_dat, inds, patch_shape, batch_size, stats, drop, want_pred, want_feat, _vols, _first_sample):
        if isinstance(img_dat[0], np.ndarray):
            r = [int((patch_shape[i] - 1) / 2.) for i in range(3)]
            subject = shapes.index(tuple(int(img_dat[0].shape[a]) - 2 * r[a] for a in range(3)))
        else:
            subject = gen.subject_of(img_dat[0])
        inds = np.asarray(inds, dtype=np.int64)
        calls.append(dict(subject=subject, inds=inds.copy(), stats=np.array(stats, dtype=np.float64), salt=model.salt,
                          n_mod=len(img_dat), patch_shape=tuple(patch_shape), ntb=batch_size))
        assert drop == (1., False, 0) and not want_feat
        for a in range(0, len(inds), chunk):
            b = min(len(inds), a + chunk)
            pred = torch.as_tensor(gen.predict(subject, inds[a:b], model.salt).astype(np.int64))
            yield a, b, torch.zeros((2, b - a), dtype=torch.float32), (pred if want_pred else None), None
    PW_NN._eval_passes = passes


def _check_calls(g, prefix, calls):
    assert len(calls) == int(g[prefix + '_n'])
    for c, d in enumerate(calls):
        assert d['subject'] == int(g['%s_%d_subject' % (prefix, c)]) and d['salt'] == int(g['%s_%d_salt' % (prefix, c)])
        np.testing.assert_array_equal(d['inds'], g['%s_%d_inds' % (prefix, c)])
        np.testing.assert_array_equal(d['stats'], g['%s_%d_stats' % (prefix, c)])
        assert d['n_mod'] == 2 and d['patch_shape'] == tuple(g['par_patch_shape']) and d['ntb'] == int(g['par_ntb'])


@pytest.fixture
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_metrics.npz'))


@pytest.fixture
def predictor(golden_dir, golden, monkeypatch):
    from nnal_amd import PW_NN, patch_utils
    gen = _generator(golden_dir)
    calls = []
    monkeypatch.setattr(PW_NN, '_eval_passes', PW_NN._eval_passes)       # restored after the test
    monkeypatch.setattr(patch_utils, 'DeviceVolumes', FakeVolumes)
    _install_predictor(gen, golden, calls)
    return gen, calls


def _experiment(root, g, paths):
    from nnal_amd import PW_AL
    expr = PW_AL.Experiment_MultiImg(root, _pars(g), paths)
    expr.add_method('entropy')
    return expr


# ------------------------------------------------------------------------------------------------ the symbol
def test_eval_symbol_is_declared_and_exported():
    from nnal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'alq.h')).read()
    assert re.search(r'\bint alq_eval_counts\(alq_ctx \*ctx, const int64_t \*d_pred, const int64_t \*d_inds, int64_t n, '
                     r'const void \*d_mask,\s+int mask_is_f64, int64_t mask_elems, int64_t \*d_counts, uint8_t \*d_seg\);', hdr)
    assert 'PW_analyze_results.py:234-258' in hdr
    assert 'alq_eval_counts' in _lib.exported_names()
    _lib.build()
    nm = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert re.search(r'\bT alq_eval_counts\b', nm)
    L = _lib.lib()
    assert L.alq_prof_num_classes() == 12
    assert L.alq_prof_class_name(11) == b'eval'
    assert L.alq_prof_class_name(0) == b'igemm_fwd' and L.alq_prof_class_name(9) == b'gnorm'
    assert L.alq_prof_class_name(10) == b'committee'
    src = os.path.join(_lib._HERE, 'csrc', 'build.sh')
    assert open(src).read().count('evalcounts') == 2                  # the compile list and the link list


# ------------------------------------------------------------------------------------------------ host metrics
def test_host_metrics_equal_the_reference_bit_for_bit(golden):
    from nnal_amd import PW_analyze_results as R
    g = golden
    for c in range(int(g['n_metric_cases'])):
        preds, mask = g['m%d_preds' % c], g['m%d_mask' % c]
        st = R.get_preds_stats(preds, mask)
        assert isinstance(st, tuple) and len(st) == 6 and all(type(v) is float for v in st)
        np.testing.assert_array_equal(np.array(st), g['m%d_stats' % c])
        fm, f1 = R.get_Fmeasure(preds, mask), R.F1_scores(preds, mask)
        assert [type(st[0]).__name__, type(fm).__name__, type(f1).__name__] == list(g['m%d_types' % c])
        assert np.array(fm).tobytes() == g['m%d_Fmeasure' % c].tobytes()
        assert np.array(f1).tobytes() == g['m%d_F1' % c].tobytes()
    dp = {'a': g['m0_preds'], 'b': g['m1_preds']}
    dm = {'a': g['m0_mask'], 'b': list(g['m1_mask'])}
    fd = R.get_Fmeasure(dp, dm)
    assert type(fd).__name__ == str(g['dict_type']) and np.array(fd).tobytes() == g['dict_Fmeasure'].tobytes()
    # no predicted positives: the float code raises like the reference's, the NumPy-integer code gives its nan
    zp = np.zeros_like(g['m0_preds'])
    assert int(g['zero_F1_raised']) == 1
    with pytest.raises(ZeroDivisionError):
        R.F1_scores(zp, g['m0_mask'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.isnan(R.get_Fmeasure(zp, g['m0_mask'])) and np.isnan(g['zero_Fmeasure'])
    np.testing.assert_array_equal(np.array(R.get_preds_stats(zp, g['m0_mask'])), g['zero_stats'])


def test_numpy_eval_counts_of_the_fake_is_get_preds_stats(golden):
    """The NumPy eval_counts the host tests run on is get_preds_stats, in both forms, accumulating."""
    from nnal_amd import PW_analyze_results as R
    g = golden
    sess = EvalSession()
    preds, mask = g['m1_preds'], g['m1_mask']
    counts = torch.zeros(6, dtype=torch.int64)
    sess.eval_counts(torch.as_tensor(preds.astype(np.int64)), None, torch.as_tensor(mask), counts)
    np.testing.assert_array_equal(counts.numpy().astype(np.float64), g['m1_stats'])
    perm = np.random.RandomState(0).permutation(len(mask))
    seg = torch.full((len(mask),), 9, dtype=torch.uint8)
    sess.eval_counts(torch.as_tensor(preds[perm[:100]].astype(np.int64)), torch.as_tensor(perm[:100]), torch.as_tensor(mask), counts, seg)
    want = np.array(R.get_preds_stats(preds, mask)) + np.array(R.get_preds_stats(preds[perm[:100]], mask[perm[:100]]))
    np.testing.assert_array_equal(counts.numpy().astype(np.float64), want)
    np.testing.assert_array_equal(seg.numpy()[perm[:100]], preds[perm[:100]].astype(np.uint8))
    assert np.all(seg.numpy()[perm[100:]] == 9)


def test_get_queries_numeric_order(tmp_path, golden):
    from nnal_amd import PW_analyze_results as R

    class E(object):
        root_dir = str(tmp_path)
    os.makedirs(str(tmp_path / 'm' / 'queries'))
    for it in (10, 2, 0, 1):
        np.savetxt(str(tmp_path / 'm' / 'queries' / ('%d' % it)), np.array([[it, 0], [it + 100, 1]]), fmt='%d')
    Qs = R.get_queries(E(), 'm')
    assert [int(q[0, 0]) for q in Qs] == [0, 1, 2, 10] and all(q.dtype == np.int32 for q in Qs)


# ------------------------------------------------------------------------------------------------ against the reference's runs
def test_test_eval_against_the_reference_run(tmp_path, golden, predictor):
    g = golden
    gen, calls = predictor
    table, paths = _write_subjects(gen, g, str(tmp_path / 'data'))
    expr = _experiment(str(tmp_path / 'e'), g, paths)
    assert not hasattr(expr, 'test_paths')                      # train subjects only were given
    from nnal_amd import PW_AL
    expr2 = PW_AL.Experiment_MultiImg(str(tmp_path / 'e'), test_paths=paths)
    assert expr2.test_paths == paths                            # the constructor keeps its test_paths argument
    expr = expr2
    expr.test_stats = PW_AL.get_stats(paths)
    np.testing.assert_array_equal(expr.test_stats, g['te_test_stats'])
    sess = EvalSession()
    model = SaltModel()
    model.salt = 2
    F1, preds = expr.test_eval(model, sess)
    _check_calls(g, 'te_call', calls)
    np.testing.assert_array_equal(expr.test_counts, g['te_subject_stats'])          # per-subject P, N, TP, FP, TN, FN
    assert type(F1).__name__ == str(g['te_F1_type']) and np.array(F1).tobytes() == g['te_F1'].tobytes()
    assert preds.dtype == np.float64
    np.testing.assert_array_equal(preds, g['te_preds'])
    assert sess.eval_calls == sum(-(-len(c['inds']) // 50) for c in calls)          # one count launch per chunk
    # explicit indices and labels
    del calls[:]
    F1g, predsg = expr.test_eval(model, sess, [list(g['tg_inds_%d' % i]) for i in range(2)],
                                 [list(g['tg_labels_%d' % i]) for i in range(2)])
    _check_calls(g, 'tg_call', calls)
    assert np.array(F1g).tobytes() == g['tg_F1'].tobytes()
    np.testing.assert_array_equal(predsg, g['tg_preds'])
    # a model without predicted positives: the reference raised, here F1 = 0
    assert int(g['tz_raised']) == 1
    model.salt = int(g['zero_salt'])
    F1z, predsz = expr.test_eval(model, sess)
    assert F1z == 0 and not np.any(predsz)
    assert np.all(expr.test_counts[:, 2:4] == 0) and np.all(expr.test_counts[:, 0] > 0)


def test_eval_MultimgAL_and_resume_against_the_reference_run(tmp_path, golden, predictor):
    from nnal_amd import PW_analyze_results as R
    g = golden
    gen, calls = predictor
    table, paths = _write_subjects(gen, g, str(tmp_path / 'data'))
    expr = _experiment(str(tmp_path / 'e'), g, paths)
    qdir = os.path.join(expr.root_dir, 'entropy', 'queries')
    n_it = int(g['n_iters'])
    for it in range(n_it):
        np.savetxt(os.path.join(qdir, '%d' % it), g['queries_%d' % it], fmt='%d')
    model = SaltModel()
    seen = []

    def factory(e, in_shape, s):
        seen.append(tuple(in_shape))
        return model
    expr.model_factory = factory
    sess = EvalSession()
    scores = R.eval_MultimgAL(expr, 'entropy', paths, sess=sess)
    assert seen == [tuple(int(v) for v in g['ev_create_model_patch_shape'])]
    assert [int(re.search(r'curr_weights_(\d+)', p).group(1)) for p in model.loaded] == list(range(1, n_it + 1))
    _check_calls(g, 'ev_call', calls)
    np.testing.assert_array_equal(scores, g['ev_scores'])
    sfile = os.path.join(expr.root_dir, 'entropy', 'test_scores.txt')
    assert open(sfile).read().encode() == g['ev_scores_text'].tobytes()
    np.testing.assert_array_equal(expr.test_stats, g['ev_last_test_stats'])
    assert expr.test_paths == paths[-1:]
    # resume: the first column kept, the rest recomputed
    with open(sfile, 'wb') as f:
        f.write(g['ev_partial_text'].tobytes())
    del calls[:]
    del model.loaded[:]
    scores2 = R.eval_MultimgAL(expr, 'entropy', paths, start_ind=1, sess=sess)
    _check_calls(g, 'er_call', calls)
    assert len(model.loaded) == n_it - 1
    assert open(sfile).read().encode() == g['er_scores_text'].tobytes() == g['ev_scores_text'].tobytes()
    np.testing.assert_array_equal(scores2, g['ev_scores'])


def test_full_slice_eval_against_the_reference_run(tmp_path, golden, predictor):
    from nnal_amd import PW_analyze_results as R
    g = golden
    gen, calls = predictor
    table, paths = _write_subjects(gen, g, str(tmp_path / 'data'))
    pars = _pars(g)
    model = SaltModel()
    model.salt = 1
    vol = R.full_slice_eval(model, EvalSession(), paths[0][:-1], list(g['fs_slices']), pars['patch_shape'], pars['ntb'], pars['stats'])
    _check_calls(g, 'fs_call', calls)
    assert vol.dtype == np.float64
    np.testing.assert_array_equal(vol, g['fs_volume'])
    # already padded arrays, as batch_eval accepts them
    del calls[:]
    padded = [np.pad(table[p], ((2, 2), (2, 2), (1, 1)), 'constant') for p in sorted(table) if 'sub0_mod' in p]
    vol2 = R.full_slice_eval(model, EvalSession(), padded, list(g['fs_slices']), pars['patch_shape'], pars['ntb'], pars['stats'])
    np.testing.assert_array_equal(vol2, g['fs_volume'])


def test_full_model_eval_with_the_seeded_predictor(tmp_path, golden, predictor):
    """full_model_eval through the (NumPy) count / scatter call: predictions, F1 and the files against the host formulas."""
    from nnal_amd import PW_analyze_results as R, nrrd_io
    g = golden
    gen, calls = predictor
    table, paths = _write_subjects(gen, g, str(tmp_path / 'data'))

    class E(object):
        pars = _pars(g)
    model = SaltModel()
    model.salt = 3
    slices = [0, 2, 4]
    out = str(tmp_path / 'full')
    preds, F1 = R.full_model_eval(E(), model, EvalSession(), paths[0][:-1], paths[0][-1], slices, save_dir=out)
    mask = table[[p for p in table if 'sub0_mask' in p][0]]
    want = np.zeros(mask.shape)
    for z in slices:
        ix = np.ravel_multi_index(np.unravel_index(np.arange(mask.shape[0] * mask.shape[1]), mask.shape[:2]) +
                                  (np.full(mask.shape[0] * mask.shape[1], z),), mask.shape)
        want.reshape(-1)[ix] = gen.predict(0, ix, 3)
    np.testing.assert_array_equal(preds, want)
    assert preds.dtype == np.float64 and np.isnan(mask[:, :, slices]).sum() > 0
    assert F1 == R.F1_scores(want[:, :, slices], mask[:, :, slices])
    segs, _ = nrrd_io.read(os.path.join(out, 'segs.nrrd'))
    assert segs.dtype == np.uint8
    np.testing.assert_array_equal(segs, want.astype(np.uint8))
    assert float(np.loadtxt(os.path.join(out, 'F1_socre.txt'))) == F1
    assert [c['stats'].tolist() for c in calls] == [E.pars['stats']] * len(slices)


# ------------------------------------------------------------------------------------------------ on the oracle-backed fakes
def _oracle_model(seed=61):
    from oracle import netspec
    ld = netspec.net_a()
    return PredModel(ld, (5, 5, 6), netspec.he_init(ld, (5, 5, 6), seed=seed, bias_std=0.3))


def test_device_path_on_the_oracle_fakes_equals_batch_eval(tmp_path, golden, golden_dir, monkeypatch):
    """The real PW_NN._eval_passes (gather + forward on the oracle-backed fakes): eval_counts_device, test_eval and
    full_model_eval equal get_preds_stats / F1 of batch_eval(..., 'prediction') on the same voxels."""
    from nnal_amd import PW_AL, PW_NN, PW_analyze_results as R, patch_utils
    monkeypatch.setattr(patch_utils, 'DeviceVolumes', FakeVolumes)
    g = golden
    gen = _generator(golden_dir)
    table, paths = _write_subjects(gen, g, str(tmp_path / 'data'))
    expr = _experiment(str(tmp_path / 'e'), g, paths)
    expr.test_paths = paths
    expr.test_stats = PW_AL.get_stats(paths)
    sess, model = EvalSession(), _oracle_model()
    inds, labels = PW_AL.gen_multimg_inds(paths, expr.pars['grid_spacing'])
    tP = tTP = tFP = 0
    rows = []
    for i in range(2):
        stats = [[expr.test_stats[i, 2 * j], expr.test_stats[i, 2 * j + 1]] for j in range(2)]
        host = PW_NN.batch_eval(model, sess, paths[i][:-1], inds[i], expr.pars['patch_shape'], expr.pars['ntb'], stats, 'prediction')[0]
        st = R.get_preds_stats(host, np.array(labels[i]))
        assert st == R.eval_counts_device(model, sess, paths[i][:-1], inds[i], expr.pars['patch_shape'], expr.pars['ntb'], stats,
                                          np.array(labels[i]))
        # the volume form: labels looked up in the mask by index
        assert st == R.eval_counts_device(model, sess, paths[i][:-1], inds[i], expr.pars['patch_shape'], expr.pars['ntb'], stats,
                                          table[[p for p in table if 'sub%d_mask' % i in p][0]])
        rows.append(st)
        tP, tTP, tFP = tP + st[0], tTP + st[2], tFP + st[3]
    assert all(min(r[2:]) > 0 for r in rows)                       # both classes predicted, all four outcomes present
    F1, preds = expr.test_eval(model, sess)
    np.testing.assert_array_equal(expr.test_counts, np.array(rows))
    Pr, Rc = tTP / (tTP + tFP), tTP / tP
    assert F1 == 2. / (1 / Pr + 1 / Rc)
    np.testing.assert_array_equal(preds, host)
    with pytest.raises(ValueError):
        R.eval_counts_device(model, sess, paths[0][:-1], inds[0], expr.pars['patch_shape'], 40, stats, np.zeros(3))


# ------------------------------------------------------------------------------------------------ sharded
def _eval_worker(rank, ws, port, q, root, data, golden_dir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    if ws > 1:
        dist.init_process_group('gloo', rank=rank, world_size=ws)
    import nnal_amd  # noqa: F401
    from nnal_amd import PW_AL, PW_analyze_results as R, patch_utils
    patch_utils.DeviceVolumes = FakeVolumes
    g = np.load(os.path.join(golden_dir, 'eval_metrics.npz'))
    gen = _generator(golden_dir)
    calls = []
    _install_predictor(gen, g, calls)
    paths = [[os.path.join(data, os.path.basename(p)) for p in sub] for sub in gen.subjects(int(g['subject_seed']))[1]]
    expr = _experiment(root, g, paths)
    if rank == 0:
        for it in range(int(g['n_iters'])):
            np.savetxt(os.path.join(root, 'entropy', 'queries', '%d' % it), g['queries_%d' % it], fmt='%d')
    if ws > 1:
        dist.barrier()
    model = SaltModel()
    expr.model_factory = lambda e, s, ss: model
    sess = EvalSession()
    scores = R.eval_MultimgAL(expr, 'entropy', paths, sess=sess)
    expr.test_paths, expr.test_stats = paths, PW_AL.get_stats(paths)
    model.salt = 2
    del calls[:]
    F1, preds = expr.test_eval(model, sess)
    q.put((rank, scores, F1, preds, expr.test_counts, sum(len(c['inds']) for c in calls),
           open(os.path.join(root, 'entropy', 'test_scores.txt')).read()))
    if ws > 1:
        dist.barrier()
        dist.destroy_process_group()


def _run_eval(ws, root, data, golden_dir):
    from tests.test_dist_gloo import _free_port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eval_worker, args=(r, ws, port, q, root, data, golden_dir)) for r in range(ws)]
    for p in procs:
        p.start()
    res = {r[0]: r[1:] for r in (q.get(timeout=600) for _ in range(ws))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def test_eval_world2_equals_single_process(tmp_path, golden, golden_dir):
    """Two gloo ranks, each evaluating its block of the concatenated test voxels, the counts summed over the ranks and the last
    subject's predictions assembled from owner-filled entries: F1, predictions, per-subject totals and test_scores.txt equal
    one process - and the reference's run - on both ranks."""
    g = golden
    gen = _generator(golden_dir)
    data = str(tmp_path / 'data')
    _write_subjects(gen, g, data)
    one = _run_eval(1, str(tmp_path / 'e1'), data, golden_dir)
    two = _run_eval(2, str(tmp_path / 'e2'), data, golden_dir)
    s1, F1_1, p1, c1, n1, text1 = one[0]
    assert text1.encode() == g['ev_scores_text'].tobytes() and np.array(F1_1).tobytes() == g['te_F1'].tobytes()
    total = 0
    for r in (0, 1):
        s2, F1_2, p2, c2, n2, text2 = two[r]
        np.testing.assert_array_equal(s1, s2)
        assert F1_1 == F1_2 and text1 == text2
        np.testing.assert_array_equal(p1, p2)
        np.testing.assert_array_equal(c1, c2)
        assert 0 < n2 < n1                                        # each rank walked a part of the voxels
        total += n2
    assert total == n1
