#!/usr/bin/env python3
"""Evaluation golden, produced by running the REFERENCE's own Python in the build container:

    python tests/golden/make_golden_eval.py   ->  tests/golden/eval_metrics.npz

Executed from /root/reference, unmodified: `PW_analyze_results.get_preds_stats`, `get_Fmeasure` (array and dict form),
`F1_scores` (PW_analyze_results.py:234-295) on synthetic predictions and NaN-bearing masks; `Experiment_MultiImg.test_eval`
(PW_AL.py:639-677), `PW_analyze_results.eval_MultimgAL` (:802-863, which walks `get_queries`, :29-50) and `full_slice_eval`
(:673-724) on a synthetic two-subject experiment.

Stand-ins bound for that run (as in make_golden_r4.py):
  * `nrrd.read(path)` -> an in-memory table of arrays (pynrrd is absent); skimage / pydensecrf / tensorflow / h5py are the
    inert placeholder modules of make_golden.import_reference(), matplotlib is the installed one (nothing of it is called);
  * `tf.Session` -> a context manager, `NN.create_model` -> an object that remembers the iteration number of the weight file
    `perform_assign_ops` was given;
  * `PW_NN.batch_eval` -> a seeded predictor, a pure function of (subject, voxel index, the model's iteration number), so
    that a sharded evaluation can be compared entry by entry; every call is recorded with the subject, the indices and the
    statistics it was handed;
  * `yaml.load(f)` -> the UnsafeLoader form (PyYAML >= 6 removed the one-argument call).
One entry has a model without predicted positives: the reference's float division raises there (recorded), which is where
this package returns F1 = 0.  The file holds data only: inputs, recorded calls, outputs."""
import os
import re
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SHAPES = [(11, 9, 5), (8, 12, 4)]
PARS = dict(grid_spacing=2, patch_shape=(5, 5, 3), model_name='PW', dropout_rate=1., learning_rate=1e-3, grad_layers=[],
            train_layers=[], optimizer_name='SGD', init_weights_path='init', k=4, B=10, lambda_=0., ntb=40, b=4, epochs=1,
            stats=[[0.1, 1.2], [0.3, 2.1]])
N_ITERS = 3
ZERO_SALT = -1          # the model that predicts class 0 everywhere


def subjects(seed=4300):
    rs = np.random.RandomState(seed)
    table, paths = {}, []
    for s_, shp in enumerate(SHAPES):
        sub = []
        for j in range(2):
            p = '/synthetic/sub%d_mod%d.nrrd' % (s_, j)
            table[p] = rs.randn(*shp) * (1. + j) + 0.3 * s_
            sub.append(p)
        mask = rs.randint(0, 2, size=shp).astype(np.float64)
        mask[rs.rand(*shp) < 0.15] = np.nan
        p = '/synthetic/sub%d_mask.nrrd' % s_
        table[p] = mask
        sub.append(p)
        paths.append(sub)
    return table, paths


def predict(subject, inds, salt):
    """The seeded predictor: class of voxel `ind` of `subject` under the model of iteration `salt`."""
    inds = np.asarray(inds, dtype=np.int64)
    if salt == ZERO_SALT:
        return np.zeros(len(inds))
    return (((inds * 7919 + salt * 104729 + subject * 13 + 5) % 11) < 5).astype(np.float64)


def subject_of(path):
    return int(re.search(r'sub(\d+)_', os.path.basename(path)).group(1))


def metric_cases(seed=4301):
    rs = np.random.RandomState(seed)
    cases = []
    for c, (n, vals) in enumerate([(400, (0., 1., np.nan)), (257, (0., 1., 2., -1., np.nan)), ((6, 7, 3), (0., 1., np.nan))]):
        mask = rs.choice(np.array(vals), size=n)
        preds = rs.randint(0, 2, size=n).astype(np.float64)
        if c == 1:
            preds[rs.rand(n) < 0.2] = 2.          # a third class index counts as a positive prediction (preds > 0)
        cases.append((preds, mask))
    return cases


def main():
    make_golden.import_reference()
    import PW_AL
    import PW_analyze_results as R
    table, paths = subjects()
    out = dict(shapes=np.array(SHAPES), subject_seed=np.array(4300), n_iters=np.array(N_ITERS), zero_salt=np.array(ZERO_SALT))
    for k, v in PARS.items():
        if isinstance(v, (int, float, tuple)):
            out['par_' + k] = np.array(v)
    out['par_stats'] = np.array(PARS['stats'])

    # ---- the metric functions
    cases = metric_cases()
    out['n_metric_cases'] = np.array(len(cases))
    for c, (preds, mask) in enumerate(cases):
        st = R.get_preds_stats(preds, mask)
        assert all(type(v) is float for v in st)
        P, N, TP, FP, TN, FN = st
        assert TP > 0 and FP > 0 and TN > 0 and FN > 0 and np.isnan(mask).sum() > 0
        fm, f1 = R.get_Fmeasure(preds, mask), R.F1_scores(preds, mask)
        out['m%d_preds' % c], out['m%d_mask' % c] = preds, mask
        out['m%d_stats' % c] = np.array(st)
        out['m%d_Fmeasure' % c], out['m%d_F1' % c] = np.array(fm), np.array(f1)
        out['m%d_types' % c] = np.array([type(st[0]).__name__, type(fm).__name__, type(f1).__name__])
    dp = {'a': cases[0][0], 'b': cases[1][0]}
    dm = {'a': cases[0][1], 'b': list(cases[1][1])}
    fd = R.get_Fmeasure(dp, dm)
    out['dict_Fmeasure'], out['dict_type'] = np.array(fd), np.array(type(fd).__name__)
    # no predicted positives: F1_scores raises, get_Fmeasure (NumPy integers) gives nan
    zp = np.zeros_like(cases[0][0])
    try:
        R.F1_scores(zp, cases[0][1])
        raised = 0
    except ZeroDivisionError:
        raised = 1
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out['zero_Fmeasure'] = np.array(R.get_Fmeasure(zp, cases[0][1]))
    out['zero_stats'] = np.array(R.get_preds_stats(zp, cases[0][1]))
    out['zero_F1_raised'] = np.array(raised)
    assert raised == 1

    # ---- test_eval / eval_MultimgAL / full_slice_eval
    PW_AL.nrrd.read = lambda p: (table[p], None)
    R.nrrd.read = lambda p: (table[p], None)
    import yaml
    _yload = yaml.load
    PW_AL.yaml.load = lambda f, Loader=None: _yload(f, Loader=Loader or yaml.UnsafeLoader)

    class _Graph(object):
        def finalize(self):
            pass

    class _Sess(object):
        graph = _Graph()

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    class _TF(object):
        @staticmethod
        def Session():
            return _Sess()

    class _Model(object):
        salt = 0
        loaded = None

        def add_assign_ops(self):
            pass

        def initialize_graph(self, sess):
            pass

        def perform_assign_ops(self, path, sess):
            self.loaded = path
            self.salt = int(re.search(r'curr_weights_(\d+)', path).group(1))
    R.tf = _TF
    made = []

    def create_model(*a, **k):
        made.append((a, k))
        return _Model()
    R.NN.create_model = create_model
    calls = []

    def fake_batch_eval(model, sess, img_paths, inds, patch_shape, ntb, stats, varnames, *a, **k):
        assert varnames == 'prediction' and not a and not k
        calls.append(dict(subject=subject_of(img_paths[0]), n_paths=len(img_paths), inds=np.array(inds, dtype=np.int64),
                          stats=np.array(stats, dtype=np.float64), patch_shape=np.array(patch_shape), ntb=ntb, salt=model.salt))
        return [predict(subject_of(img_paths[0]), inds, model.salt)]
    R.PW_NN.batch_eval = fake_batch_eval
    assert PW_AL.PW_NN is R.PW_NN

    def dump_calls(prefix, lst):
        out[prefix + '_n'] = np.array(len(lst))
        for c, d in enumerate(lst):
            out['%s_%d_subject' % (prefix, c)] = np.array(d['subject'])
            out['%s_%d_inds' % (prefix, c)] = d['inds']
            out['%s_%d_stats' % (prefix, c)] = d['stats']
            out['%s_%d_salt' % (prefix, c)] = np.array(d['salt'])
            assert d['n_paths'] == 2 and tuple(d['patch_shape']) == PARS['patch_shape'] and d['ntb'] == PARS['ntb']

    root = tempfile.mkdtemp(prefix='eval_golden_')
    expr = PW_AL.Experiment_MultiImg(root, PARS, paths)
    expr.add_method('entropy')
    # (a) test_eval over both subjects at once, stats = the reference's get_stats of the test subjects
    expr.test_paths = paths
    expr.test_stats = PW_AL.get_stats(paths)
    out['te_test_stats'] = np.asarray(expr.test_stats)
    model = _Model()
    model.salt = 2
    del calls[:]
    F1, test_preds = expr.test_eval(model, None)
    dump_calls('te_call', calls)
    out['te_F1'], out['te_F1_type'], out['te_preds'] = np.array(F1), np.array(type(F1).__name__), np.asarray(test_preds)
    inds, labels = PW_AL.gen_multimg_inds(paths, PARS['grid_spacing'])
    tot = []
    for i in range(2):
        assert np.array_equal(calls[i]['inds'], np.array(inds[i]))
        st = R.get_preds_stats(predict(i, inds[i], 2), np.array(labels[i]))
        assert min(st[2:]) > 0
        assert np.isnan(table[paths[i][-1]][::2, ::2, :]).sum() > 0        # NaN labels were dropped from this subject's grid
        assert len(inds[i]) < table[paths[i][-1]][::2, ::2, :].size
        tot.append(st)
        out['te_labels_%d' % i] = np.array(labels[i])
    out['te_subject_stats'] = np.array(tot)
    # (b) the same with explicit indices / labels (a subset, in another order)
    rs = np.random.RandomState(9)
    sub_i = [rs.permutation(len(inds[i]))[:40 + 7 * i] for i in range(2)]
    g_inds = [list(np.array(inds[i])[sub_i[i]]) for i in range(2)]
    g_labels = [list(np.array(labels[i])[sub_i[i]]) for i in range(2)]
    del calls[:]
    F1g, predsg = expr.test_eval(model, None, g_inds, g_labels)
    dump_calls('tg_call', calls)
    out['tg_F1'], out['tg_preds'] = np.array(F1g), np.asarray(predsg)
    for i in range(2):
        out['tg_inds_%d' % i], out['tg_labels_%d' % i] = np.array(g_inds[i]), np.array(g_labels[i])
    # (c) a model without predicted positives: the reference raises
    zm = _Model()
    zm.salt = ZERO_SALT
    try:
        expr.test_eval(zm, None)
        raised = 0
    except ZeroDivisionError:
        raised = 1
    assert raised == 1
    out['tz_raised'] = np.array(raised)
    # (d) eval_MultimgAL: N_ITERS iterations' weights, both subjects as test images
    qdir = os.path.join(root, 'entropy', 'queries')
    qrs = np.random.RandomState(11)
    for it in (2, 0, 1):                                            # (created out of order: get_queries sorts by number)
        q = np.stack([qrs.randint(0, 300, size=4), qrs.randint(0, 2, size=4)], axis=1)
        np.savetxt(os.path.join(qdir, '%d' % it), q, fmt='%d')
        out['queries_%d' % it] = q
    Qs = R.get_queries(expr, 'entropy')
    for it in range(N_ITERS):
        assert np.array_equal(Qs[it], out['queries_%d' % it]) and Qs[it].dtype == np.int32
    del calls[:]
    assert R.eval_MultimgAL(expr, 'entropy', paths) is None
    dump_calls('ev_call', calls)
    sfile = os.path.join(root, 'entropy', 'test_scores.txt')
    with open(sfile) as f:
        out['ev_scores_text'] = np.frombuffer(f.read().encode(), dtype=np.uint8)
    scores = np.loadtxt(sfile)
    out['ev_scores'] = scores
    assert scores.shape == (2, N_ITERS) and np.all(scores > 0) and len(np.unique(scores)) == scores.size
    out['ev_last_test_stats'] = np.asarray(expr.test_stats)
    out['ev_create_model_patch_shape'] = np.array(made[-1][0][-1])
    # (e) resume: the first column kept, the others lost
    partial = scores.copy()
    partial[:, 1:] = -1.
    np.savetxt(sfile, partial)
    with open(sfile) as f:
        out['ev_partial_text'] = np.frombuffer(f.read().encode(), dtype=np.uint8)
    del calls[:]
    R.eval_MultimgAL(expr, 'entropy', paths, start_ind=1)
    dump_calls('er_call', calls)
    with open(sfile) as f:
        out['er_scores_text'] = np.frombuffer(f.read().encode(), dtype=np.uint8)
    assert np.array_equal(out['er_scores_text'], out['ev_scores_text'])
    # (f) full_slice_eval on subject 0
    model.salt = 1
    del calls[:]
    vol = R.full_slice_eval(model, None, paths[0][:-1], [3, 0], PARS['patch_shape'], PARS['ntb'], PARS['stats'])
    dump_calls('fs_call', calls)
    out['fs_slices'], out['fs_volume'] = np.array([3, 0]), vol
    assert vol.shape == SHAPES[0] and vol[:, :, 3].sum() > 0 and vol[:, :, 1].sum() == 0
    np.savez_compressed(os.path.join(HERE, 'eval_metrics.npz'), **out)
    print('eval_metrics: scores', scores.tolist(), 'test_eval F1', F1, 'subject totals', tot)


if __name__ == '__main__':
    main()
