#!/usr/bin/env python3
"""Test-set evaluation on the device: a synthetic two-subject experiment (128 x 128 x 6 volumes, two modalities, NaN-bearing
masks; patch (25, 25, 1) x 2 modalities, the reference's patch-wise 'PW' net), a few iterations of the entropy loop
(Experiment_MultiImg.run_method), then the learning curve (PW_analyze_results.eval_MultimgAL -> test_scores.txt) and one
dense evaluation (full_model_eval: every voxel of --slices slices of one test subject).

    python tools/gpu_eval.py [--iters 3] [--slices 5] [--reps 7] [--out FILE]

Prints one JSON line: the score matrix; the voxels/s of the dense slice pass on the two arms - the device path (predictions
counted and scattered in HBM by alq_eval_counts, 48 bytes + one uint8 volume back) and the host route (PW_NN.batch_eval(...,
'prediction') per slice, then get_preds_stats on the host: what a caller had before) -, that both arms agree, and the 'eval'
profile class time and its share of the device arm."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import nnal_amd  # noqa: E402,F401
from nnal_amd import NN, PW_AL, PW_NN, PW_analyze_results, device, nrrd_io  # noqa: E402

DIMS = (128, 128, 6)


def subjects(root, tag, seed):
    rs = np.random.RandomState(seed)
    paths = []
    for s_ in range(2):
        sub = []
        # a smooth field the label is cut from, so that a patch says something about its centre voxel
        x, y, z = np.meshgrid(np.arange(DIMS[0]), np.arange(DIMS[1]), np.arange(DIMS[2]), indexing='ij')
        base = np.sin(x / (7. + s_)) + np.cos(y / (9. - s_)) + .3 * np.sin(z + s_) + .3 * rs.randn(*DIMS)
        for j in range(2):
            p = os.path.join(root, '%s%d_mod%d.nrrd' % (tag, s_, j))
            nrrd_io.write(p, base * (1. + .3 * j) + .2 * rs.randn(*DIMS) + .3 * s_)
            sub.append(p)
        mask = (base > 0.2).astype(np.float64)
        mask[rs.rand(*DIMS) < .05] = np.nan
        p = os.path.join(root, '%s%d_mask.nrrd' % (tag, s_))
        nrrd_io.write(p, mask)
        sub.append(p)
        paths.append(sub)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--slices', type=int, default=5)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    sess = device.DeviceSession(0)
    tmp = tempfile.mkdtemp(prefix='gpu_eval_')
    try:
        train = subjects(tmp, 'train', 2001)
        test = subjects(tmp, 'test', 2002)
        k = 64
        pars = dict(grid_spacing=8, patch_shape=(25, 25, 1), model_name='PW', dropout_rate=1., learning_rate=1e-2, grad_layers=[],
                    train_layers=[], optimizer_name='SGD', init_weights_path='init', k=k, B=256, lambda_=0., ntb=8192, b=32,
                    epochs=1)
        expr = PW_AL.Experiment_MultiImg(os.path.join(tmp, 'expr'), pars, train, test_paths=test)
        expr.model_factory = lambda e, in_shape, s: NN.create_PW1(e.nclass, 1., e.pars['learning_rate'], 'SGD', in_shape, sess=s,
                                                                  max_batch=8192)
        expr.add_method('entropy')
        np.random.seed(3)
        t0 = time.perf_counter()
        log = expr.run_method('entropy', a.iters * k, sess=sess)
        t_loop = time.perf_counter() - t0
        model = expr.model
        t0 = time.perf_counter()
        model.close()
        scores = PW_analyze_results.eval_MultimgAL(expr, 'entropy', test, sess=sess)
        t_curve = time.perf_counter() - t0
        out = dict(tool='gpu_eval', net='PW (NET-B)', patch=[25, 25, 2], volume=list(DIMS), iterations=len(log),
                   queries_per_iteration=k, loop_s=t_loop, learning_curve_s=t_curve, test_scores=scores.tolist(),
                   test_scores_file=open(os.path.join(expr.root_dir, 'entropy', 'test_scores.txt')).read())

        # the dense pass: every voxel of `slices` slices of test subject 0, the last iteration's weights
        model = expr.model_factory(expr, (25, 25, 2), sess)
        model.perform_assign_ops(PW_AL.LoopState(os.path.join(expr.root_dir, 'entropy')).weights_path(len(log)), sess)
        mask = nrrd_io.read(test[0][-1])[0]
        vol = [nrrd_io.read(p)[0] for p in test[0][:-1]]
        expr.pars['stats'] = [[float(v[~np.isnan(mask)].mean()), float(v[~np.isnan(mask)].std())] for v in vol]
        slices = list(range(1, 1 + a.slices))
        nvox = DIMS[0] * DIMS[1] * len(slices)
        padded = [np.pad(v, ((12, 12), (12, 12), (0, 0)), 'constant') for v in vol]

        def arm_device():
            torch.cuda.synchronize()
            t = time.perf_counter()
            preds, F1 = PW_analyze_results.full_model_eval(expr, model, sess, padded, mask, slices)
            torch.cuda.synchronize()
            return time.perf_counter() - t, preds, F1

        def arm_host():
            torch.cuda.synchronize()
            t = time.perf_counter()
            preds = PW_analyze_results.full_slice_eval(model, sess, padded, slices, expr.pars['patch_shape'], expr.pars['ntb'],
                                                       expr.pars['stats'])
            P, N, TP, FP, TN, FN = PW_analyze_results.get_preds_stats(preds[:, :, slices], mask[:, :, slices])
            F1 = PW_analyze_results.F1_scores(preds[:, :, slices], mask[:, :, slices]) if TP > 0 else 0
            torch.cuda.synchronize()
            return time.perf_counter() - t, preds, F1

        arm_device(), arm_host()                               # warm-up
        td, th = [], []
        for r in range(a.reps):                                # interleaved, order alternating
            for arm in ((arm_device, arm_host) if r % 2 == 0 else (arm_host, arm_device)):
                dt, preds, F1 = arm()
                (td if arm is arm_device else th).append(dt)
                if arm is arm_device:
                    pd, fd = preds, F1
                else:
                    ph, fh = preds, F1
        out.update(dense_voxels=nvox, dense_F1=fd, arms_agree=bool(np.array_equal(pd, ph) and fd == fh),
                   device_path_s=td, host_route_s=th, device_path_voxels_per_s=nvox / min(td),
                   host_route_voxels_per_s=nvox / min(th), host_over_device=min(th) / min(td))
        sess.prof_reset()
        sess.prof_enable(True)
        dt, _, _ = arm_device()
        prof = sess.prof_read()
        sess.prof_enable(False)
        ev = prof['eval']
        out['prof'] = dict(pass_s=dt, eval_ms=ev['ms'], eval_launches=ev['launches'], eval_share=ev['ms'] / 1e3 / dt,
                           all_classes_ms={c: v['ms'] for c, v in prof.items() if v['launches']})
        model.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    sess.close()


if __name__ == '__main__':
    main()
