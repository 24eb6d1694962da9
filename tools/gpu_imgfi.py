#!/usr/bin/env python3
"""The A matrices of the image-level multi-class Fisher query (NNAL.fi_A_matrices) on the PW net with a 10-class head
(25 x 25 x 2 inputs, 36 M parameters), 64 candidates whose posteriors keep 10 classes: the fused arm (alq_class_layer_sums:
class slots, layer sums from the backward sweep, csrc/lsum.hip) against the rows arm (alq_param_grads per-sample rows for
every class + alq_shrink_sum), both in one process, interleaved, best of several.

    python tools/gpu_imgfi.py [--B 64] [--reps 5] [--out profiles/imgfi_pw10_B64.json]
    python tools/gpu_imgfi.py --only fused --reps 3      # the program of a rocprofv3 --kernel-trace --stats run
    python tools/gpu_imgfi.py --stats kernel_stats.csv --stats-calls N [--out FILE]    # fold that run's statistics in (no GPU work)

Prints one JSON line.  With --stats: the fused arm's kernels by traced time and what the class sweep (lsum_sweep_kernel)
reaches of the HBM rate, from the bytes it moves (cotangent read + written, activation read for the mask, field read)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def sweep_bytes(model, B, J):
    """Bytes the spatial class sweeps of one scoring move: per layer and slot the cotangent once in and (ReLU layers) once
    out, the activation for the mask, 8 bytes of field per voxel; fc layers likewise on their [B, out] rows."""
    from nnal_amd import _lib
    total = 0
    spatial = list(model.in_shape[:-1])
    for d in model.layers:
        if d['type'] == _lib.ALQ_POOL:
            spatial = [-(-a // s) for a, s in zip(spatial, d['s'][-len(spatial):])]
            continue
        relu = 1 if d['relu'] else 0
        if d['type'] == _lib.ALQ_FC:
            total += B * J * (d['cout'] * 4 * (1 + 2 * relu) + 8)
            continue
        if d['type'] == _lib.ALQ_CONVT:
            spatial = [a * s for a, s in zip(spatial, d['s'][-len(spatial):])]
        vox = int(np.prod(spatial))
        total += B * J * vox * (d['cout'] * 4 * (1 + 2 * relu) + 8)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', choices=['both', 'fused', 'rows'], default='both')
    ap.add_argument('--stats', default=None, help='rocprofv3 kernel_stats.csv of a --only fused run of this tool')
    ap.add_argument('--stats-calls', type=int, default=0, help='scorings that run made (warm-up + reps)')
    ap.add_argument('--merge', default=None, help='JSON file of a timing run to extend with --stats')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch  # noqa: F401
    import nnal_amd  # noqa: F401
    from nnal_amd import NN, NNAL, device

    nclass, shape, B = 10, (25, 25, 2), a.B
    out = {}
    if a.merge:
        out = json.loads(open(a.merge).read())
    if a.stats:
        rows = list(csv.DictReader(open(a.stats)))
        calls = max(a.stats_calls, 1)
        top = [dict(name=r['Name'][:70], calls=int(r['Calls']), ms_per_scoring=float(r['TotalDurationNs']) / 1e6 / calls)
               for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:14]]
        ns = sum(float(r['TotalDurationNs']) for r in rows if 'lsum_sweep' in r['Name'])
        nf = sum(float(r['TotalDurationNs']) for r in rows if 'lsum_field' in r['Name'])
        tot = sum(float(r['TotalDurationNs']) for r in rows)
        out.update(rocprof_scorings=calls, rocprof_top=top, rocprof_total_ms_per_scoring=tot / 1e6 / calls,
                   rocprof_sweep_ms_per_scoring=ns / 1e6 / calls, rocprof_field_ms_per_scoring=nf / 1e6 / calls)
        if ns and 'sweep_bytes' in out:
            rate = out['sweep_bytes'] / (ns / 1e9 / calls)
            out.update(sweep_bytes_per_s=rate, sweep_hbm_peak_share=rate / HBM_PEAK)
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, 'w') as f:
                f.write(line + '\n')
        return

    sess = device.DeviceSession(0)
    ld = NN.pw1_layer_dict(nclass)
    model = device.DeviceModel(sess, ld, shape, (), max_batch=B)
    from nnal_amd import netspec
    pars = netspec.he_init(ld, shape, seed=31, bias_std=0.05)
    last = list(pars.keys())[-1]
    pars[last][0] = (pars[last][0] * 0.5).astype(np.float32)          # moderate posteriors: every class stays above 1e-6
    model.set_weights(pars)
    x = np.random.RandomState(6).randn(B, *shape).astype(np.float32)
    post = model.forward(x)['posteriors'].astype(np.float64)
    W = np.zeros((B, nclass))
    diag = np.zeros(B)
    for i in range(B):
        W[i], kept = NNAL.class_weights(post[:, i].copy())
        diag[i] = kept * 1e-5
    J = int((W != 0).sum(axis=1).max())
    assert J == 10 and int((W != 0).sum(axis=1).min()) == 10, 'the posteriors must keep 10 classes'

    arms = {'fused': lambda: model.fisher_classes(x, W, diag, fused=True),
            'rows': lambda: model.fisher_classes(x, W, diag, fused=False)}
    names = ['fused', 'rows'] if a.only == 'both' else [a.only]
    res, best, info = {}, {k: float('inf') for k in names}, {}
    for k in names:                                                   # warm-up (workspaces, code objects)
        res[k] = arms[k]()
        info[k] = int(sess.lib.alq_model_engine_info(model._m, 15))
    for _ in range(a.reps):                                           # interleaved
        for k in names:
            sess.synchronize()
            t0 = time.perf_counter()
            res[k] = arms[k]()
            sess.synchronize()
            best[k] = min(best[k], time.perf_counter() - t0)
    out.update(net='PW 25x25x2, %d classes' % nclass, params=int(model.num_params), B=B, J=J, reps=a.reps,
               scorings_per_arm=a.reps + 1, sweep_bytes=sweep_bytes(model, B, J))
    for k in names:
        out['%s_s' % k] = best[k]
        out['engine_info_15_%s' % k] = info[k]
    if a.only == 'both':
        out.update(rows_over_fused=best['rows'] / best['fused'],
                   A_max_diff_over_max=float(np.abs(res['fused'] - res['rows']).max() / np.abs(res['rows']).max()))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    model.close()
    sess.close()


if __name__ == '__main__':
    main()
