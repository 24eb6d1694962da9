#!/usr/bin/env python3
"""Expected-gradient-length scoring of B binary candidates on NET-C (32^3 patches): the fused path (alq_grad_sqnorms,
one unit-cotangent pass) against the materialising path (alq_param_grads per-sample rows, then squared sums per
variable on the device), and the matrix-core rate of the weight-norm launches (csrc/gnorm.hip).

    python tools/gpu_egl.py [--B 2000] [--reps 3] [--out FILE]
    python tools/gpu_egl.py --stats kernel_stats.csv [--B 2000] [--reps 3]     # after a rocprofv3 --kernel-trace --stats run

Prints one JSON line.  The share of the fp32-MFMA peak (157.3 TF) comes from the library's own per-class launch timer
(class 'gnorm') and, with --stats, from rocprofv3's kernel statistics of the same run (gnorm_wsq_kernel rows)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import nnal_amd  # noqa: E402,F401
from nnal_amd import NNAL_tools, device, netspec  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--side', type=int, default=32)
    ap.add_argument('--materialise-batch', type=int, default=64)
    ap.add_argument('--skip-materialising', action='store_true')
    ap.add_argument('--stats', default=None, help='rocprofv3 kernel_stats.csv of a run of this tool')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    sess = device.DeviceSession(0)
    ld, sk = netspec.net_c()
    shape = (a.side, a.side, a.side, 1)
    pars = netspec.he_init(ld, shape, seed=21, skips=sk, bias_std=0.05)
    last = list(pars.keys())[-1]
    pars[last][0] = (pars[last][0] * 0.2).astype(np.float32)
    model = device.DeviceModel(sess, ld, shape, sk, max_batch=512)
    model.set_weights(pars)
    B = a.B
    gen = torch.Generator(device=sess.device)
    gen.manual_seed(5)
    x = torch.randn((B, int(np.prod(shape))), generator=gen, dtype=torch.float32, device=sess.device)
    post, _, _ = model.forward_device(x, B)
    p1 = post[1].double().cpu().numpy()

    def fused():
        sq = model.grad_sqnorms_device(x, B, cls=-1).cpu().numpy()
        return NNAL_tools.egl_binary_scores(sq, p1)

    sizes = [int(np.prod(s)) for _, w, b in model.param_shapes for s in (w, b)]
    off = np.cumsum([0] + sizes)

    def materialising():
        mb = a.materialise_batch
        sq = torch.empty((B, len(sizes)), dtype=torch.float64, device=sess.device)
        for s0 in range(0, B, mb):
            s1 = min(B, s0 + mb)
            g, pp, _ = model.param_grads_device(x[s0:s1], s1 - s0, 0, cls=0, want_post=True)
            g = g / pp[1][:, None]                  # u = d log p0 / p1
            for v in range(len(sizes)):
                sq[s0:s1, v] = (g[:, off[v]:off[v + 1]].double() ** 2).sum(dim=1)
            del g
        return NNAL_tools.egl_binary_scores(sq.cpu().numpy(), p1)

    def timed(fn):
        fn()                                                   # warm-up (workspace allocation, code objects)
        ts, res = [], None
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), res

    t_fused, s_fused = timed(fused)
    out = dict(net='NET-C %d^3' % a.side, B=B, fused_s=t_fused, fused_us_per_candidate=t_fused / B * 1e6)
    if not a.skip_materialising:
        t_mat, s_mat = timed(materialising)
        out.update(materialising_s=t_mat, speedup=t_mat / t_fused,
                   score_max_rel_diff=float(np.max(np.abs(s_fused - s_mat) / np.abs(s_mat))),
                   same_top100=bool(np.array_equal(np.argsort(-s_fused, kind='stable')[:100],
                                                   np.argsort(-s_mat, kind='stable')[:100])))
    # the weight-norm launches on the library's launch timer
    sess.prof_reset()
    sess.prof_enable(True)
    model.grad_sqnorms_device(x, B, cls=-1)
    prof = sess.prof_read()
    sess.prof_enable(False)
    gp = prof['gnorm']
    out.update(gnorm_ms=gp['ms'], gnorm_launches=gp['launches'], gnorm_gflop=gp['flops'] / 1e9,
               gnorm_mflop_per_patch=gp['flops'] / B / 1e6,
               gnorm_peak_share=(gp['flops'] / (gp['ms'] * 1e-3) / PEAK_F32_MFMA) if gp['ms'] > 0 else None,
               peak_us_per_patch=gp['flops'] / B / PEAK_F32_MFMA * 1e6)
    if a.stats:
        # rocprofv3 --stats of a run of this tool: the weight-norm kernel's total device time over all its launches; the
        # FLOPs of one scoring are divided by the time of one scoring (total / scorings that ran: warm-up + reps + prof)
        rows = list(csv.DictReader(open(a.stats)))
        ns = sum(float(r['TotalDurationNs']) for r in rows if 'gnorm_wsq_kernel' in r['Name'])
        calls = sum(int(r['Calls']) for r in rows if 'gnorm_wsq_kernel' in r['Name'])
        per_scoring = gp['launches']
        scorings = calls / per_scoring if per_scoring else 0
        out.update(rocprof_gnorm_calls=calls, rocprof_gnorm_ms_per_scoring=ns / 1e6 / scorings if scorings else None,
                   rocprof_gnorm_peak_share=(gp['flops'] * scorings / (ns * 1e-9) / PEAK_F32_MFMA) if ns else None,
                   rocprof_top=[dict(name=r['Name'][:80], calls=int(r['Calls']), ms=float(r['TotalDurationNs']) / 1e6)
                                for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:12]])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    model.close()
    sess.close()


if __name__ == '__main__':
    main()
