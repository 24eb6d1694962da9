#!/usr/bin/env python3
"""Surface-distance metrics on one MI355X against their NumPy statement, and the time of every device call.

    python tools/gpu_surfdist.py [--dims 256 256 128] [--spacing 1 1 2.5] [--runs 25] [--no-host] [--out profiles/surfdist.json]

The pair is synthetic: two noisy ellipsoids (the second one shifted and a little larger, both with salt noise inside and
outside), spacing (1, 1, 2.5).  Printed: whether alq_surface_mask and alq_edt_sq give the arrays of surfdist.surface_host /
edt_sq_host (equality), the metrics of surfdist.surface_distances with the session beside those of the statement, the device
time of each call and of the whole metric - each run between its own pair of device events, the median over `--runs` runs (at
least 20) after 3 warm-up calls; the whole metric includes its two 32-byte and two 16-byte copies to the host - and, for
scale, the time of scipy.ndimage.distance_transform_edt on the same surface map.  Prints one JSON line last."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import nnal_amd  # noqa: E402,F401
from nnal_amd import device, surfdist  # noqa: E402


def ellipsoid(dims, centre, radii, noise, seed):
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing='ij')
    r2 = sum(((x - c * n) / (r * n)) ** 2 for x, c, r, n in zip(g, centre, radii, dims))
    a = r2 <= 1.
    flip = rng.rand(*dims) < noise
    return (a ^ (flip & (r2 < 1.6))).astype(np.uint8)


def time_call(fn, runs):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument('--spacing', type=float, nargs=3, default=[1., 1., 2.5])
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    runs = max(a.runs, 20)
    dims, sp = tuple(a.dims), tuple(a.spacing)
    seg = ellipsoid(dims, (0.5, 0.5, 0.5), (0.30, 0.25, 0.33), 0.002, 1)
    mask = ellipsoid(dims, (0.52, 0.49, 0.52), (0.32, 0.27, 0.33), 0.002, 2)
    sess = device.DeviceSession(0)
    d_seg, d_mask = sess.to_device(seg, torch.uint8), sess.to_device(mask, torch.uint8)
    out = dict(tool='gpu_surfdist', dims=list(dims), spacing=list(sp), runs=runs, calls=[])

    s_seg, s_mask = sess.surface_mask(d_seg, dims), sess.surface_mask(d_mask, dims)
    e_mask = sess.edt_sq(s_mask, dims, sp)
    st = sess.masked_dist_stats(e_mask, s_seg)
    ranks = surfdist.percentile_ranks(st[0], 95.)[:2]
    dev = surfdist.surface_distances(d_seg, d_mask, sp, sess=sess, shape=dims)
    out['device'] = dev
    print('surface voxels: seg %d, mask %d of %d' % (dev['n_seg'], dev['n_mask'], seg.size), flush=True)
    if not a.no_host:
        t0 = time.perf_counter()
        h_seg, h_mask = surfdist.surface_host(seg), surfdist.surface_host(mask)
        t1 = time.perf_counter()
        h_e = surfdist.edt_sq_host(h_mask, sp)
        t2 = time.perf_counter()
        out['surface_equal'] = bool(np.array_equal(s_seg.cpu().numpy(), h_seg) and np.array_equal(s_mask.cpu().numpy(), h_mask))
        out['edt_equal'] = bool(np.array_equal(e_mask.cpu().numpy(), h_e))
        out['statement_surface_s'], out['statement_edt_s'] = (t1 - t0) / 2, t2 - t1
        print('surface masks equal the statement: %s   edt_sq equals the statement: %s' % (out['surface_equal'], out['edt_equal']), flush=True)
        t0 = time.perf_counter()
        host = surfdist.surface_distances(seg, mask, sp)
        out['statement_metric_s'] = time.perf_counter() - t0
        out['host'] = host
        for k in ('HD', 'HD95', 'ASSD', 'MHD'):
            print('%-5s device %.17g   statement %.17g   diff %.3g' % (k, dev[k], host[k], dev[k] - host[k]), flush=True)
        from scipy import ndimage
        t0 = time.perf_counter()
        sc = ndimage.distance_transform_edt(~h_mask, sampling=sp)
        out['scipy_edt_s'] = time.perf_counter() - t0
        fin = np.isfinite(h_e)
        out['scipy_edt_max_rel_diff'] = float(np.max(np.abs(sc[fin] ** 2 - h_e[fin]) / np.maximum(h_e[fin], 1e-300)))
        print('scipy distance_transform_edt: %.1f ms (squared, max relative difference to the statement %.2g); statement edt %.1f s' % (
            out['scipy_edt_s'] * 1e3, out['scipy_edt_max_rel_diff'], out['statement_edt_s']), flush=True)

    buf = sess.empty(dims, torch.float64)
    smask = sess.empty(dims, torch.uint8)
    calls = (
        ('surface_mask', lambda: sess.surface_mask(d_seg, dims, out=smask)),
        ('edt_sq', lambda: sess.edt_sq(s_mask, dims, sp, out=buf)),
        ('masked_dist_stats (with its 32-byte copy)', lambda: sess.masked_dist_stats(e_mask, s_seg)),
        ('masked_select, 2 ranks (with its 16-byte copy)', lambda: sess.masked_select(e_mask, s_seg, ranks)),
        ('surface_distances, whole metric', lambda: surfdist.surface_distances(d_seg, d_mask, sp, sess=sess, shape=dims)),
    )
    for name, fn in calls:
        med, lo, hi = time_call(fn, runs)
        out['calls'].append(dict(call=name, device_s=med, device_s_min=lo, device_s_max=hi))
        print('%-48s %9.1f us  (min %9.1f, max %9.1f)' % (name, med * 1e6, lo * 1e6, hi * 1e6), flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    sess.close()


if __name__ == '__main__':
    main()
