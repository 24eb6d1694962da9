#!/usr/bin/env python3
"""Times the post-processing calls of csrc/ccl.hip on one MI355X against scipy.ndimage on the same host.

    python tools/gpu_postproc.py [--dims 256 256 128] [--runs 25] [--out profiles/postproc_256x256x128.json]

For foreground densities 0.05, 0.2 and 0.35 (rand < d, seeded): the device time of one alq_cc_label (26 neighbours),
alq_cc_keep_largest (26, skip_origin) and alq_fill_holes call - each run between its own pair of device events, the median
over `--runs` runs (at least 20) after 3 warm-up calls - beside the time of the scipy.ndimage statement of the same step
(regions.cc_label_host / keep_largest_host / fill_holes_host, timed once), after checking that both give the same array.
Also the bytes every launch of a call has to move per voxel, from the algorithm (p = share of selected voxels; the merge
launch's parent[] traffic depends on the data and is not in the table), their sum over the achievable HBM rate as the
streaming bound of the call, and the measured time as a multiple of that bound.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import nnal_amd  # noqa: E402,F401
from nnal_amd import device, regions  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def launch_bytes(call, p):
    """Bytes per voxel of every launch of a call; p = share of selected voxels (fill holes: of zero voxels)."""
    init = ('init', 1 + 4 + (0 if call == 'cc_label' else 4))                       # seg in; parent (and size / flag) out
    merge = ('merge', 1)                                                             # seg in (neighbour bytes from cache) + atomics on parent[]
    compress = ('compress', 4 + 4 * p)                                               # parent in; root out for the selected voxels
    if call == 'cc_label':
        return [init, merge, compress]
    if call == 'cc_keep_largest':
        return [init, merge, compress, ('winner', 4), ('select', 4 + 1)]
    return [init, merge, compress, ('fill', 1 + 4 + 4 * p + 1)]


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
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    runs = max(a.runs, 20)
    dims = tuple(a.dims)
    nvox = int(np.prod(dims))
    sess = device.DeviceSession(0)
    sess.bind_stream()
    L, ctx = sess.lib, sess.ctx
    cd = (C.c_int64 * 3)(*dims)
    work = sess.empty((int(L.alq_cc_work_bytes(cd)),), torch.uint8)
    info = sess.empty((4,), torch.int64)
    labels = sess.empty(dims, torch.int32)
    mask = sess.empty(dims, torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    out = dict(tool='gpu_postproc', dims=list(dims), runs=runs, hbm_achievable_Bps=HBM_ACHIEVABLE, cases=[])
    for d in (0.05, 0.2, 0.35):
        seg = (np.random.RandomState(int(1000 * d)).rand(*dims) < d).astype(np.uint8)
        seg.reshape(-1)[0] = 0
        d_seg = sess.to_device(seg, torch.uint8)

        def rc0(rc):
            assert rc == 0, L.alq_last_error()
        calls = (
            ('cc_label', d, lambda: rc0(L.alq_cc_label(ctx, p(d_seg), cd, 26, 0, p(labels))),
             lambda: labels.cpu().numpy(), lambda: regions.cc_label_host(seg, 26)),
            ('cc_keep_largest', d, lambda: rc0(L.alq_cc_keep_largest(ctx, p(d_seg), cd, 26, 1, p(mask), p(info), p(work))),
             lambda: mask.cpu().numpy(), lambda: regions.keep_largest_host(seg, 26, True)),
            ('fill_holes', 1. - d, lambda: rc0(L.alq_fill_holes(ctx, p(d_seg), cd, p(mask), p(info), p(work))),
             lambda: mask.cpu().numpy(), lambda: regions.fill_holes_host(seg)),
        )
        for name, share, fn, fetch, host in calls:
            fn()
            got = fetch()
            case = dict(call=name, density=d)
            if not a.no_host:
                t0 = time.perf_counter()
                want = host()
                case['scipy_s'] = time.perf_counter() - t0
                case['equals_host'] = bool(np.array_equal(got, want))
            med, lo, hi = time_call(fn, runs)
            table = launch_bytes(name, share)
            bound = sum(b for _, b in table) * nvox / HBM_ACHIEVABLE
            case.update(device_s=med, device_s_min=lo, device_s_max=hi, bytes_per_voxel={k: v for k, v in table},
                        bytes_per_voxel_sum=sum(b for _, b in table), streaming_bound_s=bound, times_the_bound=med / bound)
            if 'scipy_s' in case:
                case['speedup'] = case['scipy_s'] / med
            out['cases'].append(case)
            print('%-16s d=%.2f  device %9.1f us  (min %9.1f, max %9.1f)  bound %6.1f us  scipy %s  equal %s' % (
                name, d, med * 1e6, lo * 1e6, hi * 1e6, bound * 1e6,
                '%8.1f ms' % (case['scipy_s'] * 1e3) if 'scipy_s' in case else '-', case.get('equals_host', '-')), flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    sess.close()


if __name__ == '__main__':
    main()
