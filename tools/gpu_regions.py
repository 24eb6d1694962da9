#!/usr/bin/env python3
"""Times the whole-map local-variance launch (alq_local_var2d, csrc/region.hip) on one MI355X against the host route.

    python tools/gpu_regions.py [--dims 256 256 128] [--out profiles/regions.json]

For d = 5, 12 and 25 and fp32 / fp64 volumes: the median over 5 runs (after a warm-up) of the time per launch, a run being
`--iters` launches between two device events; the bytes the algorithm needs (4 or 8 read + 8 written per voxel) over that time
as a fraction of the achievable HBM rate (6.3 TB/s, the figure of DESIGN.md's tables).  The launches of a run rotate over
`--rotate` volume / map pairs, so that the footprint between two uses of a line (rotate x 12 or 16 bytes per voxel) exceeds the
256 MiB Infinity Cache and the reads come from HBM.  Also: the same launch for other row tiles per lane (ALQ_LVAR_ROWS), the
indexed form at 100,000 voxels, and the host route - patch_utils.get_vars_2d of the reference restated with scipy, slice by
slice over the same volume - timed once per d.  Every timed map is compared with the host restatement first.
Prints one JSON line."""
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
from nnal_amd import device, patch_utils, regions  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def scipy_route(vol, d):
    """get_vars_2d (patch_utils.py:794-826) per slice, as get_HV_inds calls it (PW_NNAL.py:652-656)."""
    from scipy.signal import convolve2d
    out = np.zeros(vol.shape)
    kernel = np.ones((d, d))
    for z in range(vol.shape[2]):
        img = np.uint64(vol[:, :, z])
        ex = convolve2d(img, kernel, 'same') / float(d ** 2)
        ex2 = convolve2d(img ** 2, kernel, 'same') / float(d ** 2)
        out[:, :, z] = ex2 - ex ** 2
    return out


def time_launches(fn, iters, runs=5):
    fn(0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return float(np.median(ts)), [float(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rotate', type=int, default=6)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dims = tuple(a.dims)
    nvox = int(np.prod(dims))
    sess = device.DeviceSession(0)
    rs = np.random.RandomState(77)
    vols = [(rs.randint(0, 4096, size=dims) + rs.rand(*dims)) for _ in range(2)]
    out = dict(tool='gpu_regions', dims=list(dims), iters=a.iters, rotate=a.rotate, hbm_achievable_Bps=HBM_ACHIEVABLE, cases=[], host=[])
    host_maps = {}
    for d in (5, 12, 25):
        if a.no_host:
            host_maps[d] = regions.local_var2d_host(vols[0], d)
            continue
        t0 = time.perf_counter()
        host_maps[d] = scipy_route(vols[0], d)
        out['host'].append(dict(d=d, scipy_s=time.perf_counter() - t0))
    for dtype, name, rd in ((np.float32, 'fp32', 4), (np.float64, 'fp64', 8)):
        # rotate distinct device copies (two distinct contents; the values do not change the work)
        dvs = [patch_utils.DeviceVolumes(sess, [vols[i % 2].astype(dtype)]) for i in range(a.rotate)]
        maps = [sess.empty(dims, torch.float64) for _ in range(a.rotate)]
        pd, r0 = (C.c_int64 * 3)(*dims), (C.c_int32 * 3)(0, 0, 0)
        for d in (5, 12, 25):
            got = dvs[0].local_var(d).cpu().numpy()             # also the precondition check, once
            want = host_maps[d] if dtype == np.float64 else regions.local_var2d_host(vols[0].astype(dtype), d)
            equal = bool(np.array_equal(got, want))

            def launch(i, d=d):
                k = i % a.rotate
                rc = sess.lib.alq_local_var2d(sess.ctx, C.c_void_p(dvs[k].tensors[0].data_ptr()), 1 if rd == 8 else 0, pd, r0, d,
                                              None, 0, C.c_void_p(maps[k].data_ptr()))
                assert rc == 0
            sess.bind_stream()
            med, ts = time_launches(launch, a.iters)
            nbytes = nvox * (rd + 8)
            case = dict(dtype=name, d=d, s_per_launch=med, runs=ts, bytes=nbytes, Bps=nbytes / med, frac_of_hbm=nbytes / med / HBM_ACHIEVABLE,
                        equals_host=equal)
            if d == 12:
                sweep = {}
                for rows in (4, 8, 16, 32, 64):
                    os.environ['ALQ_LVAR_ROWS'] = str(rows)
                    sweep[str(rows)] = time_launches(launch, a.iters, runs=3)[0]
                os.environ.pop('ALQ_LVAR_ROWS')
                case['s_per_launch_by_rows_per_lane'] = sweep
            out['cases'].append(case)
        # indexed form: 100,000 random voxels, d = 12
        inds = sess.to_device(rs.randint(0, nvox, size=100000).astype(np.int64), torch.int64)
        res = sess.empty((100000,), torch.float64)

        def launch_inds(i):
            rc = sess.lib.alq_local_var2d(sess.ctx, C.c_void_p(dvs[i % a.rotate].tensors[0].data_ptr()), 1 if rd == 8 else 0, pd, r0, 12,
                                          C.c_void_p(inds.data_ptr()), 100000, C.c_void_p(res.data_ptr()))
            assert rc == 0
        out['cases'].append(dict(dtype=name, d=12, indexed=100000, s_per_launch=time_launches(launch_inds, a.iters)[0]))
        dvs = maps = None
    for h in out['host']:
        dev = [c for c in out['cases'] if c.get('d') == h['d'] and c['dtype'] == 'fp64' and 'indexed' not in c][0]
        h['speedup_fp64'] = h['scipy_s'] / dev['s_per_launch']
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    sess.close()


if __name__ == '__main__':
    main()
