#!/usr/bin/env python3
"""Runs the SLIC over-segmentation (alq_slic, csrc/slic.hip) on one MI355X against its NumPy statement (nnal_amd/slic.py) and times it.

    python tools/gpu_slic.py [--dims 256 256 128] [--m 1] [--segments 1000] [--T 10] [--out profiles/slic.json]

Prints whether labels and n_per_slice equal the statement byte for byte (and the first differing pixel if not), then, as medians
over 5 runs (after a warm-up) of `--iters` calls between two device events: the whole call at T iterations, the call at T = 0
(quantise + connectivity), their difference per iteration, and the time of a device copy that moves the bytes one iteration
must read and write - per pixel the 2 m bytes of q and the 4 of the label, once for the assignment (q in, label out) and once
for the update (label in, q in): 4 m + 8 bytes, as a copy of half that many bytes (read + written) - with the ratio.  The host
statement runs once on `--threads` threads (slices in flight).  Prints one JSON line."""
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
from nnal_amd import device, regions, slic  # noqa: E402
from nnal_amd.datasets.utils import ResidentSubject  # noqa: E402


def subject(dims, m, seed=7):
    """Smooth blobs plus noise: super-pixels have edges to follow and the connectivity step has orphans to adopt."""
    rs = np.random.RandomState(seed)
    H, W, S = dims
    y, x, z = np.meshgrid(np.arange(H), np.arange(W), np.arange(S), indexing='ij')
    mods = []
    for c in range(m):
        v = np.zeros(dims)
        for _ in range(12):
            cy, cx, r, a = rs.rand() * H, rs.rand() * W, (0.05 + 0.2 * rs.rand()) * min(H, W), rs.rand() * 100
            v += a * (((y - cy) ** 2 + (x - cx - 0.1 * z) ** 2) < r * r)
        mods.append((v + 4.0 * rs.randn(*dims)).astype(np.float32))
    return mods


def time_calls(fn, iters, runs=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return float(np.median(ts)), [float(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument('--m', type=int, default=1)
    ap.add_argument('--segments', type=int, default=1000)
    ap.add_argument('--compactness', type=float, default=0.1)
    ap.add_argument('--T', type=int, default=10)
    ap.add_argument('--min-size', type=int, default=8)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--no-host', action='store_true', help='skip the statement: timings only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dims = tuple(a.dims)
    H, W, S = dims
    sess = device.DeviceSession(0)
    mods = subject(dims, a.m)
    gh, gw = slic.grid_for(H, W, a.segments)
    w = slic.spatial_weight(a.compactness, H, W, gh, gw)
    lo, scale = slic.quant_range(mods)
    vol = ResidentSubject.pack(sess, mods).vol
    out = dict(tool='gpu_slic', dims=list(dims), m=a.m, grid=[gh, gw], w=w, T=a.T, min_size=a.min_size, iters=a.iters)

    def run(T):
        return regions.slic_device(sess, vol, gh, gw, w, T, a.min_size, None, lo, scale)

    labels, counts = run(a.T)
    got_l, got_n = labels.cpu().numpy(), counts.cpu().numpy()
    out['regions_per_slice'] = [int(got_n.min()), float(got_n.mean()), int(got_n.max())]
    if not a.no_host:
        t0 = time.perf_counter()
        want_l, want_n = slic.slic_host(mods, gh, gw, w, a.T, a.min_size, None, lo, scale, threads=a.threads)
        out['host_s'] = time.perf_counter() - t0
        out['host_threads'] = a.threads
        out['counts_equal'] = bool(got_n.tobytes() == want_n.tobytes())
        out['labels_equal'] = bool(got_l.tobytes() == want_l.tobytes())
        if not out['labels_equal']:
            bad = np.argwhere(got_l.transpose(2, 0, 1) != want_l.transpose(2, 0, 1))[0]      # first in (slice, row, column) order
            z, y, x = (int(v) for v in bad)
            out['first_difference'] = dict(z=z, y=y, x=x, device=int(got_l[y, x, z]), statement=int(want_l[y, x, z]),
                                           differing=int(np.count_nonzero(got_l != want_l)))
    sess.bind_stream()
    nbytes = int(sess.lib.alq_slic_work_bytes((C.c_int64 * 3)(*dims), a.m, gh, gw))
    work = sess.empty((nbytes // 8,), torch.int64)

    def call(T):
        regions.slic_device(sess, vol, gh, gw, w, T, a.min_size, None, lo, scale, work=work)

    out['call_s'], out['call_runs'] = time_calls(lambda: call(a.T), a.iters)
    out['call_T0_s'] = time_calls(lambda: call(0), a.iters)[0]
    out['iteration_s'] = (out['call_s'] - out['call_T0_s']) / max(a.T, 1)
    px = H * W * S
    moved = px * (4 * a.m + 8)
    src = torch.empty((moved // 2,), dtype=torch.uint8, device=sess.device)
    dst = torch.empty_like(src)
    out['iteration_bytes'] = moved
    out['copy_s'] = time_calls(lambda: dst.copy_(src), 20)[0]
    out['iteration_over_copy'] = out['iteration_s'] / out['copy_s']
    if 'host_s' in out:
        out['host_over_device'] = out['host_s'] / out['call_s']
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    sess.close()


if __name__ == '__main__':
    main()
