#!/usr/bin/env python3
"""The A-optimal design solve of the `fi` query on the device (DeviceSession.aopt_design, csrc/aopt.hip) against the host solver
(NNAL_tools.SDP_query_distribution) in the same process, on synthetic Fisher-like candidates (rank 2 + diagonal load).

    python tools/gpu_aopt.py [--cases 4096x8,4096x3,20000x8,100000x8] [--reps 5] [--host-reps 3] [--out profiles/aopt_solve.json]

Per case: status and Newton steps of both, objective and the optimality gap recomputed on the host in fp64 from the returned q,
max|q_dev - q_host|, and the wall time of a whole solve (median of `reps` after a warm-up; on the device side the read-backs
and the host algebra are inside).  The device time is split into the four launches (each with its synchronising read-back)
and the rest (the L x L / m x m algebra in NumPy); launch A is also timed alone with events, next to the time its HBM read of
n m 8 bytes takes at the streaming rate.  Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 6.3e12          # bytes / s: what the project's streaming kernels reach on the MI355X (wpack_fc_kernel)


def candidates(n, L, diag_load, seed):
    rs = np.random.RandomState(seed)
    g0 = rs.randn(n, L) * 0.05 * np.exp(rs.randn(L))[None, :]
    g1 = -(0.5 + rs.rand(n, 1)) * g0 + 0.01 * rs.randn(n, L) * np.abs(g0).mean()
    p = rs.rand(n)
    idx = rs.permutation(n)
    p[idx[:n // 10]] = 0.0
    p[idx[n // 10:2 * (n // 10)]] = 1.0
    return ((g0[:, :, None] * g0[:, None, :]) * (1 - p)[:, None, None] + (g1[:, :, None] * g1[:, None, :]) * p[:, None, None]
            + diag_load * np.eye(L)[None])


def recomputed(A, q):
    Mi = np.linalg.inv(np.tensordot(q, A, axes=(0, 0)))
    f = float(np.trace(Mi))
    d = np.tensordot(A, Mi @ Mi, axes=([1, 2], [0, 1]))
    return f, float(d.max() / f - 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='4096x8,4096x3,20000x8,100000x8')
    ap.add_argument('--load', type=float, default=1e-5)
    ap.add_argument('--tol', type=float, default=1e-7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import nnal_amd  # noqa: F401
    from nnal_amd import NNAL_tools, device
    sess = device.DeviceSession(0)
    torch = sess.torch
    results = []
    for case in a.cases.split(','):
        n, L = (int(v) for v in case.split('x'))
        m = L * (L + 1) // 2
        A = candidates(n, L, a.load, seed=n + L)
        A_dev = sess.to_device(A, torch.float64)
        # per-launch wall time (launch + read-back), accumulated over one solve
        spent = {}

        def timed(name):
            fn = getattr(device.DeviceSession, name)

            def wrapper(*args, **kw):
                t0 = time.perf_counter()
                out = fn(sess, *args, **kw)
                spent[name] = spent.get(name, 0.0) + time.perf_counter() - t0
                return out
            return wrapper
        sess.aopt_design(A_dev, tol=a.tol)                                     # warm-up
        walls = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev = sess.aopt_design(A_dev, tol=a.tol)
            walls.append(time.perf_counter() - t0)
        names = ('aopt_svec', 'aopt_stats', 'aopt_direction', 'aopt_linesearch', 'aopt_update')
        for nm in names:
            setattr(sess, nm, timed(nm))
        t0 = time.perf_counter()
        sess.aopt_design(A_dev, tol=a.tol)
        split_total = time.perf_counter() - t0
        for nm in names:
            delattr(sess, nm)
        hwalls = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host = NNAL_tools.SDP_query_distribution(A, 0., [], None, tol=a.tol)
            hwalls.append(time.perf_counter() - t0)
        # launch A alone, events around back-to-back calls without read-backs
        V = sess.aopt_svec(A_dev)
        q = torch.full((n,), 1.0 / n, dtype=torch.float64, device=sess.device)
        work = sess.aopt_work(n, L)
        out = sess.empty(((m + 2) * (m + 3) // 2 + 1,), torch.float64)
        kvec, R = np.ones(m), np.ascontiguousarray(np.tril(np.ones((m, m))))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sess.bind_stream()

        def stats_call():
            device.check(sess.lib.alq_aopt_stats(sess.ctx, C.c_void_p(V.data_ptr()), C.c_void_p(q.data_ptr()), n, m,
                                                 C.c_void_p(kvec.ctypes.data), C.c_void_p(R.ctypes.data), 1.0, 1.0,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr())))
        for _ in range(3):
            stats_call()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            stats_call()
        e1.record()
        torch.cuda.synchronize()
        qd, qh = np.asarray(dev['x'][:n]), np.asarray(host['x'][:n])
        fd, gd = recomputed(A, qd)
        fh, gh = recomputed(A, qh)
        launches = sum(spent.values())
        r = {'n': n, 'L': L, 'm': m, 'diag_load': a.load, 'tol': a.tol,
             'device': {'status': dev['status'], 'iterations': dev['iterations'], 'objective': fd, 'gap': gd,
                        'seconds': float(np.median(walls)), 'seconds_all': walls},
             'host': {'status': host['status'], 'iterations': host['iterations'], 'objective': fh, 'gap': gh,
                      'seconds': float(np.median(hwalls)), 'seconds_all': hwalls},
             'max_abs_q_diff': float(np.abs(qd - qh).max()),
             'device_split_seconds': dict(spent, host_algebra=split_total - launches, total=split_total),
             'launch_A_ms': e0.elapsed_time(e1) / 20, 'launch_A_hbm_read_ms': n * m * 8 / HBM_RATE * 1e3}
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        with open(a.out, 'w') as f:
            for r in results:
                f.write(json.dumps(r) + '\n')
    sess.close()


if __name__ == '__main__':
    main()
