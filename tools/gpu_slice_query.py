#!/usr/bin/env python3
"""Slice queries on the device (csrc/sliceq.hip, nnal_amd.slice_query) - the figures DESIGN.md section 7 records.

  1. Device against the NumPy restatement (slice_query.slice_scores_host) for every kind on 7 slices of 37 x 41 voxels, c = 3,
     T = 4, a 30 % ROI: the largest |device - host| over the bound (m + 8) 2^-52 abs_sums, and the counts.
  2. alq_unc_accumulate (first = 0, with the entropy sums) and alq_slice_scores (entropy, MC-entropy, BALD, mean) at c = 2 and
     c = 8 on `--slices` slices of `--side`^2 voxels: single calls between stream events (`--reps` after `--warmup`, medians of
     `--rounds` alternating rounds), each beside a torch device-to-device copy that moves the same bytes (a copy of half of
     what the kernel reads plus writes: the copy reads them once and writes them once), in the same process.
  3. The 'BALD' query end to end - slice_query.slice_scores, T = 10 passes of net_c_2d_dense(2) with a dropout layer - beside
     the same mean posteriors taken to the host through eval_utils.full_slice_segment(..., 'MC-posterior') (unchanged by the
     query: what a caller had before it), host clock around a device synchronise; and the bytes each copies back.

    python tools/gpu_slice_query.py [--reps 20] [--warmup 5] [--rounds 5] [--slices 64] [--side 256] [--out slice_query.json]

Prints one JSON line at the end."""
import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_dense import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--slices', type=int, default=64)
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import NN_extended, device, eval_utils, netspec, slice_query
    from nnal_amd._lib import check
    sess = device.default_session()
    dev = sess.device
    res = {}
    rs = np.random.RandomState(3)

    # ---- 1. device against the restatement
    n, V, c, T = 7, 37 * 41, 3, 4
    z = (rs.randn(T, c, n, V) * rs.choice([0.1, 3., 30.], size=(1, 1, n, V))).astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    P = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    au = (rs.randn(n, V) * 3).astype(np.float32)
    roi = (rs.rand(n, V) < 0.3).astype(np.uint8)
    d_roi = sess.to_device(roi.reshape(-1), torch.uint8)
    sum_p, sum_h = sess.empty((c, n * V), torch.float64), sess.empty((n * V,), torch.float64)
    for k in range(T):
        sess.unc_accumulate(sess.to_device(P[k].reshape(c, n * V), torch.float32), sum_p, sum_h, first=k == 0)
    acc = {}
    for kind in ('entropy', 'MC-entropy', 'BALD', 'AU'):
        want, wcnt, mag = slice_query.slice_scores_host(P[:1] if kind == 'entropy' else P, kind, roi=roi, au=au)
        f32 = sess.to_device(P[0].reshape(c, n * V), torch.float32) if kind == 'entropy' else sess.to_device(au.reshape(-1), torch.float32)
        got, gcnt = sess.slice_scores(slice_query.KINDS[kind], n, V, c, T=T, sum_p=sum_p, sum_h=sum_h, f32=f32, roi=d_roi)
        m = {'entropy': wcnt * c, 'MC-entropy': wcnt * c, 'BALD': wcnt * (c * T + c), 'AU': wcnt}[kind]
        lim = (m + 8) * 2. ** -52 * mag
        acc[kind] = dict(err_over_bound=float(np.max(np.abs(got.cpu().numpy() - want) / lim)), counts_equal=bool(np.array_equal(gcnt.cpu().numpy(), wcnt)))
    res['against_restatement'] = acc
    print('device against the restatement: %s' % acc)
    assert all(v['counts_equal'] and v['err_over_bound'] <= 1 for v in acc.values()), acc

    # ---- 2. the kernels beside a copy of the same bytes
    n, V, T = a.slices, a.side * a.side, 10
    R = n * V
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    d_roi = (torch.rand((R,), generator=g, device=dev) < 0.3).to(torch.uint8)
    scores, counts = sess.empty((n,), torch.float64), sess.empty((n,), torch.int64)
    p = lambda t: ct.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    fns, nbytes, keep = {}, {}, []
    sess.bind_stream()

    def copy_fn(nb):
        s_ = torch.empty((nb // 4,), dtype=torch.float32, device=dev).normal_()
        d_ = torch.empty_like(s_)
        return lambda: d_.copy_(s_)
    for c in (2, 8):
        post = torch.softmax(torch.randn((c, R), generator=g, device=dev) * 3, dim=0).contiguous()
        sum_p, sum_h = sess.empty((c, R), torch.float64), sess.empty((R,), torch.float64)
        sess.unc_accumulate(post, sum_p, sum_h, first=True)
        for _ in range(T - 1):
            sess.unc_accumulate(post, sum_p, sum_h)
        au = torch.randn((R,), generator=g, device=dev)
        keep.append((post, sum_p, sum_h, au))
        moved = {'accumulate': (4 * c + 2 * (8 * c + 8)) * R, 'entropy': 4 * c * R, 'MC-entropy': 8 * c * R, 'BALD': (8 * c + 8) * R, 'mean': 4 * R}
        calls = {'accumulate': lambda post=post, sum_p=sum_p, sum_h=sum_h, c=c: check(sess.lib.alq_unc_accumulate(sess.ctx, p(post), c, R, 0, p(sum_p), p(sum_h)))}
        for kind, K, f32 in (('entropy', 0, post), ('MC-entropy', 1, None), ('BALD', 2, None), ('mean', 3, au)):
            for rname, r in (('', None), ('_roi30', d_roi)):
                if kind == 'mean' and c == 8:
                    continue
                args = (sess.ctx, K, T, c, n, V, p(sum_p), p(sum_h), p(f32), p(r), p(scores), p(counts))
                calls[kind + rname] = lambda args=args: check(sess.lib.alq_slice_scores(*args))
                moved[kind + rname] = moved[kind] + (R if r is not None else 0)
        for name, fn in calls.items():
            key = 'c%d_%s' % (c, name)
            fns[key] = fn
            ck = 'copy_%dMB' % (moved[name] // 2 >> 20)
            fns.setdefault(ck, copy_fn(moved[name] // 2))
            nbytes[key] = (moved[name], ck)
    meds = {k: [] for k in fns}
    for _ in range(a.rounds):          # alternating rounds: drift of a shared machine falls on every kernel alike
        for k, fn in fns.items():
            meds[k].append(timed(torch, fn, a.warmup, a.reps)[0])
    t = {k: dict(us_median=float(np.median(v)), us_rounds=[float(x) for x in v], spread=float(max(v) / min(v))) for k, v in meds.items()}
    for k, (nb, ck) in nbytes.items():
        t[k].update(bytes=nb, gbps_median=nb / t[k]['us_median'] / 1e3, ratio_to_copy=t[k]['us_median'] / t[ck]['us_median'])
        print('%-22s %8.1f us median = %6.0f GB/s moved; copy moving the same bytes %7.1f us (spread %.2f); kernel / copy %.2f'
              % (k, t[k]['us_median'], t[k]['gbps_median'], t[ck]['us_median'], t[ck]['spread'], t[k]['ratio_to_copy']))
    res['kernels'] = dict(slices=n, voxels=V, T=T, timings=t)
    del fns, keep

    # ---- 3. the BALD query end to end beside the MC-posterior volume on the host
    side, Z, c = a.side, a.slices, 2
    ld, sk = netspec.net_c_2d_dense(c)
    m = NN_extended.CNN((side, side, 1), ld, 'slice_query', list(sk), dropout=[[0], 0.5], sess=sess, max_batch=16)
    m.set_weights(netspec.he_init(ld, (side, side, 1), seed=5, skips=sk, bias_std=0.05))
    vol = rs.randn(side, side, Z).astype(np.float32)
    ways = {'query_BALD': lambda: slice_query.slice_scores(m, sess, vol, 'BALD', roi=None, T=eval_utils.MC_PASSES, seed=1),
            'MC_posterior_volume': lambda: eval_utils.full_slice_segment(m, sess, vol, None, 'MC-posterior')}
    times = {k: [] for k in ways}
    for rnd in range(1 + a.rounds):
        for k, fn in ways.items():
            np.random.seed(7)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:                       # round 0 warms both up
                times[k].append((time.perf_counter() - t0) * 1e3)
    res['end_to_end'] = dict(side=side, slices=Z, c=c, T=eval_utils.MC_PASSES, ms_query=float(np.median(times['query_BALD'])),
                             ms_volume=float(np.median(times['MC_posterior_volume'])), ms_query_rounds=times['query_BALD'],
                             ms_volume_rounds=times['MC_posterior_volume'], bytes_to_host_query=16 * Z, bytes_to_host_volume=4 * c * side * side * Z)
    e = res['end_to_end']
    print("'BALD' query, T = %d, %d slices of %d^2, c = %d: %.1f ms, %d bytes to the host; full_slice_segment('MC-posterior') of the same volume: "
          '%.1f ms, %d bytes to the host' % (e['T'], Z, side, c, e['ms_query'], e['bytes_to_host_query'], e['ms_volume'], e['bytes_to_host_volume']))
    m.close()
    res.update(reps=a.reps, warmup=a.warmup, rounds=a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
