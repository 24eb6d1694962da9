#!/usr/bin/env python3
"""The committee queries `ensemble` and `QBC-JS` (PW_NNAL.query_multimg, PW_NNAL.py:453-545) on the --config 5 geometry of
bench.py: 4 synthetic subjects of 192 x 192 x 24, in-plane grid spacing 3 (~393 k pool voxels), patch (25, 25, 1) x 2
modalities, NET-B; M = 7 He-init members (distinct seeds) written as .npz weight files, like the reference's 1 + 6.

    python tools/gpu_committee.py [--members 7] [--reps 2] [--out FILE]
    python tools/gpu_committee.py --stats kernel_stats.csv ...        # after a rocprofv3 --kernel-trace --stats run of this tool

Prints one JSON line: seconds per query of each method; of the literal restatement (M x bin_uncertainty_filter_multimg to
the host + NumPy); the sum over members of the weight load and of a forward-only pool sweep, each timed alone; the committee
kernel and top-k times from the library's profiling classes ('committee'; the top-k runs under 'reduce') and, with --stats,
from rocprofv3's kernel statistics."""
import argparse
import csv
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
from nnal_amd import PW_NNAL, device, netspec, patch_utils  # noqa: E402


def volumes():
    """bench.py volume_config's subjects (same seed and shapes)."""
    S, m = 4, 2
    dims = (192, 192, 24)
    rad = (12, 12, 0)
    rs = np.random.RandomState(1006)
    all_padded, pool_inds, stats = [], [], []
    for i in range(S):
        vols = [rs.randn(*dims) * (1. + .2 * j) + .3 * i for j in range(m)]
        mask = (rs.rand(*dims) < .5).astype(np.int64)
        all_padded.append([np.pad(v, [(r, r) for r in rad], 'constant') for v in vols] + [mask])
        g = np.zeros(dims, bool)
        g[::3, ::3, :] = True
        pool_inds.append(np.nonzero(g.ravel())[0].astype(np.int64))
        stats.append([v for vol in vols for v in (float(vol.mean()), float(vol.std()))])
    return all_padded, pool_inds, np.asarray(stats)


def ent(x):
    a, b = x.copy(), 1 - x
    a[a == 0] += 1e-6
    b[b == 0] += 1e-6
    return -a * np.log(a) - b * np.log(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=7)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--stats', default=None, help='rocprofv3 kernel_stats.csv of a run of this tool')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    sess = device.DeviceSession(0)
    all_padded, pool_inds, stats = volumes()
    n_pool = int(sum(len(p) for p in pool_inds))

    class Expr(object):
        pars = {'patch_shape': (25, 25, 1), 'ntb': 8192, 'k': 100, 'B': 4096}
        nclass = 2
        train_stats = stats
    expr = Expr()
    ld = netspec.net_b()
    in_shape = (25, 25, 2)
    model = device.DeviceModel(sess, ld, in_shape, (), max_batch=8192)
    model.set_weights(netspec.he_init(ld, in_shape, seed=16))
    tmp = tempfile.mkdtemp(prefix='committee_')
    try:
        paths = []
        for i in range(a.members):
            p = os.path.join(tmp, 'member_%d.npz' % i)
            model.set_weights(netspec.he_init(ld, in_shape, seed=200 + i))
            model.save_weights(p)
            paths.append(p)
        model.set_weights(netspec.he_init(ld, in_shape, seed=16))
        expr.pretrained_paths = paths
        labeled = [[] for _ in pool_inds]

        def query(method):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q = PW_NNAL.query_multimg(expr, model, sess, all_padded, pool_inds, labeled, method)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, q

        query('ensemble')                                   # warm-up; builds and caches expr.model_holder
        holder = expr.model_holder
        out = dict(tool='gpu_committee', members=a.members, pool_voxels=n_pool, net='NET-B', patch=[25, 25, 2], k=expr.pars['k'],
                   holder_max_batch=holder.max_batch)
        picks = {}
        for method in ('ensemble', 'QBC-JS'):
            ts = []
            for _ in range(a.reps):
                dt, q = query(method)
                ts.append(dt)
            picks[method] = q
            out['s_per_query_' + method] = min(ts)
            out['s_per_query_%s_all' % method] = ts

        # the literal restatement: M x (load + bin_uncertainty_filter_multimg to the host) + NumPy, both methods from one sweep
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        av, avh = 0, 0
        dvols = {}
        for i, p in enumerate(paths):
            holder.perform_assign_ops(p, sess)
            posts = PW_NNAL.bin_uncertainty_filter_multimg(expr, holder, sess, all_padded, pool_inds, expr.pars['k'],
                                                           {holder.keep_prob: 1.}, _vols=dvols)
            av = (posts + i * av) / (i + 1)
            avh = (ent(posts) + i * avh) / (i + 1)
        t_sweeps = time.perf_counter() - t0
        t1 = time.perf_counter()
        ens = np.argsort(np.abs(av - .5), kind='stable')[:expr.pars['k']]
        t_ens = time.perf_counter() - t1
        t1 = time.perf_counter()
        qbc = np.argsort(-(ent(av) - avh), kind='stable')[:expr.pars['k']]
        t_qbc = time.perf_counter() - t1
        sizes = [len(p) for p in pool_inds]
        out['restatement_s_ensemble'] = t_sweeps + t_ens        # (the ensemble restatement does not need the entropies; their
        out['restatement_s_QBC-JS'] = t_sweeps + t_qbc          # NumPy cost is inside t_sweeps for both: a slight overstatement)
        out['restatement_picks_equal_ensemble'] = all(np.array_equal(x, y) for x, y in
                                                      zip(patch_utils.global2local_inds(ens, sizes), picks['ensemble']))
        out['restatement_picks_equal_QBC-JS'] = all(np.array_equal(np.sort(x), np.sort(y)) for x, y in
                                                    zip(patch_utils.global2local_inds(qbc, sizes), picks['QBC-JS']))

        # the parts, each timed alone: weight loads, forward-only pool sweeps (device posteriors, no host copy)
        t_load, t_sweep = 0., 0.
        for p in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            holder.perform_assign_ops(p, sess)
            torch.cuda.synchronize()
            t_load += time.perf_counter() - t0
            t0 = time.perf_counter()
            PW_NNAL.pool_posteriors_device(expr, holder, sess, all_padded, pool_inds, {holder.keep_prob: 1.}, dvols)
            torch.cuda.synchronize()
            t_sweep += time.perf_counter() - t0
        out['sum_weight_load_s'] = t_load
        out['sum_member_sweep_s'] = t_sweep
        for method in ('ensemble', 'QBC-JS'):
            q = out['s_per_query_' + method]
            out['ratio_to_sweep_plus_load_' + method] = q / (t_load + t_sweep)
            out['speedup_vs_restatement_' + method] = out['restatement_s_' + method] / q

        # committee kernel + top-k from the library's launch timer (one more query per method)
        for method in ('ensemble', 'QBC-JS'):
            sess.prof_reset()
            sess.prof_enable(True)
            dt, _ = query(method)
            prof = sess.prof_read()
            sess.prof_enable(False)
            c, r = prof['committee'], prof['reduce']
            out['prof_' + method] = dict(query_s=dt, committee_ms=c['ms'], committee_launches=c['launches'], topk_ms=r['ms'],
                                         topk_launches=r['launches'], share=(c['ms'] + r['ms']) / 1e3 / dt)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    if a.stats:
        rows = list(csv.DictReader(open(a.stats)))
        com = [r for r in rows if 'committee_update_kernel' in r['Name']]
        tk = [r for r in rows if any(s in r['Name'] for s in ('topk_init_kernel', 'bitonic_', 'topk_emit_kernel'))]
        out['rocprof_committee'] = dict(calls=sum(int(r['Calls']) for r in com), ms=sum(float(r['TotalDurationNs']) for r in com) / 1e6)
        out['rocprof_topk'] = dict(calls=sum(int(r['Calls']) for r in tk), ms=sum(float(r['TotalDurationNs']) for r in tk) / 1e6)
        tot = sum(float(r['TotalDurationNs']) for r in rows)
        out['rocprof_top'] = [dict(name=r['Name'][:80], calls=int(r['Calls']), ms=float(r['TotalDurationNs']) / 1e6)
                              for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:8]]
        out['rocprof_total_kernel_ms'] = tot / 1e6
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    expr.model_holder.close()               # the holder's device memory belongs to the session: models first
    model.close()
    sess.close()


if __name__ == '__main__':
    main()
