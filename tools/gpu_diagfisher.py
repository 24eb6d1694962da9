#!/usr/bin/env python3
"""Cost of DeviceModel.diagonal_fisher on its two arms: the fused statistic (alq_diag_fisher, csrc/dfisher.hip) and the rows
arm (alq_param_grads per sample + alq_sq_accum) - the device halves of its two arms, diagonal_fisher_device and
diagonal_fisher_rows_device, without the copy of the result to the host that both share - NET-C at 32^3 and NET-B at [32, 32, 32], 64 samples each in one pass.

    python tools/gpu_diagfisher.py --net netc|netb [--reps 5] [--out profiles/diagf_<net>.json]
    python tools/gpu_diagfisher.py --net netc --arm fused --reps 2            # one arm only (the profiler run)
    python tools/gpu_diagfisher.py --net netc --stats kernel_stats.csv --out ...   # fold a rocprofv3 --kernel-trace --stats run in
    python tools/gpu_diagfisher.py --table profiles/diagf_netc32_B64.json profiles/diagf_netb_B64.json --design DESIGN.md

One process, one model, the two arms interleaved, best of `reps` after a warm-up; peak device memory per arm is
torch.cuda.max_memory_allocated over that arm's calls less what was allocated before them (the library's own workspaces are
not torch's and show in neither).  Prints one JSON line.  tools/run_diagfisher_profile.sh runs the timing and the profiler pass."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEGIN, END = '<!-- diagf-table:begin -->', '<!-- diagf-table:end -->'


def short_name(name):
    """Kernel name without return type, namespaces and argument list; template arguments kept (nested names inside them too)."""
    name = name.replace('(anonymous namespace)::', '')
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):           # the argument list: the first '(' outside template brackets
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            cut = i
            break
    name = name[:cut]
    depth, start = 0, 0
    for i, ch in enumerate(name):           # the last '::' or space outside template brackets
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif depth == 0 and (ch == ' ' or name[i:i + 2] == '::'):
            start = i + (1 if ch == ' ' else 2)
    return name[start:][:96]


def table(files):
    rows = ['| net | samples | parameters | rows arm (ms) | fused (ms) | ratio | rows peak (MB) | fused peak (MB) | max rel. diff. | '
            'largest kernels of the fused arm (rocprofv3, share of kernel time) |', '|---|---|---|---|---|---|---|---|---|---|']
    for f in files:
        r = json.loads(open(f).read())
        top = ', '.join('%s %.0f %%' % (k['name'], k['share'] * 100) for k in r.get('rocprof_top', [])[:4]) or 'n/a'
        rows.append('| %s | %d | %d | %.3f | %.3f | %.2f | %.1f | %.1f | %.2e | %s |' % (
            r['net'], r['samples'], r['params'], r['rows_ms'], r['fused_ms'], r['ratio'], r['rows_peak_bytes'] / 1e6,
            r['fused_peak_bytes'] / 1e6, r['max_rel_diff'], top))
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--net', choices=('netc', 'netb'), default='netc')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--arm', choices=('both', 'fused', 'rows'), default='both')
    ap.add_argument('--stats', default=None, help='rocprofv3 kernel_stats.csv of a run of this tool (no timing is done)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--table', nargs='+', default=None, help='result files -> the markdown table')
    ap.add_argument('--design', default=None, help='with --table: the document whose diagf-table block is replaced')
    a = ap.parse_args()

    if a.table:
        t = table(a.table)
        print(t)
        if a.design:
            s = open(a.design).read()
            i, j = s.index(BEGIN) + len(BEGIN), s.index(END)
            open(a.design, 'w').write(s[:i] + '\n' + t + '\n' + s[j:])
        return

    if a.stats:
        res = json.loads(open(a.out).read()) if a.out and os.path.exists(a.out) else {}
        rows = list(csv.DictReader(open(a.stats)))
        total = sum(float(r['TotalDurationNs']) for r in rows) or 1.
        res['rocprof_top'] = [dict(name=short_name(r['Name']), calls=int(r['Calls']),
                                   ms=float(r['TotalDurationNs']) / 1e6, share=float(r['TotalDurationNs']) / total)
                              for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:10]]
        line = json.dumps(res)
        print(line)
        if a.out:
            open(a.out, 'w').write(line + '\n')
        return

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import device, netspec
    sess = device.DeviceSession(0)
    B = 64
    if a.net == 'netc':
        ld, sk = netspec.net_c()
        shape, label = (32, 32, 32, 1), 'NET-C 32^3'
    else:
        ld, sk = netspec.net_b(), ()
        shape, label = (32, 32, 32), 'NET-B [32, 32, 32]'
    m = device.DeviceModel(sess, ld, shape, sk, max_batch=B)
    m.set_weights(netspec.he_init(ld, shape, seed=13, skips=sk, bias_std=0.05))
    rs = np.random.RandomState(3)
    t = sess.to_device(rs.randn(B, int(np.prod(shape))).astype(np.float32), torch.float32)
    lab = rs.randint(0, 2, size=B).astype(np.int32)
    labd = sess.to_device(lab, torch.int32)

    def fused():
        return m.diagonal_fisher_device(t, B, labd)

    def rows():
        return m.diagonal_fisher_rows_device(t, B, lab)

    arms = [('fused', fused), ('rows', rows)] if a.arm == 'both' else [(a.arm, fused if a.arm == 'fused' else rows)]
    best = {k: float('inf') for k, _ in arms}
    peak = {k: 0 for k, _ in arms}
    out = {}
    for rep in range(a.reps + 1):                       # rep 0: warm-up (workspaces, first launches)
        for k, fn in arms:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                best[k] = min(best[k], dt)
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - base)
            out[k] = r
            del r
    res = dict(net=label, samples=B, params=m.num_params, reps=a.reps)
    for k, _ in arms:
        res[k + '_ms'] = best[k]
        res[k + '_peak_bytes'] = int(peak[k])
    if a.arm == 'both':
        f, r = out['fused'], out['rows']
        res['ratio'] = best['rows'] / best['fused']
        res['max_rel_diff'] = float(((f - r).abs() / r.abs().max()).max().item())
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, 'w').write(line + '\n')
    m.close()


if __name__ == '__main__':
    main()
