#!/usr/bin/env python3
"""Cost of one exact Hessian-vector product (alq_hess_vecp, csrc/hvp.hip) next to one gradient call
(alq_param_grads mode 1, per_sample 0) on the same batch: NET-C at 32^3 with batch 32, NET-B at 25 x 25 x 2 with batch 200.

    python tools/gpu_hvp.py --net netc|netb [--reps 7] [--out profiles/hvp_<net>.json]
    python tools/gpu_hvp.py --net netc --stats kernel_stats.csv --out ...     # fold a rocprofv3 --kernel-trace --stats run in
    python tools/gpu_hvp.py --table profiles/hvp_netc32_B32.json profiles/hvp_netb_B200.json --design DESIGN.md

One process, the two arms interleaved, best of `reps` after a warm-up (the first product allocates the tangent workspaces and
uploads the fp32 weights).  By operation count a product is one forward pass, two forward-sized contractions and a backward
sweep with twice the backward-data and twice the weight-gradient work: roughly three gradient calls.  The measured ratio is
a recorded number, not a bar.  tools/run_hvp_profile.sh runs the timing and the profiler passes, each under its own time limit."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEGIN, END = '<!-- hvp-table:begin -->', '<!-- hvp-table:end -->'


def table(files):
    rows = ['| net | batch | parameters | gradient call (ms) | product (ms) | ratio | largest kernels of a product (rocprofv3, share of kernel time) |',
            '|---|---|---|---|---|---|---|']
    for f in files:
        r = json.loads(open(f).read())
        top = ', '.join('%s %.0f %%' % (k['name'], k['share'] * 100) for k in r.get('rocprof_top', [])[:4]) or 'n/a'
        rows.append('| %s | %d | %d | %.3f | %.3f | %.2f | %s |' % (r['net'], r['batch'], r['params'], r['grad_ms'], r['hvp_ms'],
                                                                  r['ratio'], top))
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--net', choices=('netc', 'netb'), default='netc')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--stats', default=None, help='rocprofv3 kernel_stats.csv of a run of this tool (no timing is done)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--table', nargs='+', default=None, help='result files -> the markdown table')
    ap.add_argument('--design', default=None, help='with --table: the document whose hvp-table block is replaced')
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
        res['rocprof_top'] = [dict(name=r['Name'].split('(')[0].split('::')[-1][:48], calls=int(r['Calls']),
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
    if a.net == 'netc':
        ld, sk = netspec.net_c()
        shape, B, label = (32, 32, 32, 1), 32, 'NET-C 32^3'
    else:
        ld, sk = netspec.net_b(), ()
        shape, B, label = (25, 25, 2), 200, 'NET-B 25 x 25 x 2'
    pars = netspec.he_init(ld, shape, seed=21, skips=sk, bias_std=0.05)
    model = device.DeviceModel(sess, ld, shape, sk, max_batch=B)
    model.set_weights(pars)
    gen = torch.Generator(device=sess.device)
    gen.manual_seed(5)
    x = torch.randn((B, int(np.prod(shape))), generator=gen, dtype=torch.float32, device=sess.device)
    lab = sess.to_device(np.random.RandomState(6).randint(0, 2, size=B).astype(np.int32), torch.int32)
    v = torch.randn((model.num_params,), generator=gen, dtype=torch.float32, device=sess.device)
    hv = sess.empty((model.num_params,), torch.float64)

    def grad():
        model.param_grads_device(x, B, 1, labels=lab, loss_scale=1. / B, per_sample=False)

    def prod():
        model.hess_vecp_device(x, B, lab, v, None, 1. / B, hv)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    once(grad), once(prod)                  # warm-up: workspaces, weights, code objects
    tg, tp = [], []
    for _ in range(a.reps):                 # arms interleaved
        tg.append(once(grad))
        tp.append(once(prod))
    out = dict(net=label, batch=B, params=model.num_params, reps=a.reps, grad_ms=min(tg) * 1e3, hvp_ms=min(tp) * 1e3,
               ratio=min(tp) / min(tg), grad_ms_all=[t * 1e3 for t in tg], hvp_ms_all=[t * 1e3 for t in tp])
    line = json.dumps(out)
    print(line)
    if a.out:
        open(a.out, 'w').write(line + '\n')
    model.close()
    sess.close()


if __name__ == '__main__':
    main()
