#!/usr/bin/env python3
"""Cost and accuracy of the stochastic influence recursion (alq_llfc_stoch_if, csrc/llfc.hip) on NET-B at [32, 32, 32] (d = 4096:
columns resident in LDS, and the same input forced through the streaming kernels) and NET-C at 32^3 (d = 262144: streaming only),
beside a plain torch implementation of the same recursion on the device, fp32 - what a user would write without the kernels.

    python tools/gpu_llfc.py --net netb|netc [--pool 4096] [--T 1000] [--ntr 64] [--reps 2] [--out profiles/llfc_<net>.json]
    python tools/gpu_llfc.py --table profiles/llfc_netb.json profiles/llfc_netc.json --design DESIGN.md

Features and posteriors come from one forward pass over the pool and one over the training patches; the timed calls are
DeviceModel.llfc_stoch_if_features_device on those device tensors (best of `reps` after a warm-up).  Accuracy: `--check-cols`
pool columns against the float64 restatement (tests/llfc_ref.py) on the same fp32 features, relative to the largest entry.
`scale` is the reference's 50, raised to twice the largest |u~|^2 of the training features when that is larger (the iteration
must contract).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEGIN, END = '<!-- llfc-table:begin -->', '<!-- llfc-table:end -->'
HBM_RATE = 6.3e12          # bytes / s a streaming kernel reaches on the MI355X


def table(files):
    rows = ['| net | d | c | pool | T | scale | resident (ms) | streaming (ms) | torch fp32 (ms) | streaming: share of the HBM rate | '
            'torch / best | max err. resident | max err. streaming | (T + 2) 2^-24 |', '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|']

    def f(v, fmt):
        return fmt % v if v is not None else 'n/a'
    for fn in files:
        r = json.loads(open(fn).read())
        best = min(v for v in (r.get('resident_ms'), r.get('streaming_ms')) if v is not None)
        rows.append('| %s | %d | %d | %d | %d | %.0f | %s | %s | %.1f | %s | %.1f | %s | %s | %.1e |' % (
            r['net'], r['d'], r['c'], r['pool'], r['T'], r['scale'], f(r.get('resident_ms'), '%.2f'), f(r.get('streaming_ms'), '%.1f'),
            r['torch_ms'], f(r.get('streaming_hbm_share'), '%.2f'), r['torch_ms'] / best, f(r.get('resident_err'), '%.1e'),
            f(r.get('streaming_err'), '%.1e'), (r['T'] + 2) * 2. ** -24))
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--net', choices=('netb', 'netc'), default='netb')
    ap.add_argument('--pool', type=int, default=4096)
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--ntr', type=int, default=64)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--check-cols', type=int, default=8)
    ap.add_argument('--out', default=None)
    ap.add_argument('--table', nargs='+', default=None, help='result files -> the markdown table')
    ap.add_argument('--design', default=None, help='with --table: the document whose llfc-table block is replaced')
    a = ap.parse_args()
    if a.table:
        t = table(a.table)
        print(t)
        if a.design:
            s = open(a.design).read()
            i, j = s.index(BEGIN) + len(BEGIN), s.index(END)
            open(a.design, 'w').write(s[:i] + '\n' + t + '\n' + s[j:])
        return

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import device, netspec
    from tests import llfc_ref
    sess = device.DeviceSession(0)
    if a.net == 'netc':
        ld, sk = netspec.net_c()
        shape, label, feat = (32, 32, 32, 1), 'NET-C 32^3', len(ld) - 2
    else:
        ld, sk = netspec.net_b(), ()
        shape, label, feat = (32, 32, 32), 'NET-B [32, 32, 32]', len(ld) - 2
    m = device.DeviceModel(sess, ld, shape, sk, feature_layer=feat, max_batch=256)
    m.set_weights(netspec.he_init(ld, shape, seed=13, skips=sk, bias_std=0.05))
    n, T, ntr = a.pool, a.T, a.ntr
    elems = int(np.prod(shape))
    gen = torch.Generator(device=sess.device).manual_seed(5)
    pool_t = torch.randn((n, elems), generator=gen, device=sess.device, dtype=torch.float32)
    tr_t = torch.randn((ntr, elems), generator=gen, device=sess.device, dtype=torch.float32)
    post, pred, pf = m.forward_device(pool_t, n, want_pred=True, want_feat=True)
    tpost, _, tf = m.forward_device(tr_t, ntr, want_feat=True)
    del pool_t, tr_t
    d, c = m.feature_dim, m.nclass
    P = (d + 1) * c
    scale = max(50., 2. * float(((tf.double() ** 2).sum(1) + 1.).max().item()))
    draws = np.random.RandomState(9).randint(0, ntr, size=T)
    res = dict(net=label, d=d, c=c, pool=n, T=T, ntr=ntr, scale=scale, reps=a.reps, auto_path=int(sess.lib.alq_llfc_if_path(d, c)))

    def torch_recursion():
        e = torch.nn.functional.one_hot(pred, c).float() - post.t()                       # [n, c]
        Gw, Vb = e[:, :, None] * pf[:, None, :], e.clone()
        Vw = Gw.clone()
        for r in draws:
            u, p = tf[r], tpost[:, r]
            s = Vw @ u + Vb
            q = p[None, :] * (s - (s * p[None, :]).sum(1, keepdim=True))
            Vw += Gw
            Vw -= (q / scale)[:, :, None] * u[None, None, :]
            Vb += e - q / scale
        return torch.cat([Vw.reshape(n, c * d), Vb], 1)

    arms = [('torch', torch_recursion)]
    if res['auto_path'] == 1:
        arms.append(('resident', lambda: m.llfc_stoch_if_features_device(pf, post, pred, tf, tpost, draws, scale, path=1)))
    arms.append(('streaming', lambda: m.llfc_stoch_if_features_device(pf, post, pred, tf, tpost, draws, scale, path=2)))
    cols = np.unique(np.linspace(0, n - 1, min(a.check_cols, n)).astype(np.int64))
    uniq, inv = np.unique(draws, return_inverse=True)
    ref = llfc_ref.stoch_if(pf[cols].cpu().numpy().T, post[:, cols].cpu().numpy(), pred[cols].cpu().numpy(),
                            tf[uniq].cpu().numpy().T, tpost[:, uniq].cpu().numpy(), inv.reshape(-1), scale).T
    for k, fn in arms:
        best = float('inf')
        for rep in range(a.reps + 1):                   # rep 0: warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            V = fn()
            torch.cuda.synchronize()
            if rep:
                best = min(best, (time.perf_counter() - t0) * 1e3)
            if rep < a.reps:
                del V
        res[k + '_ms'] = best
        res[k + '_err'] = float(np.abs(V[cols].cpu().numpy() - ref).max() / np.abs(ref).max())
        del V
    # per iteration the streaming kernels read V twice, write it once and read the pool features once
    res['streaming_hbm_share'] = (3. * n * P + n * d) * 4 * T / (res['streaming_ms'] * 1e-3) / HBM_RATE
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, 'w').write(line + '\n')
    m.close()


if __name__ == '__main__':
    main()
