#!/usr/bin/env python3
"""Mean-teacher training on the device (csrc/mteach.hip) - the figures DESIGN.md records.

  1. Accuracy: mt_cotangent_kernel at R = 64 x 32^3 voxels, c = 2, with voxel weights, class weights, the focal term and 30 %
     unlabelled voxels, against the fp64 statement (nnal_amd.mteach) on the first 2^18 voxels: the worst row error over its
     bound 4 * 2^-24 * (|labelled term| + |consistency term|), and the statistics over all voxels.
  2. Time of single launches between stream events (`--reps` after `--warmup`, medians): the kernel with its finish launch
     (32 bytes per voxel: two posteriors of each model, label, weight, two row entries), its statistics-only form, the
     existing loss_cotangent_kernel in ITS statistics-only form on the same columns (alq_loss_stats: it reads half the planes
     and writes no rows), and a device-to-device copy of the kernel's bytes in the same process.
  2b. The aleatoric-uncertainty kernels (AU_4U): mt_cotangent_au_kernel against the fp64 statement on the first 2^18 voxels, and
     in `--rounds` alternating rounds its time against mt_cotangent_kernel at the same R and c (40 against 32 bytes per voxel at
     c = 2: 4 (2c + 1) + 8 read and 4 (c + 1) written against 8c + 8 and 4c), dense_head_fwd_au_kernel at c classes against
     dense_head_fwd_kernel at c + 1 outputs (the same bytes), and device copies of each kernel's bytes.  The spread max / min of
     the parent kernel's round medians is the noise floor the ratios are read against.
  3. One mean-teacher step (train_step + ema_apply) of net_c_dense at 32^3, N = `--batch`, against the plain dense step of a
     model built without MT_SSL, alternating, host clock around a device synchronise.

    python tools/gpu_mteach.py [--reps 20] [--warmup 5] [--rounds 5] [--batch 64] [--skip-step] [--out mteach.json]

Prints one JSON line at the end."""
import argparse
import ctypes as C
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
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import NN_extended, device, mteach, netspec
    from nnal_amd._lib import LossT, check
    sess = device.default_session()
    dev = sess.device
    res = {}
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    c, R = 2, 64 * 32 ** 3
    g = torch.Generator(device='cpu').manual_seed(11)
    p = torch.softmax(2. * torch.randn((c, R), generator=g), 0).to(dev)
    q = torch.softmax(2. * torch.randn((c, R), generator=g), 0).to(dev)
    lab = torch.randint(0, c, (R,), generator=g, dtype=torch.int32)
    lab[torch.rand((R,), generator=g) < 0.3] = -1
    lab = lab.to(dev)
    sw = (0.25 + torch.rand((R,), generator=g)).to(dev)
    cw32 = np.asarray([0.3, 1.7], np.float32)          # (the statement reads the weights the device reads)
    cw = torch.tensor(cw32, device=dev)
    rows = torch.empty((R, c), dtype=torch.float32, device=dev)
    st = torch.empty((3,), dtype=torch.float64, device=dev)
    L = LossT(0, 2., 0.7, 1., cw.data_ptr(), sw.data_ptr(), None, None)
    s, k = float(np.float32(64. / (0.7 * R))), float(np.float32(2. / (c * 32 ** 3)))
    sess.bind_stream()

    def cot():
        check(sess.lib.alq_mt_cotangent(sess.ctx, P(p), P(q), c, R, P(lab), C.byref(L), s, k, mteach.L2, P(rows), P(st)))

    def stats():
        check(sess.lib.alq_mt_stats(sess.ctx, P(p), P(q), c, R, P(lab), C.byref(L), mteach.L2, P(st)))

    def old_stats():
        check(sess.lib.alq_loss_stats(sess.ctx, P(p), c, R, P(lab), C.byref(L), P(st)))

    cot()
    torch.cuda.synchronize()
    n = 1 << 18
    ref = mteach.evaluate(p[:, :n].cpu().numpy(), q[:, :n].cpu().numpy(), lab[:n].cpu().numpy(), mteach.L2, s, k, cw32,
                          sw[:n].cpu().numpy(), 2.)
    tol = 4 * 2. ** -24 * (np.abs(ref['labelled_rows']) + np.abs(ref['cons_rows']))
    err = np.abs(rows[:n].cpu().numpy().astype(np.float64) - ref['rows'])
    res['row_err_over_bound'] = float((err / np.maximum(tol, 1e-300)).max())
    full = mteach.evaluate(p.cpu().numpy(), q.cpu().numpy(), lab.cpu().numpy(), mteach.L2, s, 0., cw32, sw.cpu().numpy(), 2.)
    res['stats_rel_err'] = [float(abs(x - y) / max(abs(y), 1e-300)) for x, y in zip(st.cpu().numpy(), full['stats'])]
    print('R = %d: worst row error / bound %.3f, statistics relative error %s' % (R, res['row_err_over_bound'], res['stats_rel_err']))

    nbytes = 32 * R
    src = torch.empty((nbytes // 8,), dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    # what the fp64 transcendentals cost: the same launch without weights and focal term (one log per labelled voxel, no pow),
    # with the L2 measure and with CE (two more logs per voxel)
    Lp = LossT(0, -1., 0.7, 1., None, None, None, None)

    def plain(measure):
        return lambda: check(sess.lib.alq_mt_cotangent(sess.ctx, P(p), P(q), c, R, P(lab), C.byref(Lp), s, k, measure, P(rows), P(st)))

    for name, fn in (('mt_cotangent', cot), ('mt_stats', stats), ('mt_cotangent_plain_l2', plain(mteach.L2)),
                     ('mt_cotangent_plain_ce', plain(mteach.CE)), ('loss_stats_old_kernel', old_stats), ('copy', lambda: dst.copy_(src))):
        med, best = timed(torch, fn, a.warmup, a.reps)
        res[name] = dict(us_median=med, us_min=best)
        print('%s: %.1f us median (%.1f min)' % (name, med, best))
    res['mt_cotangent'].update(bytes=nbytes, gbps_median=nbytes / res['mt_cotangent']['us_median'] / 1e3,
                               ratio_to_copy=res['mt_cotangent']['us_median'] / res['copy']['us_median'],
                               ratio_to_old_stats=res['mt_cotangent']['us_median'] / res['loss_stats_old_kernel']['us_median'])
    print('mt_cotangent: %.1f MB = %.0f GB/s; kernel / copy = %.2f; kernel / old statistics-only kernel = %.2f'
          % (nbytes / 1e6, res['mt_cotangent']['gbps_median'], res['mt_cotangent']['ratio_to_copy'], res['mt_cotangent']['ratio_to_old_stats']))
    del src, dst

    # ---- the aleatoric-uncertainty kernels
    kappa, kau, Ci = 0.1, float(np.float32(1. / 32 ** 3)), 16
    au = (torch.clamp(torch.randn((R,), generator=g), min=0.) * 2.).to(dev)
    rows_au = torch.empty((R, c + 1), dtype=torch.float32, device=dev)
    xh = torch.randn((R, Ci), generator=g).to(dev)
    Wh, bh = (0.5 * torch.randn((Ci, c + 1), generator=g)).to(dev), torch.randn((c + 1,), generator=g).to(dev)
    post_h = torch.empty((c + 1, R), dtype=torch.float32, device=dev)
    au_h = torch.empty((R,), dtype=torch.float32, device=dev)

    def cot_au():
        check(sess.lib.alq_mt_cotangent_au(sess.ctx, P(p), P(q), P(au), c, R, P(lab), C.byref(L), s, k, kau, kappa, mteach.L2, P(rows_au), P(st)))

    def head_au():
        check(sess.lib.alq_dense_head_fwd_au(sess.ctx, P(xh), R, Ci, c, P(Wh), P(bh), P(post_h), None, P(au_h), None))

    def head():
        check(sess.lib.alq_dense_head_fwd(sess.ctx, P(xh), R, Ci, c + 1, P(Wh), P(bh), P(post_h), None))

    cot_au()
    torch.cuda.synchronize()
    ref = mteach.evaluate_au(p[:, :n].cpu().numpy(), q[:, :n].cpu().numpy(), au[:n].cpu().numpy(), lab[:n].cpu().numpy(), mteach.L2, s, k, kau,
                             kappa, cw32, sw[:n].cpu().numpy(), 2.)
    mag = np.abs(ref['labelled_rows']) + np.abs(ref['cons_rows'])
    mag[:, c] = kau * (0.5 * float(np.float32(kappa)) + ref['div'] * np.exp(-au[:n].cpu().numpy().astype(np.float64)))
    err = np.abs(rows_au[:n].cpu().numpy().astype(np.float64) - ref['rows'])
    res['au_row_err_over_bound'] = float((err / np.maximum(4 * 2. ** -24 * mag, 1e-300)).max())
    print('aleatoric cotangent: worst row error / bound %.3f' % res['au_row_err_over_bound'])
    nb = {'mt_cotangent': (8 * c + 8 + 4 * c) * R, 'mt_cotangent_au': (4 * (2 * c + 1) + 8 + 4 * (c + 1)) * R,
          'dense_head_fwd': (4 * Ci + 4 * (c + 1)) * R}
    nb['dense_head_fwd_au'] = nb['dense_head_fwd']
    bufs = {kk: (torch.empty((v // 8,), dtype=torch.float32, device=dev).normal_(), torch.empty((v // 8,), dtype=torch.float32, device=dev))
            for kk, v in nb.items() if kk != 'dense_head_fwd_au'}
    bufs['dense_head_fwd_au'] = bufs['dense_head_fwd']
    fns = {'mt_cotangent': cot, 'mt_cotangent_au': cot_au, 'dense_head_fwd': head, 'dense_head_fwd_au': head_au}
    meds = {kk: [] for kk in list(fns) + ['copy_' + kk for kk in fns]}
    for _ in range(a.rounds):          # alternating rounds: drift of a shared machine falls on every kernel alike
        for kk, fn in fns.items():
            meds[kk].append(timed(torch, fn, a.warmup, a.reps)[0])
            meds['copy_' + kk].append(timed(torch, lambda: bufs[kk][1].copy_(bufs[kk][0]), a.warmup, a.reps)[0])
    au_res = {kk: dict(us_median=float(np.median(v)), us_rounds=[float(t) for t in v], spread=float(max(v) / min(v))) for kk, v in meds.items()}
    for kk in fns:
        au_res[kk].update(bytes=nb[kk], gbps_median=nb[kk] / au_res[kk]['us_median'] / 1e3,
                          ratio_to_copy=au_res[kk]['us_median'] / au_res['copy_' + kk]['us_median'])
    for new, old in (('mt_cotangent_au', 'mt_cotangent'), ('dense_head_fwd_au', 'dense_head_fwd')):
        au_res[new].update(ratio_to_parent=au_res[new]['us_median'] / au_res[old]['us_median'], byte_ratio=nb[new] / nb[old],
                           parent_spread=au_res[old]['spread'])
        print('%s: %.1f us median = %.0f GB/s, kernel / copy %.2f; parent %s %.1f us (kernel / copy %.2f); time ratio %.3f, byte ratio '
              '%.3f, spread of the parent\'s %d round medians %.3f'
              % (new, au_res[new]['us_median'], au_res[new]['gbps_median'], au_res[new]['ratio_to_copy'], old, au_res[old]['us_median'],
                 au_res[old]['ratio_to_copy'], au_res[new]['ratio_to_parent'], au_res[new]['byte_ratio'], a.rounds, au_res[old]['spread']))
    res['aleatoric'] = au_res
    del bufs, p, q, rows, rows_au, xh, post_h, au_h, au

    if not a.skip_step:
        N, in_shape = a.batch, (32, 32, 32, 1)
        ld, sk = netspec.net_c_dense(2)
        pars = netspec.he_init(ld, in_shape, seed=5, skips=sk, bias_std=0.05)
        models = {}
        for name, kw in (('plain', {}), ('mt', dict(MT_SSL=True, output_perturbation_measure='L2', Gaussian_noise_std=0.1, max_cons_coeff=1.,
                                                    rampup_length=100))):
            m = NN_extended.CNN(in_shape, ld, name, list(sk), sess=sess, max_batch=N, optimizer_name='Adam', learning_rate=1e-4, **kw)
            m.set_weights(pars)
            m.get_optimizer()
            models[name] = m
        rs = np.random.RandomState(3)
        x = torch.as_tensor(rs.randn(N, *in_shape).astype(np.float32)).to(dev)
        lab = rs.randint(0, 2, size=(N, 32, 32, 32))
        y = (lab[..., None] == np.arange(2)).astype(np.float32)
        y[rs.rand(N, 32, 32, 32) < 0.3] = 0

        def step(m):
            sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1.})
            if m.MT_SSL:
                sess.run(m.ema_apply)
        times = {'plain': [], 'mt': []}
        for it in range(a.warmup // 2 + 1 + a.reps // 2):
            for name in ('plain', 'mt'):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(models[name])
                torch.cuda.synchronize()
                if it > a.warmup // 2:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        res['step_ms'] = {kk: dict(median=float(np.median(v)), min=float(np.min(v))) for kk, v in times.items()}
        res['step_ms']['ratio'] = res['step_ms']['mt']['median'] / res['step_ms']['plain']['median']
        print('one step of net_c_dense at 32^3, N = %d: plain %.1f ms, mean-teacher (train_step + ema_apply) %.1f ms, ratio %.2f'
              % (N, res['step_ms']['plain']['median'], res['step_ms']['mt']['median'], res['step_ms']['ratio']))
    res.update(R=R, c=c, reps=a.reps, warmup=a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
