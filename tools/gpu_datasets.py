#!/usr/bin/env python3
"""Resident volumes and device-built batches (csrc/volbatch.hip, nnal_amd.datasets) - the figures DESIGN.md section 7 records.

  1. Device against the NumPy statement at full size: alq_vol_pack of a 256 x 256 x 150 subject of two int16 modalities, and one
     alq_slice_batch of each shape below, bit for bit.
  2. Time of single launches between stream events (`--reps` after `--warmup`, medians of `--rounds` alternating rounds), each
     beside a device-to-device copy of the bytes the kernel must move, in the same process:
       * alq_vol_pack of that subject from float32 sources (4 bytes read and 4 written per voxel and modality);
       * alq_slice_batch of 2 blocks of 192 x 192 x 64 (per voxel: 4 m read and written, 1 mask byte read, 4 label bytes written);
       * alq_slice_batch of 8 slices of 256 x 256: launch-bound, reported as a time beside the smallest call of the same entry
         (one 1 x 1 x 1 window: the memset of the counts and an almost empty launch).
  3. One `train_gen_fn()` plus one dense train step of net_c_2d_dense on batches of 8 slices of 256 x 256 x 2, fed the device way
     (resident subjects, DeviceLabels) against the same step fed the NumPy statement's host arrays through the host path,
     alternating, host clock around a device synchronise, medians of the steady-state steps.

    python tools/gpu_datasets.py [--reps 20] [--warmup 5] [--rounds 5] [--steps 12] [--skip-step] [--out datasets.json]

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

SHAPE, M, NCLASS = (256, 256, 150), 2, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import NN_extended, device, netspec
    from nnal_amd._lib import check
    from nnal_amd.datasets import data_holders, utils
    sess = device.default_session()
    dev = sess.device
    res = {}
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    H, W, Z = SHAPE
    rs = np.random.RandomState(7)
    vols = [rs.randint(-500, 3000, size=SHAPE).astype(np.int16) for _ in range(M)]
    ids = rs.randint(0, NCLASS + 1, size=SHAPE).astype(np.uint8)
    ids[ids == NCLASS] = utils.NO_CLASS

    # ---- 1. the statement
    sub = utils.ResidentSubject.pack(sess, vols, ids)
    want_vol = np.stack([v.transpose(2, 0, 1) for v in vols], -1).astype(np.float32)
    want_ids = np.ascontiguousarray(ids.transpose(2, 0, 1))
    res['pack_equal'] = bool(np.array_equal(sub.vol.cpu().numpy(), want_vol) and np.array_equal(sub.mask.cpu().numpy(), want_ids))
    shapes = {'blocks_2x192x192x64': ((64, 192, 192), [(0, 40, 10, 33, 1), (0, 100, 64, 1, 0)]),
              'slices_8x256x256': ((1, 256, 256), [(0, 5 + 17 * i, 0, 0, i % 2) for i in range(8)])}
    for name, (crop, desc) in shapes.items():
        X, lab, cnt = utils.slice_batch(sess, [sub], desc, crop, NCLASS)
        z, h, w = crop
        wX = np.stack([want_vol[zc - z // 2:zc - z // 2 + z, h0:h0 + h, w0:w0 + w] for _, zc, h0, w0, _ in desc])
        wl = np.stack([want_ids[zc - z // 2:zc - z // 2 + z, h0:h0 + h, w0:w0 + w].astype(np.int32) if L else np.full(crop, -1, np.int32)
                       for _, zc, h0, w0, L in desc])
        wl[wl >= NCLASS] = -1
        wc = [int((wl == j).sum()) for j in range(NCLASS)] + [int((wl < 0).sum())]
        res[name + '_equal'] = bool(np.array_equal(X.cpu().numpy(), wX) and np.array_equal(lab.cpu().numpy(), wl) and cnt.cpu().numpy().tolist() == wc)
    print('device against the NumPy statement: pack %s, batches %s' % (res['pack_equal'], {k: v for k, v in res.items() if k != 'pack_equal'}))

    # ---- 2. launches
    src = [torch.as_tensor(v.astype(np.float32)).to(dev) for v in vols]
    out = torch.empty((Z, H, W, M), dtype=torch.float32, device=dev)
    dims = (C.c_int32 * 3)(H, W, Z)
    ptrs = (C.c_void_p * M)(*[t.data_ptr() for t in src])
    sess.bind_stream()

    def pack():
        check(sess.lib.alq_vol_pack(sess.ctx, ptrs, M, 0, dims, P(out)))

    def batch_fn(name):
        crop, desc = shapes[name]
        b = len(desc)
        bufs = (torch.empty((b,) + crop + (M,), dtype=torch.float32, device=dev), torch.empty((b,) + crop, dtype=torch.int32, device=dev),
                torch.empty((NCLASS + 1,), dtype=torch.int64, device=dev))
        return lambda: utils.slice_batch(sess, [sub], desc, crop, NCLASS, out=bufs)

    def copy_fn(nbytes):
        s_ = torch.empty((nbytes // 8,), dtype=torch.float32, device=dev).normal_()
        d_ = torch.empty_like(s_)
        return lambda: d_.copy_(s_)

    vox = {'blocks_2x192x192x64': 2 * 64 * 192 * 192, 'slices_8x256x256': 8 * 256 * 256}
    nb = {'vol_pack': 8 * H * W * Z * M}
    nb.update({k: (8 * M + 5) * v for k, v in vox.items()})
    tiny = lambda: utils.slice_batch(sess, [sub], [(0, 0, 0, 0, 1)], (1, 1, 1), NCLASS)      # noqa: E731
    fns = {'vol_pack': pack, 'blocks_2x192x192x64': batch_fn('blocks_2x192x192x64'), 'slices_8x256x256': batch_fn('slices_8x256x256'),
           'smallest_call': tiny}
    fns.update({'copy_' + k: copy_fn(v) for k, v in nb.items()})
    meds = {k: [] for k in fns}
    for _ in range(a.rounds):          # alternating rounds: drift of a shared machine falls on every kernel alike
        for k, fn in fns.items():
            meds[k].append(timed(torch, fn, a.warmup, a.reps)[0])
    t = {k: dict(us_median=float(np.median(v)), us_rounds=[float(x) for x in v], spread=float(max(v) / min(v))) for k, v in meds.items()}
    for k, v in nb.items():
        t[k].update(bytes=v, gbps_median=v / t[k]['us_median'] / 1e3, ratio_to_copy=t[k]['us_median'] / t['copy_' + k]['us_median'])
        print('%s: %.1f us median = %.0f GB/s over %.1f MB; copy of the same bytes %.1f us; kernel / copy %.2f'
              % (k, t[k]['us_median'], t[k]['gbps_median'], v / 1e6, t['copy_' + k]['us_median'], t[k]['ratio_to_copy']))
    print('slices_8x256x256 (host entry included) %.1f us beside the smallest call of the entry %.1f us'
          % (t['slices_8x256x256']['us_median'], t['smallest_call']['us_median']))
    res['launches'] = t
    del src, out, fns

    # ---- 3. generator + step
    if not a.skip_step:
        n_sub, b = 3, 8
        table, img_addrs, mask_addrs = {}, {'T1': [], 'T2': []}, []
        for s in range(n_sub):
            for mod in img_addrs:
                p = 'sub%d_%s' % (s, mod)
                table[p] = vols[0] if (s == 0 and mod == 'T1') else rs.randint(-500, 3000, size=SHAPE).astype(np.int16)
                img_addrs[mod].append(p)
            table['mask%d' % s] = rs.randint(0, NCLASS, size=SHAPE).astype(np.uint8)
            mask_addrs.append('mask%d' % s)
        luv = [np.array([0, 1]), np.array([2]), np.array([], dtype=int)]
        holders = {}
        for way in ('host', 'device'):
            dat = data_holders.regular({k: list(v) for k, v in img_addrs.items()}, list(mask_addrs), lambda p: table[p], None, luv, np.arange(NCLASS))
            dat.load_images(sess if way == 'device' else None)
            np.random.seed(5)
            dat.create_train_valid_gens(b, [H, W], n_labeled_train=b // 2)
            holders[way] = dat
        in_shape = (H, W, M)
        ld, sk = netspec.net_c_2d_dense(NCLASS)
        pars = netspec.he_init(ld, in_shape, seed=5, skips=sk, bias_std=0.05)
        models = {}
        for way in holders:
            m = NN_extended.CNN(in_shape, ld, way, list(sk), sess=sess, max_batch=b, optimizer_name='Adam', learning_rate=1e-4)
            m.set_weights(pars)
            m.get_optimizer()
            models[way] = m
        times = {way: dict(gen=[], step=[], both=[]) for way in holders}
        warm = max(2, a.steps // 4)
        for it in range(warm + a.steps):
            for way in ('host', 'device'):
                m = models[way]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X, Y = holders[way].train_gen_fn()
                if way == 'host':
                    X = X.astype(np.float32)          # (the feed of the reference's float32 placeholder)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                sess.run(m.train_step, feed_dict={m.x: X, m.y_: Y, m.keep_prob: 1.})
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if it >= warm:
                    times[way]['gen'].append((t1 - t0) * 1e3)
                    times[way]['step'].append((t2 - t1) * 1e3)
                    times[way]['both'].append((t2 - t0) * 1e3)
        res['step_ms'] = {way: {k: dict(median=float(np.median(v)), min=float(np.min(v))) for k, v in d.items()} for way, d in times.items()}
        res['step_ms']['ratio_host_over_device'] = res['step_ms']['host']['both']['median'] / res['step_ms']['device']['both']['median']
        for way in ('host', 'device'):
            d = res['step_ms'][way]
            print('%s feed, %d slices of %d x %d x %d: generator %.2f ms + train step %.2f ms = %.2f ms (medians of %d steps)'
                  % (way, b, H, W, M, d['gen']['median'], d['step']['median'], d['both']['median'], a.steps))
        print('host / device: %.2f' % res['step_ms']['ratio_host_over_device'])
    res.update(shape=list(SHAPE), m=M, reps=a.reps, warmup=a.warmup, rounds=a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
