#!/usr/bin/env python3
"""Whole-volume inference by tiles on the device (csrc/tile.hip) - the figures DESIGN.md records.

  1. Device against statement (nnal_amd/tiled.py), bit for bit, on a 40 x 44 x 36 volume with 16^3 tiles at stride 8, c = 2.
  2. Time: alq_tile_gather, alq_tile_blend and alq_tile_finalize each on its own on a 160^3 volume, m = 1, c = 2, 32^3 tiles at
     stride 16 (9^3 = 729 tiles) - gather and blend for a pass of `--tiles` tiles and for all tiles in one launch, finalize
     with and without the posteriors - timed with stream events over `--reps` launches after `--warmup`, next to a
     torch.Tensor.copy_ moving the same number of bytes (half read, half written) timed the same way in the same process.
     Bytes: gather 2 x 4 n V m; blend 4 c n V (posteriors) + 2 x 4 (c + 1) box (the accumulator over the call's bounding box, read
     and written - an upper bound: voxels of the box no tile of the call covers are skipped); finalize 4 (c + 1) N read, N bytes
     of labels and 4 c N of posteriors written.
  3. eval_utils.full_volume_segment of NET-C (32^3 input) on that volume against the sum of its forward passes alone.

    python tools/gpu_tiled.py [--reps 20] [--warmup 5] [--tiles 64] [--max-batch 64] [--skip-model] [--out tiled.json]

Prints one JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, warmup, reps):
    """Median and minimum of `reps` single-launch times in microseconds (one event pair per launch)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--tiles', type=int, default=64)
    ap.add_argument('--max-batch', type=int, default=64)
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import device, eval_utils, netspec, tiled
    sess = device.default_session()
    dev = sess.device
    res = {}

    # 1. device against statement
    dims, tile, stride, c = (40, 44, 36), (16, 16, 16), (8, 8, 8), 2
    rs = np.random.RandomState(1)
    lat = sess.tile_lattice(dims, tile, stride)
    nt, V = sess.tile_count(lat), int(np.prod(tile))
    vol = rs.randn(*dims, 1).astype(np.float32)
    X = sess.tile_gather(sess.to_device(vol, torch.float32), lat, 0, nt)
    ok_gather = X.cpu().numpy().tobytes() == tiled.gather_host(vol, tile, stride).tobytes()
    p = rs.rand(c, nt * V) + 0.01
    post = (p / p.sum(0, keepdims=True)).astype(np.float32)
    wins_h = [tiled.window('gaussian', t) for t in tile]
    wins = tuple(sess.to_device(w, torch.float32) for w in wins_h)
    acc = torch.zeros((c + 1,) + dims, dtype=torch.float32, device=dev)
    for first in range(0, nt, 50):
        n = min(50, nt - first)
        sess.tile_blend(sess.to_device(np.ascontiguousarray(post.reshape(c, nt, V)[:, first:first + n]).reshape(c, n * V), torch.float32), lat,
                        first, n, wins, acc)
    want = tiled.blend_host(np.zeros((c + 1,) + dims, dtype=np.float32), post, tile, stride, *wins_h)
    ok_blend = acc.cpu().numpy().tobytes() == want.tobytes()
    q, lab = tiled.finalize_host(want, hwz=True)
    dq, dl = sess.tile_finalize(acc, hwz=True)
    ok_fin = dq.cpu().numpy().tobytes() == q.tobytes() and dl.cpu().numpy().tobytes() == lab.tobytes()
    res['equal_bits'] = dict(gather=ok_gather, blend=ok_blend, finalize=ok_fin, tiles=nt)
    print('device == statement, bit for bit, %d tiles: gather %s, blend (cuts of 50) %s, finalize %s' % (nt, ok_gather, ok_blend, ok_fin))

    # 2. the launches alone
    dims, tile, stride, c, m = (160, 160, 160), (32, 32, 32), (16, 16, 16), 2, 1
    N, V = int(np.prod(dims)), int(np.prod(tile))
    lat = sess.tile_lattice(dims, tile, stride)
    nt = sess.tile_count(lat)
    vol = torch.randn(dims + (m,), device=dev)
    wins = tuple(sess.to_device(tiled.window('gaussian', t), torch.float32) for t in tile)
    acc = torch.zeros((c + 1,) + dims, dtype=torch.float32, device=dev)
    counts = tiled.tile_counts(dims, tile, stride)
    launches = []
    for n in sorted({min(a.tiles, nt), nt}):
        X = sess.empty((n,) + tile + (m,), torch.float32)
        post = torch.rand((c, n * V), device=dev)
        # the bounding box of tiles 0 .. n - 1 (as the library takes it: whole faster axes once a slower index changes)
        last = n - 1
        iz, ih, iw = last // (counts[1] * counts[2]), (last // counts[2]) % counts[1], last % counts[2]
        oz, oh, ow = (tiled.lattice_origins(D, t, s) for D, t, s in zip(dims, tile, stride))
        bz = int(oz[iz]) + tile[0]
        bh = dims[1] if iz > 0 else int(oh[ih]) + tile[1]
        bw = dims[2] if (iz > 0 or ih > 0) else int(ow[iw]) + tile[2]
        box = bz * bh * bw
        launches.append(('gather n=%d' % n, lambda X=X, n=n: sess.tile_gather(vol, lat, 0, n, out=X), 2 * 4 * n * V * m))
        launches.append(('blend n=%d' % n, lambda post=post, n=n: sess.tile_blend(post, lat, 0, n, wins, acc), 4 * c * n * V + 8 * (c + 1) * box))
    fq = sess.empty((c,) + dims, torch.float32)
    fl = sess.empty(dims, torch.uint8)
    launches.append(('finalize hwz labels', lambda: sess.tile_finalize(acc, hwz=True, want_post=False, label=fl), 4 * (c + 1) * N + N))
    launches.append(('finalize hwz labels+posteriors', lambda: sess.tile_finalize(acc, hwz=True, post=fq, label=fl), 4 * (c + 1) * N + N + 4 * c * N))
    launches.append(('finalize zhw labels+posteriors', lambda: sess.tile_finalize(acc, hwz=False, post=fq, label=fl), 4 * (c + 1) * N + N + 4 * c * N))
    res['launches'] = {}
    for name, fn, nbytes in launches:
        half = nbytes // 2 // 16 * 16
        src = torch.empty((half // 4,), dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        med, best = timed(torch, fn, a.warmup, a.reps)
        cmed, cbest = timed(torch, lambda: dst.copy_(src), a.warmup, a.reps)
        res['launches'][name] = dict(us_median=med, us_min=best, bytes=nbytes, gbps_median=nbytes / med / 1e3, copy_us_median=cmed,
                                     copy_us_min=cbest, ratio_to_copy=med / cmed)
        print('%s: %.1f us median (%.1f min) for %.1f MB = %.0f GB/s; copy of the same bytes %.1f us median (%.1f min); kernel / copy = %.2f'
              % (name, med, best, nbytes / 1e6, nbytes / med / 1e3, cmed, cbest, med / cmed))
        del src, dst
    del acc, fq, fl

    # 3. the whole call against its forward passes
    if not a.skip_model:
        from nnal_amd.datasets.utils import ResidentSubject
        ld, sk = netspec.net_c_dense(2)
        in_shape = tile + (m,)
        model = device.DeviceModel(sess, ld, in_shape, sk, max_batch=a.max_batch)
        model.set_weights(netspec.he_init(ld, in_shape, seed=5, skips=sk, bias_std=0.05))
        subject = ResidentSubject(sess, vol, None)
        X = sess.tile_gather(vol, lat, 0, min(model.max_batch, nt))

        def forwards():
            for first in range(0, nt, model.max_batch):
                n = min(model.max_batch, nt - first)
                model.forward_maps_device(X[:n], n)

        def whole():
            eval_utils.full_volume_segment(model, sess, subject, keep_on_device=True)

        out = {}
        for name, fn in (('forward passes', forwards), ('full_volume_segment', whole)):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            out[name] = float(np.median(ts))
            print('%s: %.1f ms (median of 3), %d tiles in passes of %d' % (name, 1e3 * out[name], nt, model.max_batch))
        res['whole'] = dict(forward_ms=1e3 * out['forward passes'], segment_ms=1e3 * out['full_volume_segment'],
                            ratio=out['full_volume_segment'] / out['forward passes'], tiles=nt, max_batch=model.max_batch)
        print('full_volume_segment / forward passes = %.3f' % res['whole']['ratio'])
        model.close()
    res.update(reps=a.reps, warmup=a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
