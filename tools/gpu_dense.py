#!/usr/bin/env python3
"""Fully-convolutional models on the device (csrc/dense.hip) - the figures DESIGN.md records.

  1. Accuracy: every case of tests/test_gpu_dense.py (head alone and whole nets) against the fp64 torch restatement; the
     cases print their own lines, the tool adds the largest e_dev / e_32 of the gradients.
  2. Time: dense_head_fwd and dense_head_bwd (the latter with its reduce launch) on their own (alq_dense_head_fwd / _bwd) at
     32^3 voxels x N = 64, Ci = 8, c = 2, timed with stream events over `--reps` launches after `--warmup`, next to a
     device-to-device copy moving the same number of bytes (half read, half written) timed the same way in the same process.

    python tools/gpu_dense.py [--reps 20] [--warmup 5] [--skip-accuracy] [--out dense.json]

Prints one JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import sys

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
    ap.add_argument('--skip-accuracy', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import device, netspec
    from nnal_amd._lib import check
    sess = device.default_session()
    res = {}

    if not a.skip_accuracy:
        from tests import test_gpu_dense as T
        worst = 0.
        for shape in sorted(T.HEAD_SHAPES):
            in_shape, N = T.HEAD_SHAPES[shape]
            for ci in (4, 8, 12, 16, 20, 64):
                for c in (2, 3, 8):
                    ld, sk = T._head_net(ci, c, len(in_shape) - 1)
                    worst = max(worst, T._check_case(sess, 'head %s Ci=%d c=%d' % (shape, ci, c), ld, sk, in_shape, N, c, 300 + ci + c, 4))
        for net in sorted(T.NETS):
            fn, c, in_shape, N, seed = T.NETS[net]
            ld, sk = getattr(netspec, fn)(c)
            worst = max(worst, T._check_case(sess, 'net %s' % net, ld, sk, in_shape, N, c, seed, 8))
        res['max_grad_err_ratio_dev_over_fp32'] = worst
        print('largest e_dev / e_32 over all cases and objective variants: %.2f' % worst)

    N, V, Ci, c = 64, 32 ** 3, 8, 2
    R = N * V
    dev = sess.device
    g = torch.Generator(device='cpu').manual_seed(7)
    x = torch.randn((R, Ci), generator=g).to(dev)
    W = (0.5 * torch.randn((Ci, c), generator=g)).to(dev)
    b = (0.05 * torch.randn((c,), generator=g)).to(dev)
    delta = (torch.randn((R, c), generator=g) / R).to(dev)
    post = torch.empty((c, R), dtype=torch.float32, device=dev)
    dx = torch.empty((R, Ci), dtype=torch.float32, device=dev)
    gout = torch.empty((Ci * c + c,), dtype=torch.float32, device=dev)
    work = torch.empty((sess.lib.alq_dense_head_work_bytes(Ci, c),), dtype=torch.uint8, device=dev)
    sess.bind_stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def fwd():
        check(sess.lib.alq_dense_head_fwd(sess.ctx, P(x), R, Ci, c, P(W), P(b), P(post), None))

    def bwd():
        check(sess.lib.alq_dense_head_bwd(sess.ctx, P(delta), P(x), R, Ci, c, P(W), P(dx), P(work), P(gout)))

    # what the kernels computed at this size, against torch in fp64 on a slice (the whole tensors for the sums)
    fwd()
    bwd()
    torch.cuda.synchronize()
    sl = slice(0, 1 << 16)
    p64 = torch.softmax(x[sl].double() @ W.double() + b.double(), dim=1).t()
    res['post_err_32cube'] = float((post[:, sl].double() - p64).abs().max())
    res['dx_err_32cube'] = float((dx[sl].double() - delta[sl].double() @ W.double().t()).abs().max() / (delta[sl].abs().max() * W.abs().max()))
    gw = torch.cat([(x.double().t() @ delta.double()).reshape(-1), delta.double().sum(0)])
    res['dw_rel_err_32cube'] = float((gout.double() - gw).abs().max() / gw.abs().max())
    print('32^3 x 64: |post - post64| %.3e, dX error / (max|delta| max|W|) %.3e, [dW, db] error / max %.3e'
          % (res['post_err_32cube'], res['dx_err_32cube'], res['dw_rel_err_32cube']))

    for name, fn, nbytes in (('dense_head_fwd', fwd, 4 * R * (Ci + c)), ('dense_head_bwd', bwd, 4 * R * (2 * Ci + c))):
        half = nbytes // 2 // 16 * 16
        src = torch.empty((half // 4,), dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        med, best = timed(torch, fn, a.warmup, a.reps)
        cmed, cbest = timed(torch, lambda: dst.copy_(src), a.warmup, a.reps)
        res[name] = dict(us_median=med, us_min=best, bytes=nbytes, gbps_median=nbytes / med / 1e3, copy_us_median=cmed, copy_us_min=cbest,
                         copy_gbps_median=2 * half / cmed / 1e3, ratio_to_copy=med / cmed)
        print('%s: %.1f us median (%.1f min) for %.1f MB = %.0f GB/s; copy of the same bytes %.1f us median (%.1f min) = %.0f GB/s; '
              'kernel / copy = %.2f' % (name, med, best, nbytes / 1e6, nbytes / med / 1e3, cmed, cbest, 2 * half / cmed / 1e3, med / cmed))
        del src, dst
    res.update(N=N, voxels=V, Ci=Ci, c=c, reps=a.reps, warmup=a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
