#!/usr/bin/env python3
"""Times the dense CRF of csrc/dcrf.hip (alq_dcrf2d) on one MI355X and measures its deviation from the fp64 restatement.

    python tools/gpu_dcrf.py [--runs 20] [--out profiles/dcrf.json] [--design DESIGN.md]
    python tools/gpu_dcrf.py --from-json profiles/dcrf.json --design DESIGN.md          (no GPU: renders a stored result)

For [S, H, W] = 32 x 256 x 256 and 8 x 512 x 512 (scenes of tests/dcrf_cases.py, one seed per slice): the device time of one
alq_dcrf2d call with 1 and with 5 iterations, each run between its own pair of device events, the median over `--runs` runs
after 3 warm-up calls.  One iteration = one filter launch = (t_5 - t_1) / 4; the two set-up launches (normalisation sums, per-pixel
constants) are filter launches of the same cost.  Beside it the host's time for the same filter on ONE slice:
dcrf.meanfield_host's windowed float32 form (window='cutoff'), one application to both label planes, timed once.

The filter launch against its vector-issue floor: taps (pixels x the 59 x 59 appearance window) x the issue cycles of one tap
/ 64 lanes / 1024 SIMDs / 2.4 GHz.  The cycles per tap are counted on the device assembly of the kernel's inner loop (16 taps
per trip: 16 v_sub_f32, 16 v_fma_f32, 8 v_pk_fma_f32, 4 v_readlane_b32, 4 v_mov_b32, 1 v_lshl_add_u32 at 4 issue cycles each and
16 v_exp_f32 at 8: 324 cycles, 20.25 per tap); the launch evaluates 62 x 60 window positions per pixel instead of 59 x 59 (rows
shared by the 4 outputs of a wave, columns in steps of four) and the 13 x 13 smoothness taps on top.

Then, on the shapes of tests/test_gpu_dcrf.py: max |q1_device - Q_1,fp64 all pairs| after 1 and 5 iterations, the fp32 host
restatement's deviation on the same input and their ratio.  Prints one JSON line; --design rewrites the table between the
`<!-- dcrf-table -->` markers of that file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAP_ISSUE_CYCLES = 324. / 16.
SIMDS, LANES, CLOCK = 1024, 64, 2.4e9
MARK = '<!-- dcrf-table -->'


def render(res):
    rows = ['| shape [S, H, W] | call, 5 iterations | per slice | one filter launch | per slice and iteration | host fp32 windowed filter, one slice | '
            'issue floor of a launch | launch / floor |', '|---|---|---|---|---|---|---|---|']
    for c in res['timing']:
        rows.append('| %d x %d x %d | %.3f ms [%.3f, %.3f] | %.1f us | %.1f us | %.2f us | %.2f s (%.0f x) | %.1f us | %.2f |' % (
            c['dims'][0], c['dims'][1], c['dims'][2], c['call5_s'] * 1e3, c['call5_s_min'] * 1e3, c['call5_s_max'] * 1e3,
            c['call5_s'] / c['dims'][0] * 1e6, c['launch_s'] * 1e6, c['launch_s'] / c['dims'][0] * 1e6, c['host_filter_s'],
            c['host_filter_s'] / (c['launch_s'] / c['dims'][0]), c['floor_s'] * 1e6, c['launch_s'] / c['floor_s']))
    rows += ['', '| test shape | iterations | device vs fp64 | fp32 host vs fp64 | ratio | tol = 4 x fp32 host + 1e-6 |', '|---|---|---|---|---|---|']
    for d in res['deviation']:
        rows.append('| %d x %d x %d | %d | %.2e | %.2e | %s | %.2e |' % (
            d['shape'][0], d['shape'][1], d['shape'][2], d['niter'], d['device'], d['host32'],
            '%.2f' % (d['device'] / d['host32']) if d['host32'] > 1e-9 else '-', d['tol']))
    return '\n'.join(rows)


def write_design(path, res):
    text = open(path).read()
    a = text.index(MARK) + len(MARK)
    b = text.index(MARK, a)
    open(path, 'w').write(text[:a] + '\n' + render(res) + '\n' + text[b:])


def measure(runs):
    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import _lib, dcrf, device
    from tests import dcrf_cases as dc
    sess = device.DeviceSession(0)
    sess.bind_stream()
    L, ctx = sess.lib, sess.ctx
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731

    def cpar(niter):
        return _lib.DcrfParams((C.c_float * 2)(1., 1.), (C.c_float * 2)(5., 5.), 1., 20., 30., niter)

    def run(post, img, niter):
        dims = tuple(post.shape)
        cd = (C.c_int64 * 3)(*dims)
        d_post, d_img = sess.to_device(post, torch.float32), sess.to_device(img, torch.float32)
        q = sess.empty(dims, torch.float32)
        mp = sess.empty(dims, torch.uint8)
        work = sess.empty((int(L.alq_dcrf_work_bytes(cd)),), torch.uint8)
        par = cpar(niter)

        def fn():
            assert L.alq_dcrf2d(ctx, p(d_post), p(d_img), cd, C.byref(par), p(q), p(mp), p(work)) == 0, L.alq_last_error()
        return fn, q, mp

    def time_call(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    res = dict(tool='gpu_dcrf', runs=runs, tap_issue_cycles=TAP_ISSUE_CYCLES, timing=[], deviation=[])
    for S, H, W in ((32, 256, 256), (8, 512, 512)):
        scenes = [dc.scene(H, W, 100 + s) for s in range(S)]
        img = np.stack([s[1] for s in scenes]).astype(np.float32)
        post = np.stack([s[2] for s in scenes]).astype(np.float32)
        fn5, q5, m5 = run(post, img, 5)
        fn1, _, _ = run(post, img, 1)
        t5, lo5, hi5 = time_call(fn5)
        t1, _, _ = time_call(fn1)
        launch = (t5 - t1) / 4.
        taps = float(S) * H * W * 59 * 59
        floor = taps * TAP_ISSUE_CYCLES / LANES / SIMDS / CLOCK
        flt, _ = dcrf.make_filter(img[0], np.float32, 'cutoff')
        Q = dcrf.meanfield_host(post[0].copy(), img[0], np.float32, 'cutoff', niter=0, _filter=(flt, dcrf.make_params()))[0]
        t0 = time.perf_counter()
        flt.apply(Q)
        host = time.perf_counter() - t0
        c = dict(dims=[S, H, W], call5_s=t5, call5_s_min=lo5, call5_s_max=hi5, call1_s=t1, launch_s=launch, taps_per_launch=taps,
                 floor_s=floor, host_filter_s=host, labelled_one=float(m5.float().mean().item()))
        res['timing'].append(c)
        print('%d x %d x %d: call(5) %.3f ms, call(1) %.3f ms, one filter launch %.1f us, floor %.1f us (x %.2f), host filter of one slice %.2f s'
              % (S, H, W, t5 * 1e3, t1 * 1e3, launch * 1e6, floor * 1e6, launch / floor, host), flush=True)
    for shape in sorted(dc.GPU_SHAPES):
        for niter in (1, 5):
            fn, q, _ = run(dc.stacked(shape, 'post'), dc.stacked(shape, 'img'), niter)
            fn()
            dev = float(np.abs(q.cpu().numpy().astype(np.float64) - dc.q1_stack(shape, np.float64, niter)).max())
            tol, host32 = dc.tolerance(shape, niter)
            res['deviation'].append(dict(shape=list(shape), niter=niter, device=dev, host32=host32, tol=tol))
            print('%r niter %d: device %.3e, fp32 host %.3e, tol %.3e' % (shape, niter, dev, host32, tol), flush=True)
    sess.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--design', default=None, help='file whose <!-- dcrf-table --> block is rewritten')
    ap.add_argument('--from-json', default=None, help='render a stored result instead of measuring')
    a = ap.parse_args()
    res = json.loads(open(a.from_json).read()) if a.from_json else measure(max(a.runs, 5))
    line = json.dumps(res)
    print(render(res))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if a.design:
        write_design(a.design, res)


if __name__ == '__main__':
    main()
