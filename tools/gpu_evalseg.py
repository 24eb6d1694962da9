#!/usr/bin/env python3
"""Segmentation evaluation on the device (csrc/confusion.hip, csrc/ccl.hip, nnal_amd.eval_utils, nnal_amd.datasets.lesion_utils) -
the figures DESIGN.md section 7 records.

  1. Device against NumPy for each entry point: alq_confusion_counts in its four uses, eval_full_segs_explicit_partitions /
     _label_percentage with a session against their NumPy path, alq_cc_sizes / alq_cc_relabel and the lesion functions against the
     host statement.
  2. alq_confusion_counts, single launches between stream events (`--reps` after `--warmup`, medians of `--rounds` alternating
     rounds), each beside a torch device-to-device copy of the bytes the kernel reads, in the same process: 2 M uint8 pairs (a
     128 x 128 x 128 volume) and 64 x 32^3 int64 / int32 pairs; groups = 1 and per slice (inner = 1, groups = 128 / 32); C = 2 and
     8; one input with 95 % background and one uniform-random.
  3. eval_metrics: `--iters` iterations of net_c_2d_dense at 64 x 64, batch 8, c = 3, fed from a `datasets` generator of resident
     subjects - the device path against the host path (sess.run(model.posteriors), np.asarray(DeviceLabels), two argmax: what
     eval_metrics did for this model before the device path existed) on the same batches (drawn from the generator once), alternating; host clock
     around a device synchronise; and the bytes each copies to the host per call.
  4. find_lesion_components at 128 x 128 x 64, density 0.35, against the host statement (scipy.ndimage.label).

    python tools/gpu_evalseg.py [--reps 20] [--warmup 5] [--rounds 5] [--iters 50] [--out evalseg.json]

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


def numpy_counts(pred, lab, C, inner, groups, first=0, fill=-1):
    p, t = pred.astype(np.int64), lab.astype(np.int64)
    g = ((first + np.arange(len(p), dtype=np.int64)) // inner) % groups
    if 0 <= fill < C:
        t = np.where((t < 0) | (t >= C), fill, t)
    ok = (t >= 0) & (t < C) & (p >= 0) & (p < C)
    return np.bincount(((g * C + t) * C + p)[ok], minlength=groups * C * C).reshape(groups, C, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import NN_extended, device, eval_utils, netspec, regions
    from nnal_amd._lib import check
    from nnal_amd.datasets import data_holders, lesion_utils
    sess = device.default_session()
    dev = sess.device
    res = {}
    rs = np.random.RandomState(11)

    # ---- 1. device against NumPy
    eq = {}
    n = 3 * 40 * 36
    pred, lab = rs.randint(0, 4, size=n), rs.randint(-1, 3, size=n)
    for name, inner, groups, first, fill in (('whole', n, 1, 0, 0), ('per_sample', 40 * 36, 3, 0, -1), ('per_slice', 1, 36, 5, 0),
                                             ('packed', 40 * 3, 36, 0, 2)):
        for pt, lt in ((torch.int64, torch.int32), (torch.uint8, torch.uint8)):
            dp, dl = sess.to_device(pred, pt), sess.to_device(lab, lt)
            got = sess.confusion_counts(dp, dl, 3, inner=inner, groups=groups, first=first, fill=fill).cpu().numpy()
            want = numpy_counts(dp.cpu().numpy(), dl.cpu().numpy(), 3, inner, groups, first, fill)
            eq['confusion_%s_%s' % (name, str(pt).split('.')[-1])] = bool(np.array_equal(got, want))
    shape = (64, 56, 48)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[10:50, 8:48, 10:38] = 1
    mask[20:40, 20:40, 18:30] = 2
    mask[:8] = 1
    seg = mask.copy()
    flip = rs.rand(*shape) < 0.1
    seg[flip] = rs.randint(0, 3, size=int(flip.sum()))
    d_, h_ = (eval_utils.eval_full_segs_explicit_partitions([seg], [mask], [[12, 30]], sess=s) for s in (sess, None))
    eq['explicit_partitions'] = bool(np.array_equal(d_[0], h_[0]) and np.array_equal(d_[1], h_[1]))
    d_, h_ = (eval_utils.eval_full_segs_label_percentage([seg], [mask], 1, 0.3, sess=s) for s in (sess, None))
    eq['label_percentage'] = bool(np.array_equal(d_[0], h_[0]) and np.array_equal(d_[1], h_[1]) and np.all(d_[1] > 0))
    big = (rs.rand(128, 128, 64) < 0.35).astype(np.uint8)
    big[0, 0, 0] = 0
    hl = regions.cc_label_host(big, 26)
    roots, cnt = np.unique(hl[hl >= 0], return_counts=True)
    want_sizes = np.zeros(big.size, dtype=np.int32)
    want_sizes[roots] = cnt
    d_lab = sess.cc_label(sess.to_device(big, torch.uint8), big.shape, 26)
    d_sizes = sess.cc_sizes(d_lab)
    eq['cc_sizes'] = bool(np.array_equal(d_sizes.cpu().numpy().reshape(-1), want_sizes))
    eq['cc_relabel'] = bool(np.array_equal(sess.cc_relabel(d_lab, sizes=d_sizes, min_size=5).cpu().numpy().reshape(-1),
                                           (hl.reshape(-1) >= 0) & (want_sizes[np.maximum(hl.reshape(-1), 0)] >= 5)))
    t0 = time.perf_counter()
    host_ranks = lesion_utils.find_lesion_components_host(big)
    t_host = time.perf_counter() - t0
    eq['find_lesion_components'] = bool(np.array_equal(lesion_utils.find_lesion_components(big, sess=sess), host_ranks))
    eq['drop_lesions_with_threshold'] = bool(np.array_equal(lesion_utils.drop_lesions_with_threshold(big, 6, sess=sess),
                                                            lesion_utils.drop_lesions_with_threshold_host(big, 6)))
    res['equal'] = eq
    print('device against NumPy: %s' % eq)
    assert all(eq.values()), eq

    # ---- 2. alq_confusion_counts beside a copy of the same bytes
    def inputs(n, C, kind, pt, lt):
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        if kind == 'uniform':
            p, t = torch.randint(0, C, (n,), generator=g, device=dev), torch.randint(0, C, (n,), generator=g, device=dev)
        else:                                          # 95 % background: both maps 0 there, a lesion class elsewhere, 1 % disagreement
            fg = torch.rand((n,), generator=g, device=dev) < 0.05
            t = torch.where(fg, torch.randint(1, C, (n,), generator=g, device=dev), 0)
            p = torch.where(torch.rand((n,), generator=g, device=dev) < 0.01, torch.randint(0, C, (n,), generator=g, device=dev), t)
        return p.to(pt).contiguous(), t.to(lt).contiguous()

    def copy_fn(nbytes):
        s_ = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev).normal_()
        d_ = torch.empty_like(s_)
        return lambda: d_.copy_(s_)

    fns, nbytes = {}, {}
    keep = []
    ids = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}
    sess.bind_stream()
    for tag, n, slices, pt, lt in (('u8_128cube', 128 ** 3, 128, torch.uint8, torch.uint8), ('i64_i32_64x32cube', 64 * 32 ** 3, 32, torch.int64, torch.int32)):
        per = (1 if pt == torch.uint8 else 8) + (1 if lt == torch.uint8 else 4)
        fns['copy_' + tag] = copy_fn(n * per)
        for C in (2, 8):
            for kind in ('background', 'uniform'):
                p, t = inputs(n, C, kind, pt, lt)
                keep.append((p, t))
                for gname, inner, groups in (('groups1', n, 1), ('per_slice', 1, slices)):
                    counts = torch.zeros((groups, C, C), dtype=torch.int64, device=dev)
                    key = '%s_C%d_%s_%s' % (tag, C, kind, gname)
                    args = (sess.ctx, ct.c_void_p(p.data_ptr()), ids[pt], ct.c_void_p(t.data_ptr()), ids[lt], n, 0, inner, groups, C, -1,
                            ct.c_void_p(counts.data_ptr()), None)
                    fns[key] = lambda args=args: check(sess.lib.alq_confusion_counts(*args))      # the C entry itself: no Python around it
                    nbytes[key] = (n * per, 'copy_' + tag)
                    want = numpy_counts(p.cpu().numpy(), t.cpu().numpy(), C, inner, groups)
                    fns[key]()
                    assert np.array_equal(counts.cpu().numpy(), want), key
                    counts.zero_()
    meds = {k: [] for k in fns}
    for _ in range(a.rounds):          # alternating rounds: drift of a shared machine falls on every kernel alike
        for k, fn in fns.items():
            meds[k].append(timed(torch, fn, a.warmup, a.reps)[0])
    t = {k: dict(us_median=float(np.median(v)), us_rounds=[float(x) for x in v], spread=float(max(v) / min(v))) for k, v in meds.items()}
    for k, (nb, ck) in nbytes.items():
        t[k].update(bytes=nb, gbps_median=nb / t[k]['us_median'] / 1e3, ratio_to_copy=t[k]['us_median'] / t[ck]['us_median'])
        print('%-48s %8.1f us median = %6.0f GB/s read; copy of the same bytes %7.1f us (spread %.2f); kernel / copy %.2f'
              % (k, t[k]['us_median'], t[k]['gbps_median'], t[ck]['us_median'], t[ck]['spread'], t[k]['ratio_to_copy']))
    res['confusion'] = t
    del fns, keep

    # ---- 3. eval_metrics, device path against host path
    H = W = 64
    b, c, M, Z = 8, 3, 2, 40
    table, img_addrs, mask_addrs = {}, {'T1': [], 'T2': []}, []
    for s in range(3):
        for mod in img_addrs:
            p = 'sub%d_%s' % (s, mod)
            table[p] = rs.randint(-500, 3000, size=(H, W, Z)).astype(np.int16)
            img_addrs[mod].append(p)
        table['mask%d' % s] = rs.randint(0, c, size=(H, W, Z)).astype(np.uint8)
        mask_addrs.append('mask%d' % s)
    luv = [np.array([0, 1]), np.array([2]), np.array([], dtype=int)]
    dat = data_holders.regular({k: list(v) for k, v in img_addrs.items()}, list(mask_addrs), lambda p: table[p], None, luv, np.arange(c))
    dat.load_images(sess)
    np.random.seed(5)
    dat.create_train_valid_gens(b, [H, W], n_labeled_train=b // 2)
    ld, sk = netspec.net_c_2d_dense(c)
    m = NN_extended.CNN((H, W, M), ld, 'evalseg', list(sk), sess=sess, max_batch=b)
    m.set_weights(netspec.he_init(ld, (H, W, M), seed=5, skips=sk, bias_std=0.05))
    # the generator's batches, drawn once (its epoch state is not a function of the seed alone): both ways see the same ones
    drawn = [dat.train_gen_fn() for _ in range(a.iters)]

    def replay():
        state = {'k': 0}

        def gen():
            state['k'] += 1
            return drawn[(state['k'] - 1) % len(drawn)]
        return gen
    on_device = eval_utils._on_device
    times, values = {'device': [], 'host': []}, {}
    for rnd in range(1 + a.rounds):
        for way in ('host', 'device'):
            eval_utils._on_device = on_device if way == 'device' else (lambda model: False)
            m.valid_metrics = {'acc': [], 'F1': [], 'av_loss': []}
            gen = replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_utils.eval_metrics(m, sess, gen, iters=a.iters)
            torch.cuda.synchronize()
            if rnd:                       # round 0 warms both paths up
                times[way].append((time.perf_counter() - t0) * 1e3)
            values[way] = {k: v[0] for k, v in m.valid_metrics.items()}
    eval_utils._on_device = on_device
    res['eval_metrics'] = dict(ms_device=float(np.median(times['device'])), ms_host=float(np.median(times['host'])),
                               ms_device_rounds=times['device'], ms_host_rounds=times['host'], iters=a.iters,
                               equal=bool(values['device'] == values['host']), values=values['device'],
                               bytes_to_host_before=a.iters * (b * H * W * c * 4 + b * H * W * 4), bytes_to_host_after=8 * c * c)
    e = res['eval_metrics']
    e['ratio_host_over_device'] = e['ms_host'] / e['ms_device']
    print('eval_metrics, %d iterations of %d x %d x %d, c = %d: host path %.1f ms, device path %.1f ms (host / device %.2f); same values: %s; '
          'bytes copied to the host per call: %d before (posterior maps and labels), %d after'
          % (a.iters, b, H, W, c, e['ms_host'], e['ms_device'], e['ratio_host_over_device'], e['equal'], e['bytes_to_host_before'],
             e['bytes_to_host_after']))

    # ---- 4. lesions
    d_big = sess.to_device(big, torch.uint8)
    fn = lambda: lesion_utils.find_lesion_components(d_big, sess=sess)      # noqa: E731
    for _ in range(3):
        fn()
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    lesion_utils.find_lesion_components(big, sess=sess)
    t_array = (time.perf_counter() - t0) * 1e3
    res['lesions'] = dict(shape=list(big.shape), components=int(len(roots)), ms_device_tensor=float(np.median(ts)), ms_array_in_array_out=t_array,
                          ms_host_statement=t_host * 1e3)
    print('find_lesion_components at %r, %d components: device tensor in / out %.2f ms, array in / out %.1f ms, host statement %.0f ms'
          % (big.shape, len(roots), res['lesions']['ms_device_tensor'], t_array, t_host * 1e3))
    res.update(reps=a.reps, warmup=a.warmup, rounds=a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
