#!/usr/bin/env python3
"""What a training step and a weight load cost with the weights packed on the device (alq_model_set_weights_device) against
the host repack (ALQ_HOST_REPACK=1 at model creation: the path every step took before), all arms in one process.

    python tools/gpu_train_step.py [--reps 7] [--batch 32] [--only netb,netc,load] [--out FILE]

Arms, alternating, `reps` repetitions each after one warm-up, best and range reported:
  * NET-B (create_PW1, 32 x 32 x 32-channel patches: fc 6144 -> 4096 -> 4096 -> 2, 42 M parameters) train step of `batch` patches;
  * NET-C (32^3 patches) train step of `batch` patches;
  * load_weights of one NET-B member at the reference's patch (25, 25, 2) (fc 4704 -> 4096 -> 4096 -> 2, a 144 MB file), split
    into np.load (weights_io.read_weights) and the rest (set_weights).  At this shape fc1's 4704 inputs are no multiple of
    64: its backward Gemm is not on the streaming GEMM and the layer stays on the host packers; fc2 is packed on the device.
Prints one JSON line.  The pack kernels' own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool
(--only netb --reps 2); `pack_bytes` in the line is what each kernel moves per call."""
import argparse
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
from nnal_amd import device, netspec, weights_io  # noqa: E402


def model_under(env, sess, *args, **kwargs):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return device.DeviceModel(sess, *args, **kwargs)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def summary(ts):
    return dict(best_s=min(ts), max_s=max(ts), spread_s=max(ts) - min(ts), all_s=ts)


def alternate(reps, arms):
    """arms: name -> callable returning seconds; one warm-up each, then `reps` rounds in alternating order."""
    names = list(arms)
    for n in names:
        arms[n]()
    ts = {n: [] for n in names}
    for r in range(reps):
        for n in (names if r % 2 == 0 else names[::-1]):
            ts[n].append(arms[n]())
    return {n: summary(v) for n, v in ts.items()}


def train_arms(sess, ld, in_shape, sk, batch, reps, seed):
    pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    rs = np.random.RandomState(seed + 1)
    x = rs.randn(batch, *in_shape).astype(np.float32)
    lab = rs.randint(0, 2, size=batch)
    y = np.zeros((2, batch))
    y[lab, np.arange(batch)] = 1
    models = {}
    for name, env in (('device', {}), ('host_repack', {'ALQ_HOST_REPACK': '1'})):
        m = model_under(env, sess, ld, in_shape, sk, max_batch=batch)
        m.set_weights(pars)
        m.get_optimizer(1e-3, [], 'SGD')
        models[name] = m
    losses = {n: [] for n in models}

    def arm(name):
        def run():
            m = models[name]
            torch.cuda.synchronize()
            t = time.perf_counter()
            losses[name].append(m.train_on_batch(x, y))
            torch.cuda.synchronize()
            return time.perf_counter() - t
        return run
    res = alternate(reps, {n: arm(n) for n in models})
    res['same_losses'] = losses['device'] == losses['host_repack']
    res['same_weights'] = bool(np.array_equal(models['device'].flat_params().view(np.uint32), models['host_repack'].flat_params().view(np.uint32)))
    res['parameters'] = models['device'].num_params
    res['device_packed_layers'] = [models['device'].var_names[t] for t in range(models['device'].L) if models['device']._dev_pack[t]]
    d, h = res['device'], res['host_repack']
    res['host_over_device'] = h['best_s'] / d['best_s']
    res['gain_s'] = h['best_s'] - d['best_s']
    res['gain_exceeds_host_spread'] = bool(res['gain_s'] > h['spread_s'])
    res['device_not_slower_than_host_by_more_than_its_spread'] = bool(d['best_s'] - h['best_s'] <= h['spread_s'])
    # bytes one device set of a wide fc layer moves, per kernel (fp32 in, bf16 triples + fp16 pairs out, both orientations)
    pb = {}
    for t, (nme, ws, _) in enumerate(models['device'].param_shapes):
        if models['device']._dev_pack[t]:
            e = int(np.prod(ws))
            pb[nme] = dict(elements=e, stats=4 * e, permute=8 * e, pack_per_orientation=14 * e)
    res['pack_bytes'] = pb
    for m in models.values():
        m.close()
    return res


def load_arms(sess, reps, tmp):
    ld, in_shape = netspec.net_b(), (25, 25, 2)
    pars = netspec.he_init(ld, in_shape, seed=11, bias_std=0.05)
    path = os.path.join(tmp, 'member.npz')
    models = {n: model_under(env, sess, ld, in_shape, (), max_batch=64)
              for n, env in (('device', {}), ('host_repack', {'ALQ_HOST_REPACK': '1'}))}
    weights_io.write_weights(path, pars)
    del pars
    t_load = {n: [] for n in models}

    def arm(name):
        def run():
            m = models[name]
            torch.cuda.synchronize()
            t = time.perf_counter()
            p = weights_io.read_weights(path, m.var_names)
            p = {k: [np.asarray(W), np.asarray(b)] for k, (W, b) in p.items()}
            t1 = time.perf_counter()
            m.set_weights(p)
            torch.cuda.synchronize()
            t_load[name].append(t1 - t)
            return time.perf_counter() - t1
        return run
    res = alternate(reps, {n: arm(n) for n in models})
    res['file_bytes'] = os.path.getsize(path)
    res['np_load'] = {n: summary(v[1:]) for n, v in t_load.items()}
    res['rest_is'] = 'set_weights: packing and upload'
    res['device_packed_layers'] = [models['device'].var_names[t] for t in range(models['device'].L) if models['device']._dev_pack[t]]
    res['host_over_device'] = res['host_repack']['best_s'] / res['device']['best_s']
    for m in models.values():
        m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--only', default='netb,netc,load')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    only = a.only.split(',')
    sess = device.DeviceSession(0)
    out = dict(tool='gpu_train_step', reps=a.reps, batch=a.batch, optimizer='SGD')
    tmp = tempfile.mkdtemp(prefix='gpu_train_step_')
    try:
        if 'netb' in only:
            out['netb_train_step'] = train_arms(sess, netspec.net_b(), (32, 32, 32), (), a.batch, a.reps, 5)
        if 'netc' in only:
            ld, sk = netspec.net_c()
            out['netc_train_step'] = train_arms(sess, ld, (32, 32, 32, 1), sk, a.batch, a.reps, 7)
        if 'load' in only:
            out['netb_load_weights'] = load_arms(sess, a.reps, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    sess.close()


if __name__ == '__main__':
    main()
