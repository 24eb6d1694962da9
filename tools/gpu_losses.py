#!/usr/bin/env python3
"""The training objectives of NN_extended.CNN on the device (csrc/loss.hip) against their NumPy restatement (nnal_amd.losses),
one small net (NET-A at 20 x 20, 12 samples): per loss, the largest difference of a cotangent row in fp32 ulp of the row's
largest entry and the relative difference of the three statistics, on the device's own posteriors.

    python tools/gpu_losses.py [--out losses.json]

Prints one line per loss and one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import nnal_amd  # noqa: F401
    from nnal_amd import device, losses, netspec
    from nnal_amd._lib import LossT, check
    sess = device.DeviceSession(0)
    ld, shape, n = netspec.net_a(), (20, 20, 1), 12
    m = device.DeviceModel(sess, ld, shape, (), max_batch=16)
    m.set_weights(netspec.he_init(ld, shape, seed=71, bias_std=0.05))
    rs = np.random.RandomState(21)
    x = sess.to_device(rs.randn(n, 400).astype(np.float32), torch.float32)
    lab = rs.randint(0, 2, size=n).astype(np.int32)
    lab[3] = -1
    soft = rs.rand(2, n).astype(np.float32)
    soft /= soft.sum(0)
    sw = (0.25 + rs.rand(n)).astype(np.float32)
    sw[n - 2] = 0
    old = (rs.randn(2, n) * 2).astype(np.float32)
    cw = np.array([0.3, 1.7], np.float32)
    q = float(np.float32(0.7))
    dev = {k: sess.to_device(v, torch.int32 if k == 'lab' else torch.float32)
           for k, v in dict(lab=lab, soft=soft, sw=sw, old=old, cw=cw).items()}
    cases = [('weighted CE', losses.CE, dict(class_w=cw, sample_w=sw)),
             ('focal CE, gamma 2', losses.CE, dict(class_w=cw, sample_w=sw, focal_gamma=2.)),
             ('focal CE, gamma 0.5', losses.CE, dict(focal_gamma=0.5)),
             ('CE_softclasses', losses.CE_SOFT, dict(targets=soft)),
             ('GCE, q 0.7', losses.GCE, dict(targets=soft, q=q)),
             ('CE + LwF, T 2', losses.CE, dict(old_logits=old, T=2.))]
    res = []
    arr = (C.c_int32 * 1)()
    s, s2 = float(np.float32(1. / 9)), float(np.float32(0.5 / n))
    sess.bind_stream()
    for name, kind, kw in cases:
        L = LossT(kind, kw.get('focal_gamma', -1.), q, kw.get('T', 1.), dev['cw'].data_ptr() if 'class_w' in kw else None,
                  dev['sw'].data_ptr() if 'sample_w' in kw else None, dev['soft'].data_ptr() if 'targets' in kw else None,
                  dev['old'].data_ptr() if 'old_logits' in kw else None)
        g = sess.empty((m.num_params,), torch.float32)
        post = sess.empty((2, n), torch.float32)
        st = sess.empty((3,), torch.float64)
        check(m.lib.alq_param_grads_loss(m._m, C.c_void_p(x.data_ptr()), n, C.c_void_p(dev['lab'].data_ptr()), C.byref(L), s, s2, 1., 0, 0,
                                         arr, 0, C.c_void_p(g.data_ptr()), C.c_void_p(post.data_ptr()), C.c_void_p(st.data_ptr())))
        rows = sess.empty((n * 2,), torch.float32)
        check(m.lib.alq_model_debug_copy(m._m, len(m.layers) - 1, 1, n, C.c_void_p(rows.data_ptr()), None))
        rows = rows.cpu().numpy().reshape(n, 2).astype(np.float64)
        ref = losses.evaluate(post.cpu().numpy(), lab, kind, loss_scale=s, lwf_scale=s2, **kw)
        top = np.abs(ref['rows']).max(1)
        ulp = np.where(top > 0, np.spacing(top.astype(np.float32)).astype(np.float64), 1.)
        row_ulp = float((np.abs(rows - ref['rows']).max(1) / ulp).max())
        stats = st.cpu().numpy()
        rel = [abs(a_ - b_) / abs(b_) if b_ else abs(a_) for a_, b_ in zip(stats, ref['stats'])]
        print('%-22s rows: %.2f ulp   stats: device %s   restatement %s   rel. diff. %.1e' %
              (name, row_ulp, np.array2string(stats, precision=10), np.array2string(np.array(ref['stats']), precision=10), max(rel)))
        res.append(dict(loss=name, row_ulp=row_ulp, stats_rel=max(rel), stats=[float(v) for v in stats]))
    line = json.dumps(dict(net='NET-A 20x20', samples=n, cases=res))
    print(line)
    if a.out:
        open(a.out, 'w').write(line + '\n')
    m.close()


if __name__ == '__main__':
    main()
