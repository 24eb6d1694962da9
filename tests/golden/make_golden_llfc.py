#!/usr/bin/env python3
"""Goldens of the last-layer closed forms and the stochastic influence recursion (build container only):

    python tests/golden/make_golden_llfc.py      ->  tests/golden/llfc.npz

`tests/golden/tfshim.py` is registered as `tensorflow`; then, unmodified from the reference:
  * NN.CNN(x, layer_dict, name, feature_layer, dropout) + get_optimizer                        (NN.py:56-619)
  * NN.LLFC_grads (given labels and labels=None), NN.LLFC_hess                                  (NN.py:874-955)
  * PW_NNAL.stoch_approx_IF under np.random.seed                                                (PW_NNAL.py:851-881)
run on two small nets: `pool` (feature layer = a pool layer: the reference's reversed flatten order, c = 2) and `fc`
(feature layer behind an fc: already flat, c = 3).  Inputs are scaled so that |u~|^2 <= scale: -H / scale then has no
eigenvalue above 1/2 and the recursion does not grow faster than t * max|G| (asserted).  The implicit float64 restatement
(tests/llfc_ref.py) must reproduce every output to 1e-12 from the stored features, posteriors and draws.  Arrays only.

The session handed to the reference returns the graph's float32 values as float64 arrays (Float64Session): the reference's
NumPy products then round in float64 whatever the fetch dtype (on float32 fetches `rep_pies * rep_U` and `np.kron` would
round to float32, 4e-7 of the largest entry), which is what lets the goldens pin the algebra to 1e-12."""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden_refgraph  # noqa: E402
import tfshim  # noqa: E402

NETS = [
    ('pool', OrderedDict([('conv1', [2, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [2, 'fc'])]), 1, 61),
    ('fc', OrderedDict([('conv1', [3, 'conv', [3, 3]]), ('max1', [[2, 2], 'pool']), ('fc1', [10, 'fc']), ('fc2', [3, 'fc'])]), 2, 62),
]
IN_SHAPE = (12, 12, 1)
N_POOL, N_TR, MAX_ITER, SCALE = 7, 5, 25, 50


class Float64Session(object):
    def __init__(self, sess):
        self.sess = sess

    def run(self, fetches, feed_dict=None):
        r = self.sess.run(fetches, feed_dict=feed_dict)
        return np.asarray(r, dtype=np.float64) if isinstance(r, np.ndarray) and r.dtype.kind == 'f' else r


def main():
    from oracle import netspec
    from tests import llfc_ref
    mods = make_golden_refgraph.import_reference_with_shim()
    PW_NNAL, NN = mods[3], mods[4]
    tf = tfshim
    out = {'max_iter': np.int64(MAX_ITER), 'scale': np.float64(SCALE), 'in_shape': np.array(IN_SHAPE)}
    for tag, ld, feat, seed in NETS:
        tf.reset_default_graph()
        pars = netspec.he_init(ld, IN_SHAPE, seed=seed, bias_std=0.05)
        x = tf.placeholder(tf.float32, [None] + list(IN_SHAPE), name='input')
        model = NN.CNN(x, type(ld)((k, list(v)) for k, v in ld.items()), tag, feat, [[len(ld) - 1], 1.], [])
        model.get_optimizer(1e-3, [], 'SGD')
        for n in pars:
            W, b = model.var_dict[n][-2:]
            W.load(pars[n][0])
            b.load(pars[n][1])
        sess = Float64Session(tf.Session())
        rs = np.random.RandomState(seed + 100)
        pool = (0.25 * rs.randn(N_POOL, *IN_SHAPE)).astype(np.float32)
        tr = (0.25 * rs.randn(N_TR, *IN_SHAPE)).astype(np.float32)
        fd_pool = {model.x: pool, model.keep_prob: 1.}
        Up = np.asarray(sess.run(model.feature_layer, feed_dict=fd_pool))
        Pp = np.asarray(sess.run(model.posteriors, feed_dict=fd_pool))
        # one training sample per run, as stoch_approx_IF feeds them (a batched forward may round differently)
        Ut = np.concatenate([sess.run(model.feature_layer, feed_dict={model.x: tr[[i]], model.keep_prob: 1.}) for i in range(N_TR)], 1)
        Pt = np.concatenate([sess.run(model.posteriors, feed_dict={model.x: tr[[i]], model.keep_prob: 1.}) for i in range(N_TR)], 1)
        d, c = Up.shape[0], Pp.shape[0]
        assert d <= 200 and ((Ut.astype(np.float64) ** 2).sum(0) + 1. <= SCALE).all(), (d, (Ut ** 2).sum(0))
        given = (np.arange(N_POOL) * 2 + 1) % c
        G_given = NN.LLFC_grads(model, sess, fd_pool, given)
        G_pred, pred = NN.LLFC_grads(model, sess, fd_pool)
        H = NN.LLFC_hess(model, sess, {model.x: tr[[3]], model.keep_prob: 1.})
        np.random.seed(seed)
        V, weak = PW_NNAL.stoch_approx_IF(model, sess, tr, pool, MAX_ITER, SCALE)
        np.random.seed(seed)
        draws = np.array([np.random.randint(N_TR) for _ in range(MAX_ITER)])
        assert np.abs(V).max() < MAX_ITER * np.abs(G_pred).max()

        def rel(a, b):
            return np.abs(a - b).max() / np.abs(b).max()
        errs = (rel(llfc_ref.llfc_grads(Up, Pp, given), G_given), rel(llfc_ref.llfc_grads(Up, Pp, pred), G_pred),
                rel(llfc_ref.llfc_hess(Ut[:, 3], Pt[:, 3]), H), rel(llfc_ref.stoch_if(Up, Pp, weak, Ut, Pt, draws, SCALE), V))
        assert max(errs) < 1e-12, errs
        np.testing.assert_array_equal(weak, pred)
        for k, v in dict(pool_x=pool, tr_x=tr, pool_feat=Up, pool_post=Pp, tr_feat=Ut, tr_post=Pt, labels=given, G_given=G_given,
                         G_pred=G_pred, pred=pred, H3=H, V=V, weak=weak, draws=draws, seed=np.int64(seed),
                         feature_layer=np.int64(feat)).items():
            out['%s_%s' % (tag, k)] = v
        for n in pars:
            out['%s_W_%s' % (tag, n)] = pars[n][0]
            out['%s_b_%s' % (tag, n)] = pars[n][1]
        print('%-4s d = %d, c = %d: max|u~|^2 = %.2f, max|G| = %.3f, max|V| = %.3f, restatement within %.1e' %
              (tag, d, c, (Ut.astype(np.float64) ** 2).sum(0).max() + 1., np.abs(G_pred).max(), np.abs(V).max(), max(errs)))
    np.savez_compressed(os.path.join(HERE, 'llfc.npz'), **out)
    print('wrote llfc.npz (%d arrays, %d bytes)' % (len(out), os.path.getsize(os.path.join(HERE, 'llfc.npz'))))


if __name__ == '__main__':
    main()
