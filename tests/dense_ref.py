"""fp64 / fp32 truth for fully-convolutional models (1x1 conv head): a short torch graph over oracle.tfops with autograd.
TEST INFRASTRUCTURE for tests/test_dense_host.py and tests/test_gpu_dense.py; oracle.model.OracleModel asserts an fc head.

DenseGraph carries the three attributes tests.test_gpu_losses._oracle / _TorchStep read of an oracle model (`params`, `_graph`,
`_as_input`), with `_graph(x)['output']` = the logits as columns [c, N * V] (voxel index n V + v, v in memory order), so the
objective restated there applies with voxels as samples."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tfops


class DenseGraph(object):
    def __init__(self, layer_dict, in_shape, pars, skips=(), dtype=torch.float64):
        self.layer_dict, self.in_shape, self.skips, self.dtype = layer_dict, tuple(in_shape), [list(s) for s in skips], dtype
        self.names = list(layer_dict.keys())
        self.params = OrderedDict()
        for name in self.names:
            if layer_dict[name][0] in ('conv', 'conv_transpose'):
                W, b = pars[name]
                self.params[name] = [torch.tensor(np.asarray(W), dtype=dtype, requires_grad=True),
                                     torch.tensor(np.asarray(b).reshape(-1), dtype=dtype, requires_grad=True)]
        assert layer_dict[self.names[-1]][0] == 'conv', 'a dense graph ends in a conv head'
        self.drop = None          # dict(layers, keep_prob, seed, first_sample) like OracleModel's
        self.fragile = 0          # fragile ReLU / pool decisions of the last maps() call made with eps

    def _as_input(self, x):
        return torch.as_tensor(np.asarray(x)).to(self.dtype).reshape((-1,) + self.in_shape)

    @staticmethod
    def _rms(t):
        return torch.sqrt((t.detach() ** 2).mean(dim=list(range(1, t.dim())), keepdim=True))

    def _pool(self, t, w, eps):
        out = tfops.max_pool_same(t, w, w)
        if eps:      # a positive window maximum whose runner-up is within eps * rms of it (the rule of alq_ref64_scores)
            nd = t.dim() - 2
            flat = []
            for d in reversed(range(nd)):
                _, lo, hi = tfops.same_pads(t.shape[1 + d], list(w)[d], list(w)[d])
                flat += [lo, hi]
            xp = F.pad(tfops._to_cf(t.detach()), flat, value=float('-inf'))
            fn = F.max_pool2d if nd == 2 else F.max_pool3d
            best, idx = fn(xp, list(w), list(w), return_indices=True)
            shp = xp.shape
            x2 = xp.reshape(shp[0], shp[1], -1).clone()
            x2.scatter_(2, idx.reshape(shp[0], shp[1], -1), float('-inf'))
            second = fn(x2.reshape(shp), list(w), list(w))
            rms = self._rms(t).reshape(-1, *([1] * (nd + 1)))
            self.fragile += int(((best > 0) & ((best - second) <= eps * rms)).sum())
        return out

    def maps(self, x, eps=0.):
        """Logits [N, *spatial, c] of x [N, *in_shape] (a tensor of the graph's dtype)."""
        self.fragile = 0
        out, sources = x, {}
        src_idx = [s[0] for s in self.skips]
        for i, name in enumerate(self.names):
            spec = self.layer_dict[name]
            for (src, dsts, kind) in self.skips:
                if i in dsts:
                    assert kind == 'con'
                    out = torch.cat((sources[src], out), dim=out.dim() - 1)      # the earlier output first
            ltype = spec[0]
            if ltype == 'conv':
                out = tfops.conv_same(out, *self.params[name])
            elif ltype == 'conv_transpose':
                out = tfops.conv_transpose_same(out, self.params[name][0], self.params[name][1], spec[1][2])
            elif ltype == 'pool':
                out = self._pool(out, spec[1], eps)
            else:
                raise ValueError(ltype)
            if len(spec) > 2 and 'A' in spec[2]:
                if eps:
                    self.fragile += int((out.detach().abs() <= eps * self._rms(out)).sum())
                out = torch.relu(out)
            d = self.drop
            if d is not None and d['keep_prob'] < 1. and i in d['layers']:
                N, per = out.shape[0], int(np.prod(out.shape[1:]))
                keep = tfops.dropout_keep(d['seed'], i, d.get('first_sample', 0) + np.arange(N), per, d['keep_prob'])
                k = torch.as_tensor(np.ascontiguousarray(keep.reshape(tuple(out.shape)))).to(out.dtype)
                out = out * k * torch.tensor(np.float32(1.0) / np.float32(d['keep_prob']), dtype=torch.float32).to(out.dtype)
            if i in src_idx:
                sources[i] = out
        return out

    def _graph(self, x, drop=None):
        z = self.maps(x)
        c = z.shape[-1]
        return {'output': z.reshape(-1, c).t()}

    def posteriors(self, x):
        with torch.no_grad():
            return torch.softmax(self.maps(self._as_input(x)), dim=-1).numpy()


def select_inputs(g64, in_shape, n, seed, eps, max_draws=400):
    """The first n samples of the stream RandomState(seed).randn(*in_shape) whose fp64 evaluation has no fragile ReLU input or
    pool near-tie at eps; (x [n, *in_shape] float32, samples drawn)."""
    rs = np.random.RandomState(seed)
    keep, drawn = [], 0
    while len(keep) < n:
        assert drawn < max_draws, 'no %d clean samples among %d' % (n, drawn)
        x = rs.randn(1, *in_shape).astype(np.float32)
        drawn += 1
        with torch.no_grad():
            g64.maps(g64._as_input(x), eps=eps)
        if g64.fragile == 0:
            keep.append(x)
    return np.concatenate(keep, axis=0), drawn


def flat_grads(g, diff):
    plist = [p for pair in g.params.values() for p in pair]
    grads = torch.autograd.grad(diff, plist, allow_unused=True)
    return [np.zeros(tuple(p.shape)) if gr is None else gr.numpy() for p, gr in zip(plist, grads)]
