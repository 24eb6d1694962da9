"""The device model behind the reference's `model`: creation, weights, the forward calls and the Fisher pass with its
pipelines; the gradient entry points and training are the mixins of device_grads and device_train."""
import contextlib
import ctypes as C
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import ALQ_CONV, ALQ_CONVT, ALQ_POOL, LayerT, check, check_tensor, ptr
from .device_grads import ModelGrads
from .device_host import Handle, LazyVarDict, _fc_only, out_map_shape, tf_param_shapes, translate_layers
from .device_session import DeviceSession, _track, side_stream
from .device_train import ModelTrain


class DeviceModel(ModelGrads, ModelTrain):
    """The reference model protocol (`x, keep_prob, posteriors, prediction, feature_layer,
    grad_posts, var_dict, dropout_rate`) over a libalq model."""

    def __init__(self, sess, layer_dict, in_shape, skips=(), feature_layer=None, dropout=None,
                 max_batch=256, name='model', aleatoric=False, au_log_rel_coeff=0.1):
        self.sess = sess
        self.lib = sess.lib
        self.name = name
        self.layer_dict = layer_dict
        self.in_shape = tuple(int(v) for v in in_shape)
        self.skips = [list(s) for s in skips]
        self.max_batch = int(max_batch)
        self.layers = translate_layers(layer_dict, self.in_shape, skips)
        self.param_shapes = tf_param_shapes(self.layers, self.in_shape)
        self.var_names = [p[0] for p in self.param_shapes]
        nd = len(self.in_shape) - 1
        dims = [1] * (3 - nd) + list(self.in_shape[:-1]) + [self.in_shape[-1]]
        arr = (LayerT * len(self.layers))()
        for i, d in enumerate(self.layers):
            arr[i].type = d['type']
            arr[i].cout = d['cout']
            arr[i].k[:] = d['k']
            arr[i].s[:] = d['s']
            arr[i].relu = d['relu']
            arr[i].skip_src = d['skip_src']
        self._m = C.c_void_p()
        cd = (C.c_int32 * 4)(*dims)
        self._create_args = (arr, len(self.layers), cd)
        check(self.lib.alq_model_create(sess.ctx, arr, len(self.layers), cd, self.max_batch, C.byref(self._m)))
        _track(self)
        self.max_batch = int(self.lib.alq_model_max_batch(self._m))      # may be below the request: 32-bit tensor offsets (alq.h)
        # extra scoring pipelines (fisher_device): created at the first call that has that many device passes to run.  Default
        # since round 6: two (ALQ_LANES=1: one pipeline; up to 4: three measured no faster than two, four slower): outputs are
        # bit-identical; each costs a set of workspaces
        self.lanes = max(1, min(4, int(os.environ.get('ALQ_LANES', '2'))))
        self._xlanes = []                 # the extra pipelines (lanes - 1 of them once a call spans that many passes)
        self._create_env = {k: v for k, v in os.environ.items() if k.startswith('ALQ_')}     # engine switches are read at creation
        self.L = self.lib.alq_model_num_param_layers(self._m)
        self.nclass = self.layers[-1]['cout']
        # AU_4U (NN_extended.py:265-288): the head's last channel, through a ReLU, is a per-voxel log-variance; class_num = cout - 1
        self.AU_4U = bool(aleatoric)
        self.AU_log_rel_coeff = float(au_log_rel_coeff)
        if self.AU_4U:
            check(self.lib.alq_model_set_aleatoric(self._m, 1))
            self.nclass -= 1
        self.class_num = self.nclass
        # a fully-convolutional model (1x1 conv head, csrc/dense.hip): every voxel of the head's output map is a sample
        self.dense = self.layers[-1]['type'] == ALQ_CONV
        self.out_voxels = int(self.lib.alq_model_out_voxels(self._m))
        self.out_map_shape = out_map_shape(self.layers, self.in_shape) if self.dense else ()
        if self.dense and int(np.prod(self.out_map_shape)) != self.out_voxels:
            raise AssertionError('output map %r against %d voxels in the library' % (self.out_map_shape, self.out_voxels))
        self.elems_per_patch = int(np.prod(self.in_shape))
        # reference-style attributes
        self.x = Handle('x')
        self.keep_prob = Handle('keep_prob')
        self.dropout_layers, self.dropout_rate = (dropout[0], dropout[1]) if dropout else ([], 1.)
        self.posteriors = Handle('posteriors')
        self.prediction = Handle('prediction')
        self.feature_idx = feature_layer
        fdim = 0
        if feature_layer is not None:
            e = C.c_int64()
            check(self.lib.alq_model_layer_out_elems(self._m, int(feature_layer), C.byref(e)))
            fdim = e.value
        self.feature_dim = fdim
        self.feature_layer = Handle('feature_layer', (fdim,))
        for h in (self.posteriors, self.prediction, self.feature_layer):
            h.model = self
        if self.AU_4U:
            self.AU_vals, self.output = Handle('AU_vals'), Handle('output')          # [n, *spatial] and [n, *spatial, c + 1]
            self.AU_vals.model = self.output.model = self
        # 2L opaque entries per class, so that len(model.grad_posts['1'])/2 == L (PW_NNAL.py:751)
        self.var_dict = LazyVarDict((n, None) for n in self.var_names)
        # Weights that are already in device memory are packed there (alq_model_set_weights_device): per parameterised layer,
        # whether the library has device packers for it (wide fc layers) and the device tensors (W, b) its current weights were
        # packed from (None: host arrays only).  ALQ_HOST_REPACK=1 at creation (A/B, tests): everything through the host packers.
        self._host_repack = os.environ.get('ALQ_HOST_REPACK', '0') not in ('', '0')
        self._dev_pack = [self.lib.alq_model_layer_packs_on_device(self._m, t) == 1 for t in range(self.L)]
        self._dev_w = [None] * self.L
        self.grad_layers = []
        self._build_grad_handles()
        self.y_ = Handle('y_')
        self.loss = Handle('loss')        # mean softmax cross-entropy of a labelled batch (NN.py:583-588)
        self.loss.model = self
        self.train_step = None            # get_optimizer() creates it (NN.py:557-615)
        self._opt = None
        # NN_extended.set_hypers: None = the batch-mean cross-entropy of NN.py:583-588; else the objective of NN_extended.get_loss
        self.hypers = None
        self._obj = None
        self.input_weights = Handle('input_weights')      # per-sample loss weights [n], fed through feed_dict
        self.input_vox_weights = Handle('input_vox_weights', self.out_map_shape) if self.dense else None      # [n, *spatial] (get_FCN_loss)
        self.labels = Handle('labels')
        self.pt = Handle('pt')
        self.labels.model = self.pt.model = self
        self._weights_version = 0         # bumped by every set_weights: the optimiser's device copy follows it
        self.PFT_bflag = False            # set_PFT_mask: the summed gradient is multiplied by a binary mask (NN_extended.py:1441-1449)
        self._pft_mask = None             # float32 device [P]
        self._pft_layers = None           # parameterised layers with a non-zero mask entry
        self._mt = None                   # set_mean_teacher: the settings and state of mean-teacher training
        self.num_params = int(self.lib.alq_model_num_params(self._m))
        self._feature_perm = self._feature_permutation()

    # -- gradients of the log-posteriors (get_gradients, NN.py:621-645) -------------------
    def _build_grad_handles(self):
        """2L' opaque entries per class - L' = the layers of `grad_layers` (all when empty) - so that
        len(model.grad_posts['1'])/2 is the A-matrix size PW_NNAL.gen_A_matrices reads (PW_NNAL.py:751)."""
        names = list(self.grad_layers) if len(self.grad_layers) else list(self.var_names)
        for nme in names:
            if nme not in self.var_names:
                raise KeyError('grad layer %r is not a parameterised layer of the model' % (nme,))
        self.grad_layer_idx = [self.var_names.index(nme) for nme in names]
        self.grad_posts = {}
        for j in range(self.nclass):
            hs = []
            for t in self.grad_layer_idx:
                for part in ('W', 'b'):
                    h = Handle('grad_%d_%s_%s' % (j, self.var_names[t], part))
                    h.model, h.cls = self, j
                    hs.append(h)
            self.grad_posts[str(j)] = hs

    @_fc_only
    def get_gradients(self, grad_layers=[]):
        """NN.py:621-645 / NN_extended.py:1011-1035: the gradient lists cover `grad_layers` (all layers when empty)."""
        self.grad_layers = list(grad_layers)
        self._build_grad_handles()

    def unflatten(self, vec, layers=None):
        """Flat parameter-order vector [W_0, b_0, W_1, ...] -> list of arrays in TF variable shapes (of `layers`)."""
        out, off = [], 0
        keep = set(range(self.L)) if layers is None else set(layers)
        for t, (name, wshape, bshape) in enumerate(self.param_shapes):
            nw, nb = int(np.prod(wshape)), int(np.prod(bshape))
            if t in keep:
                out += [vec[off:off + nw].reshape(wshape), vec[off + nw:off + nw + nb].reshape(bshape)]
            off += nw + nb
        return out

    def flat_params(self):
        return np.concatenate([np.concatenate([np.asarray(W, np.float32).ravel(), np.asarray(b, np.float32).ravel()])
                               for W, b in self.var_dict.values()])

    def set_flat_params(self, vec):
        arrs = self.unflatten(np.asarray(vec, dtype=np.float32))
        self.set_weights({n: [arrs[2 * t], arrs[2 * t + 1]] for t, n in enumerate(self.var_names)})

    def _drop_args(self, keep_prob, seed):
        kp = float(keep_prob)
        lay = [int(v) for v in self.dropout_layers] if kp < 1. else []
        arr = (C.c_int32 * max(len(lay), 1))(*lay)
        if seed is None:
            # the reference's tf.nn.dropout draws a fresh mask per sess.run from TF's stream; here: a fresh seed per
            # call from the global NumPy stream (reproducible under np.random.seed like the rest of the query code)
            seed = int(np.random.randint(0, 2 ** 31 - 1)) if kp < 1. else 0
        return kp, arr, len(lay), int(seed)

    def _cuts(self, n):
        """(first, end) of every device pass over n patches: at most max_batch patches each, in order, none empty."""
        for a in range(0, n, self.max_batch):
            yield a, min(n, a + self.max_batch)

    def _patch_ptr(self, t, a):
        """Where patch `a` of the float32 device batch `t` starts."""
        return ptr(t, a * self.elems_per_patch * 4)

    # -- weights ---------------------------------------------------------------------------
    def set_weights(self, pars):
        """`pars`: name -> [W, b] in TF layouts (HWIO / DHWIO, transpose [k..,out,in], fc [out,in],
        fc bias [out,1]); the weight interchange of NN.py:390-394 / :508-517 with numpy arrays in
        place of the HDF5 datasets (h5py is not in the image)."""
        staged = []
        for t, (name, wshape, bshape) in enumerate(self.param_shapes):
            W, b = pars[name]
            W = np.ascontiguousarray(np.asarray(W, dtype=np.float32))
            b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
            if tuple(W.shape) != tuple(wshape) or b.size != int(np.prod(bshape)):
                raise ValueError('layer %s: expected W%s b%s, got W%s b%s' % (name, wshape, bshape, W.shape, b.shape))
            staged.append((W, b))
        torch = self.sess.torch
        self.var_dict.mark_fresh()
        self.sess.bind_stream()
        for t, name in enumerate(self.var_names):
            W, b = staged[t]
            if self._dev_pack[t] and not self._host_repack:
                # a wide fc layer: the raw arrays are uploaded once and packed on the device; the extra pipelines' models are fed
                # from the same tensors (_extra_lanes)
                Wd, bd = self.sess.to_device(W, torch.float32), self.sess.to_device(b, torch.float32)
                check(self.lib.alq_model_set_weights_device(self._m, t, ptr(Wd), ptr(bd)))
                self._dev_w[t] = (Wd, bd)
            else:
                check(self.lib.alq_model_set_weights(self._m, t, W.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
                self._dev_w[t] = None
            self.var_dict[name] = [W, b]
        self._weights_version += 1

    def _device_slices(self, src):
        """[(W, b)] device fp32 tensors per parameterised layer from a flat parameter-order vector [P], a dict
        name -> (W, b) or a list of (W, b)."""
        torch = self.sess.torch
        if isinstance(src, torch.Tensor):
            if src.dtype != torch.float32 or not src.is_contiguous() or int(src.numel()) != self.num_params or not src.is_cuda:
                raise ValueError('expected a contiguous device fp32 vector of %d parameters' % self.num_params)
            flat = src.reshape(-1)
            pairs = self.unflatten(flat)
            return [(pairs[2 * t], pairs[2 * t + 1]) for t in range(self.L)]
        if isinstance(src, dict):
            src = [src[nme] for nme in self.var_names]
        if len(src) != self.L:
            raise ValueError('expected %d (W, b) pairs, got %d' % (self.L, len(src)))
        out = []
        for (name, wshape, bshape), (W, b) in zip(self.param_shapes, src):
            for a, shp in ((W, wshape), (b, bshape)):
                if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and
                        int(a.numel()) == int(np.prod(shp))):
                    raise ValueError('layer %s: expected contiguous device fp32 tensors W%s b%s' % (name, wshape, bshape))
            out.append((W, b))
        return out

    def set_weights_device(self, theta_or_slices, only=None):
        """`set_weights` from DEVICE memory (alq_model_set_weights_device): a flat parameter-order fp32 vector [P] (what the
        optimiser step updates), a dict name -> (W, b) or a list of (W, b) device tensors in TF layouts.  The tensors must be
        ready on the current stream.  Wide fc layers are packed by device kernels, any other layer's slice takes the host
        packers; `var_dict` turns stale and is fetched on its next read.  `only`: the layer indices whose values changed
        (the rest of the model keeps its packed weights); the source still holds every layer.  The model keeps a reference
        to the tensors (they feed the extra scoring pipelines): the caller may update them in place only together with
        another call."""
        torch = self.sess.torch
        sl = self._device_slices(theta_or_slices)
        if self._host_repack:
            pars = OrderedDict((nme, [sl[t][0].cpu().numpy().reshape(self.param_shapes[t][1]),
                                      sl[t][1].cpu().numpy().reshape(self.param_shapes[t][2])])
                               for t, nme in enumerate(self.var_names))
            return self.set_weights(pars)
        if only is not None and any(v is None for v in OrderedDict.values(self.var_dict)) and not self.var_dict.stale:
            only = None          # nothing set yet: every layer needs its weights
        self.sess.bind_stream()
        for t in (range(self.L) if only is None else only):
            W, b = sl[t]
            check(self.lib.alq_model_set_weights_device(self._m, t, ptr(W), ptr(b)))
        self._dev_w = list(sl)
        flat = theta_or_slices if isinstance(theta_or_slices, torch.Tensor) else None

        def refresh():
            if flat is not None:          # one copy of the whole vector, cut like set_flat_params cuts it
                arrs = self.unflatten(flat.reshape(-1).cpu().numpy())
            else:
                arrs = [a.cpu().numpy().reshape(shp) for (W, b), (_, ws, bs) in zip(sl, self.param_shapes)
                        for a, shp in ((W, ws), (b, bs))]
            for t, nme in enumerate(self.var_names):
                self.var_dict.put(nme, [arrs[2 * t], arrs[2 * t + 1]])
        self.var_dict.mark_stale(refresh)
        self._weights_version += 1

    def load_weights(self, path, session=None):
        """CNN.load_weights (NN.py:396-419; NN_extended.py:708-760): an HDF5 file of the reference - groups per layer, datasets
        `Weight` / `Bias` in TF layouts - when h5py is importable, or the .npz twin (keys '<layer>/Weight', '<layer>/Bias')."""
        from . import weights_io
        self.set_weights(weights_io.read_weights(path, self.var_names))

    def save_weights(self, path):
        """CNN.save_weights (NN.py:379-394): `.h5` -> the reference's HDF5 layout (needs h5py), anything else -> the .npz twin."""
        from . import weights_io
        weights_io.write_weights(path, self.var_dict)

    def add_assign_ops(self):
        """No graph to extend (NN.py:421-458): kept so loop code calls it unchanged."""

    def perform_assign_ops(self, file_path, sess=None):
        """NN.py:462-519: 'init' draws He-normal weights with the global np.random in variable
        creation order (std = sqrt(2/n), zero biases); otherwise loads a weight file."""
        if file_path != 'init':
            return self.load_weights(file_path)
        pars = OrderedDict()
        for name, wshape, bshape in self.param_shapes:
            n = int(np.prod(wshape[:-1])) if len(wshape) > 2 else wshape[1]
            pars[name] = [np.sqrt(2. / n) * np.random.randn(*wshape), np.zeros(bshape)]
        self.set_weights(pars)

    # -- evaluation ------------------------------------------------------------------------
    def _feature_permutation(self):
        """feature_layer of a conv/pool layer is flattened in the reference's order (full axis
        reversal, NN.py:296-301,337-340); the device returns memory order.  Identity after an fc."""
        if self.feature_idx is None:
            return None
        # re-derive the layer's output geometry
        nd = len(self.in_shape) - 1
        spatial = list(self.in_shape[:-1])
        ch = self.in_shape[-1]
        for i, d in enumerate(self.layers):
            if d['type'] == ALQ_CONV:
                ch = d['cout']
            elif d['type'] == ALQ_CONVT:
                spatial = [a * b for a, b in zip(spatial, d['s'][3 - nd:])]
                ch = d['cout']
            elif d['type'] == ALQ_POOL:
                spatial = [-(-a // b) for a, b in zip(spatial, d['s'][3 - nd:])]
            else:
                return None                      # at or after an fc: already a flat vector
            if i == self.feature_idx:
                mem = np.arange(int(np.prod(spatial)) * ch).reshape(spatial + [ch])
                return mem.transpose(*reversed(range(nd + 1))).reshape(-1)
        return None

    def _as_device_batch(self, x):
        torch = self.sess.torch
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.sess.device, dtype=torch.float32).contiguous()
        else:
            t = self.sess.to_device(np.asarray(x), torch.float32)    # placeholder is tf.float32
        n = t.numel() // self.elems_per_patch
        if n * self.elems_per_patch != t.numel():
            raise ValueError('batch of %d elements is not a multiple of the patch size %d' % (t.numel(), self.elems_per_patch))
        return t, n

    def forward_dropout_device(self, t, n, keep_prob, seed=None, first_sample=0, want_pred=False):
        """Posteriors at keep_prob < 1 (MC strategies): alq_forward_dropout over device passes; masks keyed by sample id."""
        torch = self.sess.torch
        self.sess.bind_stream()
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        V = self.out_voxels          # samples per patch: 1, or the voxels of a dense model's output map
        post = self.sess.empty((self.nclass, n * V), torch.float32)
        pred = self.sess.empty((n * V,), torch.int64) if want_pred else None
        for a, b in self._cuts(n):
            pb = self.sess.empty((self.nclass, (b - a) * V), torch.float32)
            check(self.lib.alq_forward_dropout(self._m, self._patch_ptr(t, a), b - a, kp, seed, int(first_sample) + a, arr, nl, ptr(pb),
                                               ptr(pred, a * V * 8)))
            post[:, a * V:b * V] = pb
        return post, pred

    def forward_device(self, t, n, want_pred=False, want_feat=False, rows=None):
        """t: device fp32 tensor of n patches - or, with `rows` (int64 device tensor [n]), a resident pool whose
        rows `rows` are the patches (alq_forward_rows: no gathered copy on the caller's side).
        Returns device tensors (post [c,n], pred, feat)."""
        torch = self.sess.torch
        self.sess.bind_stream()
        V = self.out_voxels          # samples per patch: 1, or the voxels of a dense model's output map
        if rows is not None and self.dense:
            raise NotImplementedError('forward_device(rows=...): not defined for a fully-convolutional model (1x1 conv head)')
        post = self.sess.empty((self.nclass, n * V), torch.float32)
        pred = self.sess.empty((n * V,), torch.int64) if want_pred else None
        feat = self.sess.empty((n, self.feature_dim), torch.float32) if want_feat else None
        check_tensor(rows, torch.int64, n, optional=True)
        # one pipeline: forward-only passes leave no gaps a second one could fill (configs[4]'s filter: 0.3625 s per 200k patches
        # with two pipelines against 0.3601 s with one, same box)
        for a, b in self._cuts(n):
            pb = self.sess.empty((self.nclass, (b - a) * V), torch.float32)
            outs = (ptr(pb), ptr(pred, a * V * 8), ptr(feat, a * self.feature_dim * 4), self.feature_idx if want_feat else -1)
            if rows is None:
                check(self.lib.alq_forward(self._m, self._patch_ptr(t, a), b - a, *outs))
            else:
                check(self.lib.alq_forward_rows(self._m, ptr(t), ptr(rows, a * 8), b - a, *outs))
            post[:, a * V:b * V] = pb
        return post, pred, feat

    def forward_maps_device(self, t, n, keep_prob=1., want_pred=False, seed=None, first_sample=0):
        """A dense model's outputs as maps, on the device: (posteriors [n, *spatial, c] float32 - `model.posteriors` of the
        reference's FCN branch, NN_extended.py:262-294 - and prediction [n, *spatial] int64 or None).  The posteriors are a view of
        the class-major planes [c, n V] the library wrote (`.movedim(-1, 0)` is that array again).  first_sample: the dropout keys
        of the samples are first_sample .. first_sample + n - 1 (keep_prob < 1)."""
        if not self.dense:
            raise NotImplementedError('forward_maps_device: the model has an fc head (no output map)')
        if float(keep_prob) < 1. and len(self.dropout_layers):
            post, pred = self.forward_dropout_device(t, n, keep_prob, seed=seed, first_sample=first_sample, want_pred=want_pred)
        else:
            post, pred, _ = self.forward_device(t, n, want_pred)
        maps = post.reshape((self.nclass, n) + self.out_map_shape).movedim(0, -1)
        return maps, (pred.reshape((n,) + self.out_map_shape) if pred is not None else None)

    def forward_au_device(self, t, n, keep_prob=1., seed=None, want_output=True):
        """An AU_4U model's `AU_vals` [n, *spatial] and `output` [n, *spatial, c + 1] (or None) on the device: alq_forward_au over
        passes of max_batch; keep_prob < 1 drops as forward_dropout_device does ('MC-sigma')."""
        if not self.AU_4U:
            raise NotImplementedError('forward_au_device: the model has no aleatoric-uncertainty head (AU_4U)')
        torch = self.sess.torch
        self.sess.bind_stream()
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        V, ct = self.out_voxels, self.nclass + 1
        au = self.sess.empty((n * V,), torch.float32)
        out = self.sess.empty((n * V, ct), torch.float32) if want_output else None
        for a, b in self._cuts(n):
            check(self.lib.alq_forward_au(self._m, self._patch_ptr(t, a), b - a, kp, seed, a, arr, nl, None, None, ptr(au, a * V * 4),
                                          ptr(out, a * V * ct * 4)))
        return au.reshape((n,) + self.out_map_shape), (out.reshape((n,) + self.out_map_shape + (ct,)) if want_output else None)

    def forward(self, x, want=('posteriors',), keep_prob=1.):
        t, n = self._as_device_batch(x)
        if float(keep_prob) < 1. and len(self.dropout_layers):
            if 'feature_layer' in want:
                raise NotImplementedError('feature_layer at keep_prob < 1')
            (post, pred), feat = self.forward_dropout_device(t, n, keep_prob, want_pred='prediction' in want), None
        else:
            post, pred, feat = self.forward_device(t, n, 'prediction' in want, 'feature_layer' in want)
        res = {'posteriors': post.cpu().numpy()}
        if pred is not None:
            res['prediction'] = pred.cpu().numpy()
        if feat is not None:
            f = feat.cpu().numpy()
            if self._feature_perm is not None:
                f = f[:, self._feature_perm]
            res['feature_layer'] = np.ascontiguousarray(f.T)       # [F, n] like the reference
        return res

    @_fc_only
    def fisher_device(self, t, n, p1_in=None, diag_load=1e-5, want=('p1', 'g0', 'g1', 'A', 'trace', 'Asum'), rows=None):
        """Device-resident Fisher scoring of n patches (t: device fp32; with `rows`, rows of the resident pool `t`:
        alq_fisher_rows).  Returns device tensors; 'Asum' is the sum over the n patches (fixed summation order per
        launch).  'H' (Shannon entropy of the posteriors, alq_score_entropy) is produced on request."""
        torch = self.sess.torch
        self.sess.bind_stream()
        check_tensor(rows, torch.int64, n, optional=True)
        L = self.L
        out = {}
        out['p1'] = self.sess.empty((n,), torch.float32) if 'p1' in want else None
        out['g0'] = self.sess.empty((n, L), torch.float64) if 'g0' in want else None
        out['g1'] = self.sess.empty((n, L), torch.float64) if 'g1' in want else None
        out['A'] = self.sess.empty((n, L, L), torch.float64) if 'A' in want else None
        out['trace'] = self.sess.empty((n,), torch.float64) if 'trace' in want else None
        asum = torch.zeros((L, L), dtype=torch.float64, device=self.sess.device) if 'Asum' in want else None

        # Device passes of max_batch patches alternate between two PIPELINES (own libalq context = own stream pair, own
        # workspaces, the same weights): the tail of one pass (the last box-filter dot products, finalisation) and its
        # small kernels run beside the next pass's first launches instead of leaving the chip idle.  Each pass is the same
        # launches on the same data whichever pipeline runs it, so every per-patch output is bit-identical to ALQ_LANES=1;
        # the passes' partial sums of A are added in pass order after the join.  pass_cut gives an EVEN number of equal passes, so
        # that two pipelines get the same work; it does not depend on the number of pipelines, so the sum of A is the same bits with
        # one, two or three (DESIGN.md section 6 has the measurements).
        step, starts = self.pass_cut(n)
        nl = min(self.lanes, len(starts))
        extra = self._extra_lanes(nl - 1) if nl > 1 else []
        part = self.sess.empty((max(len(starts), 1), L, L), torch.float64) if asum is not None else None
        cur = torch.cuda.current_stream(self.sess.device)
        # with several pipelines whole passes overlap and the per-context side streams only compete for the same gaps (274.4 ->
        # 277.8 k patches/s without them); a single pipeline keeps its side stream (+3.4 %).  Same kernels, same results either way.
        side_on = 0 if (extra and not os.environ.get('ALQ_LANES_SIDE_STREAM')) else 1
        with side_stream(self.lib, self.sess.ctx, side_on):
            for ln in extra:
                check(self.lib.alq_ctx_use_side_stream(ln['sess'].ctx, side_on))
                ln['stream'].wait_stream(cur)          # inputs, output buffers and the weights are ordered on the caller's stream
            for k, a in enumerate(starts):
                b = min(n, a + step)
                outs = (ptr(p1_in, a * 4), float(diag_load), ptr(out['p1'], a * 4), ptr(out['g0'], a * L * 8), ptr(out['g1'], a * L * 8),
                        ptr(out['A'], a * L * L * 8), ptr(out['trace'], a * 8), ptr(part, k * L * L * 8))

                def launch(m):
                    if rows is None:
                        check(self.lib.alq_fisher(m, self._patch_ptr(t, a), b - a, *outs))
                    else:
                        check(self.lib.alq_fisher_rows(m, ptr(t), ptr(rows, a * 8), b - a, *outs))
                which = k % nl
                if which:
                    ln = extra[which - 1]
                    with torch.cuda.stream(ln['stream']):
                        ln['sess'].bind_stream()
                        launch(ln['m'])
                else:
                    launch(self._m)
            for ln in extra:
                cur.wait_stream(ln['stream'])
        if asum is not None:
            for k in range(len(starts)):
                asum += part[k]
        out['Asum'] = asum
        if 'H' in want or 'absdev' in want:
            if out['p1'] is None:
                raise ValueError("'H' / 'absdev' need 'p1' in `want`")
            out['H'] = self.sess.empty((n,), torch.float32) if 'H' in want else None
            out['absdev'] = self.sess.empty((n,), torch.float64) if 'absdev' in want else None
            check(self.lib.alq_score_entropy(self.sess.ctx, ptr(out['p1']), n, ptr(out['absdev']), ptr(out['H'])))
        return out

    @contextlib.contextmanager
    def _creation_env(self):
        """The ALQ_* engine switches are read when a model is created and when its weights are packed: the second pipeline's
        model is built under the ones the first was created with."""
        now = {k: v for k, v in os.environ.items() if k.startswith('ALQ_')}
        for k in now:
            del os.environ[k]
        os.environ.update(self._create_env)
        try:
            yield
        finally:
            for k in self._create_env:
                os.environ.pop(k, None)
            os.environ.update(now)

    def pass_cut(self, n):
        """How fisher_device cuts n patches into device passes: (patches per pass, first patch of every pass)."""
        step = self.max_batch
        if n > self.max_batch and not os.environ.get('ALQ_NO_PASS_BALANCE'):
            P = -(-n // self.max_batch)
            mult = int(os.environ.get('ALQ_PASS_MULT', '2'))          # (tuning experiments)
            P = -(-P // mult) * mult if P >= mult else P + (P & 1)
            step = -(-n // P)
        return step, list(range(0, n, step))

    @property
    def _lane2(self):
        """The first extra pipeline (None until a call needed one): what the tests of round 5 look at."""
        return self._xlanes[0] if self._xlanes else None

    def _extra_lanes(self, count):
        """`count` extra scoring pipelines of fisher_device: each a libalq context on its own torch stream and a model of the same
        layers on it; their weights follow `set_weights` / `set_weights_device`: wide fc layers from the device tensors the first
        model was fed from, the other layers from the host copies in var_dict."""
        torch = self.sess.torch
        while len(self._xlanes) < count:
            stream = torch.cuda.Stream(self.sess.device)
            with torch.cuda.stream(stream):
                sess2 = DeviceSession(self.sess.device.index)
            m = C.c_void_p()
            arr, nl, cd = self._create_args
            with self._creation_env():
                check(self.lib.alq_model_create(sess2.ctx, arr, nl, cd, self.max_batch, C.byref(m)))
            if int(self.lib.alq_model_max_batch(m)) != self.max_batch:
                self.lib.alq_model_destroy(m)
                raise _lib.AlqError('extra pipeline: the library granted another batch size')
            self._xlanes.append(dict(sess=sess2, stream=stream, m=m, version=None))
        for ln in self._xlanes[:count]:
            if ln['version'] != self._weights_version:
                if not self.var_dict.stale and any(v is None for v in self.var_dict.values()):
                    raise RuntimeError('set_weights() has not been called')
                # the pipeline's context runs on its own stream: what fills the device tensors (an upload, the optimiser step) is
                # ordered on the caller's
                ln['stream'].wait_stream(torch.cuda.current_stream(self.sess.device))
                with self._creation_env():
                    for ti, name in enumerate(self.var_names):
                        if self._dev_pack[ti] and self._dev_w[ti] is not None and not self._host_repack:
                            Wd, bd = self._dev_w[ti]
                            with torch.cuda.stream(ln['stream']):
                                ln['sess'].bind_stream()
                                check(self.lib.alq_model_set_weights_device(ln['m'], ti, ptr(Wd), ptr(bd)))
                            continue
                        W, b = self.var_dict[name]
                        check(self.lib.alq_model_set_weights(ln['m'], ti, W.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
                ln['version'] = self._weights_version
        return self._xlanes[:count]

    @_fc_only
    def fisher(self, x, p1=None, diag_load=1e-5):
        t, n = self._as_device_batch(x)
        p1_in = None if p1 is None else self.sess.to_device(np.asarray(p1, dtype=np.float32), self.sess.torch.float32)
        out = self.fisher_device(t, n, p1_in, diag_load)
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}

    def debug_tensor(self, layer_idx, what, n):
        """Test hook (alq_model_debug_copy): internal tensor of the last forward/fisher call."""
        torch = self.sess.torch
        e = C.c_int64()
        # size query by over-allocation: the largest activation of a patch is bounded by 64x input
        buf = self.sess.empty((n * max(self.elems_per_patch * 64, 1 << 16),), torch.float32)
        check(self.lib.alq_model_debug_copy(self._m, int(layer_idx), int(what), int(n), ptr(buf), C.byref(e)))
        return buf[:e.value].cpu().numpy()

    def close(self):
        for ln in getattr(self, '_xlanes', []):
            self.lib.alq_model_destroy(ln['m'])
            ln['sess'].close()
        self._xlanes = []
        if getattr(self, 'teacher', None) is not None:
            self.teacher.close()
        if self._m:
            self.lib.alq_model_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
