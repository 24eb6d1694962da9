"""Gradient entry points of a device model, a mixin of device.DeviceModel: parameter gradients and their squared norms, Hessian-
vector products, diagonal Fisher, class layer sums, last-layer closed forms (csrc/grads, gnorm, hvp, dfisher, lsum, llfc .hip)."""
import ctypes as C
import os

import numpy as np

from ._lib import ALQ_FC, check, check_tensor, ptr
from .device_host import _fc_only


class ModelGrads(object):
    @_fc_only
    def param_grads_device(self, t, n, mode, cls=0, labels=None, loss_scale=1., keep_prob=1., seed=None, first_sample=0,
                           per_sample=True, want_post=False, want_loss=False):
        """alq_param_grads on n device patches (n <= max_batch): mode 0 = gradients of log posteriors[cls, .] per sample,
        mode 1 = gradient of loss_scale * sum CE.  Returns (grads [n, P] or [P], post [c, n] or None, loss or None)."""
        torch = self.sess.torch
        self.sess.bind_stream()
        if n > self.max_batch:
            raise ValueError('%d patches exceed max_batch = %d' % (n, self.max_batch))
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        g = self.sess.empty((n, self.num_params) if per_sample else (self.num_params,), torch.float32)
        post = self.sess.empty((self.nclass, n), torch.float32) if want_post else None
        loss = self.sess.empty((1,), torch.float64) if want_loss else None
        lab = None
        if mode == 1:
            lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels, dtype=np.int32), torch.int32)
        check(self.lib.alq_param_grads(self._m, ptr(t), n, int(mode), int(cls), ptr(lab), float(loss_scale), kp, seed, int(first_sample),
                                       arr, nl, 1 if per_sample else 0, ptr(g), ptr(post), ptr(loss)))
        return g, post, loss

    @_fc_only
    def grad_sqnorms_device(self, t, n, cls=-1, cls_per_sample=None):
        """alq_grad_sqnorms over device passes of max_batch patches: [n, 2L'] float64 on the device, column 2t' =
        ||dW||^2 and 2t' + 1 = ||db||^2 of the t'-th layer of `grad_layers` (all layers when empty).  cls = -1: the
        unit-cotangent gradient u = d(z0 - z1) / d theta of a two-class net; cls in [0, c): d log posteriors[cls] /
        d theta; cls_per_sample (int array or device int32 tensor [n]) overrides cls per sample.  Rows do not depend
        on the pass cut."""
        torch = self.sess.torch
        self.sess.bind_stream()
        L = self.L
        dc = cls_per_sample
        if dc is not None and not isinstance(dc, torch.Tensor):
            dc = self.sess.to_device(np.asarray(dc, dtype=np.int32).reshape(n), torch.int32)
        check_tensor(dc, torch.int32, n, optional=True)
        sq = self.sess.empty((n, 2 * L), torch.float64)
        for a, b in self._cuts(n):
            check(self.lib.alq_grad_sqnorms(self._m, self._patch_ptr(t, a), b - a, int(cls), ptr(dc, a * 4), None, ptr(sq, a * 2 * L * 8)))
        if list(self.grad_layer_idx) != list(range(L)):
            cols = [2 * i + h for i in self.grad_layer_idx for h in (0, 1)]
            sq = sq[:, cols].contiguous()
        return sq

    @_fc_only
    def grad_log_post(self, x, j, keep_prob=1.):
        """`sess.run(model.grad_posts[str(j)], {x: batch})`: gradients of log posteriors[j, 0] - sample 0 of the batch,
        like the reference's graph node (NN.py:639-645) - w.r.t. the variables of `grad_layers`, TF shapes."""
        t, n = self._as_device_batch(x)
        g, _, _ = self.param_grads_device(t, 1, 0, cls=j, keep_prob=keep_prob)
        return self.unflatten(g[0].cpu().numpy(), self.grad_layer_idx)

    # -- Hessian-vector products (Influence.py:64-166) ---------------------------------------
    def hess_layer_idx(self, layers='all'):
        """Parameterised-layer indices of `layers`: 'all' / None, layer names (the reference's Hess_layers) or indices."""
        if layers is None or (isinstance(layers, str) and layers == 'all'):
            return list(range(self.L))
        idx = [self.var_names.index(l) if isinstance(l, str) else int(l) for l in layers]
        if len(idx) == 0 or len(set(idx)) != len(idx) or min(idx) < 0 or max(idx) >= self.L:
            raise KeyError('Hessian layers %r' % (layers,))
        return idx

    def _param_offsets(self):
        off, out = 0, []
        for _, wshape, bshape in self.param_shapes:
            nw, nb = int(np.prod(wshape)), int(np.prod(bshape))
            out.append((off, nw, nb))
            off += nw + nb
        return out

    def ravel_for_layers(self, v, idx):
        """`v` - a flat vector over all parameters, a flat vector over the layers `idx` (in that order) or a list
        [VW, Vb, ...] of arrays for them - as a flat float32 vector [P] in parameter order (zero outside `idx`)."""
        offs = self._param_offsets()
        if isinstance(v, (list, tuple)):
            if len(v) != 2 * len(idx):
                raise ValueError('expected %d arrays (W, b per layer), got %d' % (2 * len(idx), len(v)))
            v = np.concatenate([np.asarray(a, dtype=np.float32).ravel() for a in v])
        v = np.asarray(v, dtype=np.float32).ravel()
        if v.size == self.num_params:
            return np.ascontiguousarray(v)
        if v.size != sum(offs[t][1] + offs[t][2] for t in idx):
            raise ValueError('vector of %d entries fits neither all %d parameters nor the chosen layers' % (v.size, self.num_params))
        full = np.zeros(self.num_params, dtype=np.float32)
        c = 0
        for t in idx:
            o, nw, nb = offs[t]
            full[o:o + nw + nb] = v[c:c + nw + nb]
            c += nw + nb
        return full

    def _require_default_objective(self, what):
        """The exact R-operator (csrc/hvp.hip) is that of the batch-mean cross-entropy: a model whose loss set_hypers changed
        has no Hessian-vector product, whichever way it is asked for."""
        if self._obj is not None:
            raise NotImplementedError('%s of a non-default objective (set_hypers): the R-operator covers the batch-mean '
                                      'cross-entropy only' % what)

    @_fc_only
    def hess_vecp_device(self, t, n, labels, v, idx=None, loss_scale=1., out=None, want_loss=False):
        """alq_hess_vecp on n device patches (any n: passes of max_batch with the same loss_scale): `out` (float64 device
        [P]; created and overwritten when None) += H v, H the Hessian of loss_scale * sum CE over the layers `idx` (indices;
        None = all).  labels / v: int32 [n] / float32 [P] device tensors.  Returns (out, scaled loss of the passes or None)."""
        self._require_default_objective('hess_vecp')      # every caller: hess_vecp, sess.run, PW_NN.batch_eval, Influence
        torch = self.sess.torch
        self.sess.bind_stream()
        check_tensor(labels, torch.int32, n)
        check_tensor(v, torch.float32, self.num_params)
        on = None
        if idx is not None and sorted(idx) != list(range(self.L)):
            on = (C.c_uint8 * self.L)(*[1 if q in idx else 0 for q in range(self.L)])
        acc = out is not None
        if out is None:
            out = self.sess.empty((self.num_params,), torch.float64)
        check_tensor(out, torch.float64, self.num_params)
        loss = self.sess.empty((1,), torch.float64) if want_loss else None
        total = torch.zeros((1,), dtype=torch.float64, device=self.sess.device) if want_loss else None
        for a, b in self._cuts(n):
            check(self.lib.alq_hess_vecp(self._m, self._patch_ptr(t, a), b - a, ptr(labels, a * 4), float(loss_scale), ptr(v), on,
                                         1 if (acc or a > 0) else 0, ptr(out), ptr(loss)))
            if want_loss:
                total += loss
        return out, total

    @_fc_only
    def hess_vecp(self, x, labels, v, layers='all', loss_scale=None, out=None):
        """H v for the Hessian of loss_scale * sum_n CE(softmax(z_n), labels[n]) (loss_scale None: 1 / n, the mean loss of
        NN.py:583-588) over the parameters of `layers` ('all', names or indices; the others are held constant).  `v`: see
        ravel_for_layers.  Returns the list [HW, Hb, ...] of the chosen layers in TF shapes, float64.  `out`: a float64
        device vector [P] the product is ADDED to (multi-pass sums); the list then holds the accumulated values."""
        self._require_default_objective('hess_vecp')
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        idx = self.hess_layer_idx(layers)
        lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        vd = self.sess.to_device(self.ravel_for_layers(v, idx), torch.float32)
        hv, _ = self.hess_vecp_device(t, n, lab, vd, idx, 1. / n if loss_scale is None else loss_scale, out)
        return self.unflatten(hv.cpu().numpy(), idx)

    @_fc_only
    def diagonal_fisher_device(self, t, n, labels):
        """alq_diag_fisher over device passes of max_batch patches: the mean over the n samples of the squared gradient of
        log posteriors[labels[i], i], flat float64 device tensor [P] in parameter order.  No per-sample gradient rows are
        formed; labels: int array or int32 device tensor [n]."""
        torch = self.sess.torch
        self.sess.bind_stream()
        lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        check_tensor(lab, torch.int32, n)
        acc = torch.zeros((self.num_params,), dtype=torch.float64, device=self.sess.device)
        for a, b in self._cuts(n):
            check(self.lib.alq_diag_fisher(self._m, self._patch_ptr(t, a), b - a, ptr(lab, a * 4), ptr(acc)))
        return acc.div_(max(n, 1))

    @_fc_only
    def diagonal_fisher(self, x, labels=None, batch=None, fused=None):
        """model_utils.diagonal_Fisher (model_utils.py:294-330): mean over samples of the squared gradient of the
        log-likelihood of the sample's label (labels given) or of the model's own prediction (None), per parameter.
        Returns the list of arrays in variable shapes.  Default: the fused statistic (diagonal_fisher_device); fused=False or
        ALQ_DIAGF_ROWS=1: per-sample gradient rows squared and folded (alq_param_grads + alq_sq_accum), the A/B arm; `batch`
        caps the rows of one of its passes (the fused arm forms none and runs passes of max_batch)."""
        t, n = self._as_device_batch(x)
        if labels is None:
            post, pred, _ = self.forward_device(t, n, want_pred=True)
            labels = pred.cpu().numpy()
        labels = np.asarray(labels).astype(np.int64)
        if fused is None:
            fused = os.environ.get('ALQ_DIAGF_ROWS', '0') in ('', '0')
        if fused:
            return self.unflatten(self.diagonal_fisher_device(t.reshape(n, -1), n, labels.astype(np.int32)).cpu().numpy())
        return self.unflatten(self.diagonal_fisher_rows_device(t, n, labels, batch).cpu().numpy())

    @_fc_only
    def diagonal_fisher_rows_device(self, t, n, labels, batch=None):
        """The rows arm of diagonal_fisher on the device (A/B; tools/gpu_diagfisher.py): per class, the per-sample gradient rows
        of up to `batch` samples (alq_param_grads) squared and folded (alq_sq_accum).  labels: host int array [n].  Flat
        float64 device tensor [P], the mean over the n samples."""
        torch = self.sess.torch
        labels = np.asarray(labels).astype(np.int64)
        acc = torch.zeros((self.num_params,), dtype=torch.float64, device=self.sess.device)
        step = min(self.max_batch, batch or self.max_batch)
        for j in range(self.nclass):
            idx = np.nonzero(labels == j)[0]
            for a in range(0, len(idx), step):
                sel = self.sess.to_device(idx[a:a + step], torch.int64)
                xs = t.reshape(n, -1).index_select(0, sel)
                g, _, _ = self.param_grads_device(xs, int(sel.numel()), 0, cls=j)
                check(self.lib.alq_sq_accum(self.sess.ctx, ptr(g), self.num_params, int(sel.numel()), ptr(acc)))
        return acc.div_(max(n, 1))

    # -- last-layer closed forms (NN.py:874-1029, PW_NNAL.py:851-881) -------------------------
    _LLFC_SLICE = 32768        # samples / columns per launch (alq.h: at most 65535; they are independent)

    def _require_llfc(self):
        """The closed forms take `feature_layer` as the input u of the last fc layer."""
        wshape = self.param_shapes[-1][1]
        if self.feature_idx is None or self.layers[-1]['type'] != ALQ_FC or self.feature_dim * self.nclass != int(np.prod(wshape)):
            raise ValueError('feature_layer (%r, %d values) is not the input of the last fc layer (weights %r)' %
                             (self.feature_idx, self.feature_dim, tuple(wshape)))

    @_fc_only
    def llfc_reference_order(self):
        """Index vector [P]: entry j*d + i of a reference-ordered last-layer vector (NN.py:296-301 flatten order) is entry
        idx[j*d + i] of the device's (feature-memory order); the biases keep their places."""
        d, c = self.feature_dim, self.nclass
        perm = self._feature_perm if self._feature_perm is not None else np.arange(d)
        return np.concatenate([(np.arange(c)[:, None] * d + np.asarray(perm)[None, :]).reshape(-1), c * d + np.arange(c)])

    @_fc_only
    def llfc_grads_device(self, feat, post, labels):
        """alq_llfc_grads: the gradients of log posteriors[labels[n], n] with respect to the last fc layer, float32 device
        tensor [n, (d+1)c] (W class-major, then b), from device tensors feat [n, d], post [c, n] (forward_device) and labels
        (int array or device tensor [n]).  Features in the device's memory order (llfc_reference_order)."""
        torch = self.sess.torch
        self._require_llfc()
        self.sess.bind_stream()
        n, d, c = int(feat.shape[0]), self.feature_dim, self.nclass
        lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels).reshape(n), torch.int32)
        lab = lab.to(torch.int32).contiguous()
        check_tensor(feat, torch.float32)
        assert tuple(feat.shape) == (n, d)
        assert post.dtype == torch.float32 and tuple(post.shape) == (c, n) and int(lab.numel()) == n
        out = self.sess.empty((n, (d + 1) * c), torch.float32)
        for a in range(0, n, self._LLFC_SLICE):
            b = min(n, a + self._LLFC_SLICE)
            pb = post[:, a:b].contiguous()
            check(self.lib.alq_llfc_grads(self.sess.ctx, ptr(feat, a * d * 4), ptr(pb), ptr(lab, a * 4), b - a, d, c, ptr(out, a * (d + 1) * c * 4)))
        return out

    def _require_llfc_hess_fits(self):
        """Before anything is computed or allocated: the explicit matrix must stay under the library's byte cap."""
        self._require_llfc()
        P = (self.feature_dim + 1) * self.nclass
        cap = int(self.lib.alq_llfc_hess_max_bytes())
        if P * P * 8 > cap:
            raise ValueError('the explicit last-layer Hessian of (d+1)c = %d parameters takes %d bytes (cap %d): use the implicit '
                             'routes, PW_NNAL.stoch_approx_IF / DeviceModel.llfc_stoch_if_device' % (P, P * P * 8, cap))

    @_fc_only
    def llfc_hess_device(self, feat_one, post_one):
        """alq_llfc_hess: the explicit [(d+1)c, (d+1)c] float64 Hessian of one sample's loss in the last fc layer."""
        torch = self.sess.torch
        self._require_llfc_hess_fits()
        d, c = self.feature_dim, self.nclass
        P = (d + 1) * c
        self.sess.bind_stream()
        f = feat_one.reshape(-1).contiguous()
        p = post_one.reshape(-1).contiguous()
        check_tensor(f, torch.float32, d)
        check_tensor(p, torch.float32, c)
        H = self.sess.empty((P, P), torch.float64)
        check(self.lib.alq_llfc_hess(self.sess.ctx, ptr(f), ptr(p), d, c, ptr(H)))
        return H

    @_fc_only
    def llfc_stoch_if_features_device(self, pool_feat, pool_post, pool_labels, tr_feat, tr_post, draws, scale, path=0):
        """alq_llfc_stoch_if on features that are already there: pool_feat [n_pool, d], pool_post [c, n_pool], tr_feat [n_tr, d],
        tr_post [c, n_tr] float32 device tensors, `draws` indices into the training rows.  float32 device tensor [n_pool, (d+1)c]."""
        torch = self.sess.torch
        self.sess.bind_stream()
        d, c = int(pool_feat.shape[1]), int(pool_post.shape[0])
        n_pool, n_tr = int(pool_feat.shape[0]), int(tr_feat.shape[0]) if tr_feat is not None else 0
        draws = np.asarray(draws, dtype=np.int64).reshape(-1)
        T = int(draws.size)
        if T and (n_tr < 1 or draws.min() < 0 or draws.max() >= n_tr):
            raise ValueError('draws outside the %d training samples' % n_tr)
        dr = self.sess.to_device(draws.astype(np.int32), torch.int32) if T else None
        lab = pool_labels.to(torch.int32).contiguous()
        for t_ in (pool_feat, tr_feat):
            check_tensor(t_, torch.float32, optional=True)
            assert t_ is None or int(t_.shape[1]) == d
        tp = tr_post.contiguous() if tr_post is not None else None
        P = (d + 1) * c
        V = self.sess.empty((n_pool, P), torch.float32)
        for a in range(0, n_pool, self._LLFC_SLICE):
            b = min(n_pool, a + self._LLFC_SLICE)
            pb = pool_post[:, a:b].contiguous()
            work = self.sess.empty((max(int(self.lib.alq_llfc_if_work_bytes(b - a, c)), 8),), torch.uint8)
            check(self.lib.alq_llfc_stoch_if(self.sess.ctx, ptr(pool_feat, a * d * 4), ptr(pb), ptr(lab, a * 4), b - a, ptr(tr_feat), ptr(tp),
                                             n_tr, ptr(dr), T, float(scale), d, c, int(path), ptr(V, a * P * 4), ptr(work)))
        return V

    @_fc_only
    def llfc_stoch_if_device(self, pool_t, n_pool, tr_t, draws, scale, path=0):
        """The recursion of PW_NNAL.stoch_approx_IF on the device: V_0 = the last-layer gradients of the n_pool device patches
        `pool_t` at their predicted labels, then one step per entry of `draws` (row indices into the device patches `tr_t`).
        One forward pass over the pool and one over the training patches; nothing leaves the device.  Returns (V float32 device
        [n_pool, (d+1)c] in the device's feature order - llfc_reference_order - and the predicted labels, int64 device [n_pool])."""
        self._require_llfc()
        post, pred, feat = self.forward_device(pool_t, n_pool, want_pred=True, want_feat=True)
        tpost = tfeat = None
        if len(draws):
            n_tr = int(tr_t.numel()) // self.elems_per_patch
            tpost, _, tfeat = self.forward_device(tr_t, n_tr, want_feat=True)
        return self.llfc_stoch_if_features_device(feat, post, pred, tfeat, tpost, draws, scale, path), pred

    @_fc_only
    def shrunk_class_gradients(self, x):
        """g [n, c, L'] float64: shrink_gradient(d log posteriors[j, sample] / d theta, 'sum') for every sample and class -
        what the reference obtains with one session.run(model.grad_posts[str(j)]) per sample and class plus a host
        reduction (NNAL.py:381-405, NNAL_tools.py:784-796).  Per device pass: alq_param_grads (mode 0, per-sample rows)
        for class j, alq_shrink_sum on the rows; nothing of size |theta| reaches the host.  L' = the layers of
        `grad_layers` (all when empty).  Also returns the posteriors [c, n] of these passes (device fp32).
        The A/B arm of the query since class_layer_sums_device (fisher_classes(..., fused=False), ALQ_FI_ROWS=1)."""
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        c, L = self.nclass, self.L
        elems = (C.c_int64 * L)(*[int(np.prod(w)) + int(np.prod(b)) for _, w, b in self.param_shapes])
        g = self.sess.empty((n, c, L), torch.float64)
        post = self.sess.empty((c, n), torch.float32)
        tmp = self.sess.empty((min(n, self.max_batch), L), torch.float64)
        flat = t.reshape(n, -1)
        for a, b in self._cuts(n):
            for j in range(c):
                rows, pb, _ = self.param_grads_device(flat[a:b], b - a, 0, cls=j, want_post=(j == 0))
                if j == 0:
                    post[:, a:b] = pb
                check(self.lib.alq_shrink_sum(self.sess.ctx, ptr(rows), b - a, self.num_params, elems, L, ptr(tmp)))
                g[a:b, j, :] = tmp[:b - a]
        return self._grad_layer_columns(g), post

    @_fc_only
    def class_layer_sums_device(self, t, n, classes):
        """alq_class_layer_sums over device passes of max_batch samples: g [n, J, L'] float64 on the device, g[i, j] =
        shrink_gradient(d log posteriors[classes[i, j], i] / d theta, 'sum') over the layers of `grad_layers` (all when
        empty), like shrunk_class_gradients but for the class slots given per sample and with nothing of the size of theta
        formed: per pass one forward pass, one field launch per layer, then per slot a backward-data sweep with the fused
        mask + channel-sum + dot kernels (csrc/lsum.hip).  classes: int array [n, J], entries in [0, c); the slots of a pass
        are uploaded with it.  Rows do not depend on the pass cut."""
        torch = self.sess.torch
        self.sess.bind_stream()
        classes = np.asarray(classes)
        if classes.ndim != 2 or classes.shape[0] != n or not 1 <= classes.shape[1] <= 64:
            raise ValueError('classes must be [n = %d, J] with 1 <= J <= 64, got %r' % (n, classes.shape))
        J, L = int(classes.shape[1]), self.L
        g = self.sess.empty((n, J, L), torch.float64)
        flat = t.reshape(n, -1)
        for a, b in self._cuts(n):
            dc = self.sess.to_device(np.ascontiguousarray(classes[a:b].T, dtype=np.int32), torch.int32)      # [J][b - a]
            check(self.lib.alq_class_layer_sums(self._m, ptr(flat[a:b]), b - a, J, ptr(dc), None, ptr(g, a * J * L * 8)))
        return self._grad_layer_columns(g)

    def _grad_layer_columns(self, g):
        idx = list(self.grad_layer_idx)
        return g if idx == list(range(self.L)) else g[:, :, idx].contiguous()

    @staticmethod
    def class_slots(W):
        """The slot form of per-sample class weights W [n, c] (0 = class not kept): (classes [n, J] int, weights [n, J]) with
        J the largest kept-class count over the samples; slot j of sample i is its j-th kept class in ascending class order,
        spare slots repeat class 0 with weight 0.  sum_j weights[i, j] g(classes[i, j]) g(..)^T = sum_c W[i, c] g(c) g(c)^T."""
        W = np.asarray(W, dtype=np.float64)
        n = W.shape[0]
        kept = [np.flatnonzero(W[i] != 0.) for i in range(n)]
        J = max(1, max(len(k) for k in kept)) if n else 1
        classes = np.zeros((n, J), dtype=np.int64)
        weights = np.zeros((n, J))
        for i, k in enumerate(kept):
            classes[i, :len(k)] = k
            weights[i, :len(k)] = W[i, k]
        return classes, weights

    @_fc_only
    def fisher_classes(self, x, W, diag, fused=None):
        """A [n, L', L'] float64 = sum_j W[i, j] g_ij g_ij^T + diag[i] I (alq_fisher_classes).  fused (default; None = on unless
        ALQ_FI_ROWS=1): only the classes with a non-zero weight are differentiated, as class slots (class_slots) through
        class_layer_sums_device, and alq_fisher_classes runs over the J slots.  Otherwise the gradients of all c classes come
        from shrunk_class_gradients (alq_param_grads rows + alq_shrink_sum per class): the A/B arm."""
        torch = self.sess.torch
        if fused is None:
            fused = os.environ.get('ALQ_FI_ROWS', '0') in ('', '0')
        if fused:
            t, n = self._as_device_batch(x)
            classes, W = self.class_slots(np.asarray(W, dtype=np.float64).reshape(n, self.nclass))
            g = self.class_layer_sums_device(t, n, classes)
        else:
            g, _ = self.shrunk_class_gradients(x)
        n, c, L = [int(v) for v in g.shape]
        Wd = self.sess.to_device(np.asarray(W, dtype=np.float64).reshape(n, c), torch.float64)
        dd = self.sess.to_device(np.asarray(diag, dtype=np.float64).reshape(n), torch.float64)
        A = self.sess.empty((n, L, L), torch.float64)
        self.sess.bind_stream()
        check(self.lib.alq_fisher_classes(self.sess.ctx, ptr(g), ptr(Wd), ptr(dd), n, c, L, ptr(A)))
        return A.cpu().numpy()
