"""Training of a device model, a mixin of device.DeviceModel: hypers and optimiser of NN / NN_extended, the objective pass, mean-
teacher training, partial fine-tuning and the train step (csrc/train.hip, loss.hip, mteach.hip)."""
import ctypes as C

import numpy as np

from ._lib import LossT, check, check_tensor, ptr
from .device_host import Handle, nonzero_weight_count


class ModelTrain(object):
    def _check_input_weights(self, input_weights):
        """Per-sample weights belong to NN_extended.get_loss (NN_extended.py:1252-1255); NN.py's loss has none."""
        if input_weights is not None and self._obj is None and not self.dense:
            raise ValueError('input_weights on a model without training hypers: the batch-mean cross-entropy of NN.py:583-588 '
                             'takes no sample weights (build the NN_extended.CNN with loss_name=\'CE\' for the weighted mean)')

    def mean_loss(self, x, labels, targets=None, input_weights=None):
        """`sess.run(model.loss, {x, y_})`: the mean softmax cross-entropy of the batch (unlabelled samples add 0 to the sum),
        or the model's own objective once set_hypers gave it one (forward passes + alq_loss_stats; `targets` [c, n]: the
        soft targets of CE_softclasses / GCE, one-hot columns of `labels` when None; `input_weights` [n])."""
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        self._check_input_weights(input_weights)
        if self._obj is not None or self.dense:
            y = self._onehot(labels, n * self.out_voxels) if targets is None else targets
            return self._objective_pass(t, n, y, 1., None, input_weights, None, want_grad=False)[1]
        lab = self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        loss = 0.
        for a, b in self._cuts(n):
            _, _, l = self.param_grads_device(t[a:b], b - a, 1, labels=lab[a:b], loss_scale=1. / n, per_sample=False, want_loss=True)
            loss += float(l.item()) * (b - a) / n
        return loss

    def mean_loss_grad(self, x, labels, layers='all', targets=None, input_weights=None):
        """`sess.run(model.loss_grad, {x, y_})` (NN.add_loss_grad, NN.py:862-871): gradient of the mean cross-entropy with
        respect to the variables of `layers`, TF shapes (alq_param_grads mode 1) - of the model's own objective once set_hypers
        gave it one (alq_param_grads_loss; `targets` / `input_weights` as in mean_loss)."""
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        self._check_input_weights(input_weights)
        if self._obj is not None or self.dense:
            y = self._onehot(labels, n * self.out_voxels) if targets is None else targets
            g, _ = self._objective_pass(t, n, y, 1., None, input_weights, None)
            return self.unflatten(g.cpu().numpy(), self.hess_layer_idx(layers))
        lab = self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        g = torch.zeros((self.num_params,), dtype=torch.float64, device=self.sess.device)
        for a, b in self._cuts(n):
            gp, _, _ = self.param_grads_device(t[a:b], b - a, 1, labels=lab[a:b], loss_scale=1. / n, per_sample=False)
            g += gp
        return self.unflatten(g.cpu().numpy().astype(np.float32), self.hess_layer_idx(layers))

    # -- training step (get_optimizer / train_step, NN.py:557-615) --------------------------
    def set_hypers(self, hypers):
        """NN_extended.CNN.set_hypers (NN_extended.py:24-63) for the keys a device step reads (NN_extended.CNN.DEFAULT_HYPERS):
        from here on the model's loss is NN_extended.get_loss's (:1221-1277) and get_optimizer() takes no arguments."""
        from . import losses
        torch = self.sess.torch
        h = dict(hypers)
        kind = losses.KINDS[h.get('loss_name', 'CE')]
        bcw, gamma = h.get('bin_class_weights'), h.get('focal_gamma')
        if (bcw is not None or gamma is not None) and self.nclass != 2:
            raise ValueError('bin_class_weights / focal_gamma need a two-class net, got %d classes' % self.nclass)
        if kind == losses.GCE and float(h.get('q', 0.7)) == 0:
            raise ValueError('q cannot be equal to zero.')
        self.hypers = h
        self._obj = dict(kind=kind, divisor='nonzero', q=float(h.get('q', 0.7)),
                         gamma=float(gamma) if (gamma is not None and kind == losses.CE) else None,
                         class_w=self.sess.to_device(np.asarray(bcw, dtype=np.float32).reshape(2), torch.float32)
                         if (bcw is not None and kind == losses.CE) else None)

    def get_optimizer(self, learning_rate=None, train_layers=[], optimizer_name=None):
        """Mean softmax cross-entropy + SGD or Adam on all layers or on `train_layers` (NN.py:583-615).  Without arguments
        (NN_extended.get_optimizer, NN_extended.py:1380-1449): the optimiser - SGD, Adam(beta1, beta2) or RMSProp(decay, momentum,
        epsilon) - and the learning rate (`learning_rate`, else `lr_schedule(step)` evaluated on the host before every step,
        step = 0 before the first) of the model's hypers; `train_layers` as set on the model before the call, if at all."""
        h = self.hypers or {}
        if learning_rate is None and optimizer_name is None and not train_layers:
            if self.hypers is None:
                raise TypeError('get_optimizer() without arguments needs the hyper-parameters of an NN_extended.CNN')
            train_layers = list(getattr(self, 'train_layers', []))
        if optimizer_name is None:
            optimizer_name = h.get('optimizer_name', 'SGD')
        if optimizer_name not in ('SGD', 'Adam', 'RMSProp'):
            raise NotImplementedError('optimizer %r (SGD, Adam and RMSProp are known)' % (optimizer_name,))
        if self.AU_4U and self._mt is None:
            raise NotImplementedError('an AU_4U model trains with MT_SSL: its log-variance channel has a gradient only under the '
                                      'consistency term')
        schedule = None
        if learning_rate is None:
            learning_rate = h.get('learning_rate')
            if learning_rate is None:
                schedule = h.get('lr_schedule')
                if schedule is None:
                    raise ValueError('neither learning_rate nor lr_schedule is set')
                learning_rate = schedule(0)
        for nme in train_layers:
            if nme not in self.var_names:
                raise KeyError('train layer %r' % (nme,))
        self.train_layers = list(train_layers)
        self.train_step = Handle('train_step')
        self.train_step.model = self
        self._opt = dict(name=optimizer_name, lr=float(learning_rate), schedule=schedule, t=0, theta=None, m=None, v=None,
                         beta1=float(h.get('beta1', 0.9)), beta2=float(h.get('beta2', 0.999)), decay=float(h.get('decay', 0.9)),
                         momentum=float(h.get('momentum', 0.)), epsilon=float(h.get('epsilon', 1e-10)))
        if self._mt is not None:
            self._build_teacher()

    # -- mean-teacher consistency training (NN_extended.py:913-926, :1337-1396) -------------
    @property
    def global_step(self):
        """Optimiser steps taken so far (the reference's `global_step` variable)."""
        return self._opt['t'] if self._opt is not None else 0

    def set_mean_teacher(self, mt):
        """MT_SSL of NN_extended.CNN: `mt` holds output_perturbation_measure, MT_ema_decay_schedule, Gaussian_noise_std,
        rotation_angle, max_cons_coeff and rampup_length.  get_optimizer() then builds the teacher."""
        from . import mteach
        if not self.dense:
            raise NotImplementedError('mean-teacher training is defined for fully-convolutional models')
        if mt.get('rotation_angle') is not None and len(self.in_shape) != 3:
            raise ValueError('rotation_angle on a 3-D model')
        self._mt = dict(measure=mteach.MEASURES[mt['output_perturbation_measure']], decay=mt['MT_ema_decay_schedule'],
                        std=float(mt['Gaussian_noise_std'] or 0.), angle=mt.get('rotation_angle'),
                        max_coeff=float(mt['max_cons_coeff']), rampup=float(mt['rampup_length']), shadow=None, tver=0)
        self.cons_coeff = mteach.cons_coeff(0, self._mt['rampup'], self._mt['max_coeff'])

    def _build_teacher(self):
        """get_FCN_loss with MT_SSL (NN_extended.py:1337-1396): a second model over the same layers on the same session whose
        weights are the moving averages of this model's, its input `perturbed_x`, and the handles of the step."""
        from .device_model import DeviceModel
        drop = [self.dropout_layers, self.dropout_rate] if len(self.dropout_layers) else None
        if getattr(self, 'teacher', None) is not None:      # (a second get_optimizer(): a new teacher, as a new graph would hold)
            self.teacher.close()
        self.teacher = DeviceModel(self.sess, self.layer_dict, self.in_shape, self.skips, None, drop, self.max_batch,
                                   self.name + '_teacher', aleatoric=self.AU_4U, au_log_rel_coeff=self.AU_log_rel_coeff)
        self.perturbed_x = Handle('perturbed_x')
        for nme in ('ema_apply', 'labeled_loss', 'cons_loss'):
            h = Handle(nme)
            h.model = self
            setattr(self, nme, h)
        self._mt.update(shadow=None, tver=0)

    def _student_theta(self):
        """This model's weights as a flat device vector: the optimiser's own when it is current."""
        o = self._opt
        if o is not None and o['theta'] is not None and o.get('version') == self._weights_version:
            return o['theta']
        return self.sess.to_device(self.flat_params(), self.sess.torch.float32)

    def _mt_shadow(self):
        """The teacher's weights, flat fp32 on the device.  They start as a copy of this model's weights at the first use -
        of the teacher's own when teacher.set_weights / load_weights was called (again after every later such call)."""
        mt, T = self._mt, self.teacher
        if mt['shadow'] is None or T._weights_version != mt['tver']:
            src = self._student_theta() if T._weights_version == 0 else self.sess.to_device(T.flat_params(), self.sess.torch.float32)
            mt['shadow'] = src.clone()
            T.set_weights_device(mt['shadow'])
            mt['tver'] = T._weights_version
        return mt['shadow']

    def apply_ema(self):
        """`sess.run(model.ema_apply)`: shadow -= (shadow - theta) * (1 - decay) on the device (alq_ema_step), decay =
        MT_ema_decay_schedule(global_step) evaluated on the host; the teacher is repacked from the shadow vector."""
        if self._mt is None or self._opt is None:
            raise RuntimeError('ema_apply needs MT_SSL and get_optimizer()')
        mt = self._mt
        shadow = self._mt_shadow()
        theta = self._student_theta()
        self.sess.bind_stream()
        check(self.lib.alq_ema_step(self.sess.ctx, ptr(shadow), ptr(theta), self.num_params, float(mt['decay'](self.global_step))))
        self.teacher.set_weights_device(shadow)
        mt['tver'] = self.teacher._weights_version

    def perturb_device(self, t, n, seed, first_sample=0):
        """`model.perturbed_x` of n device patches (alq_perturb_input): Gaussian noise, then the rotation."""
        mt = self._mt
        out = self.sess.empty((n, self.elems_per_patch), self.sess.torch.float32)
        H, W, Cc = (self.in_shape if len(self.in_shape) == 3 else (self.in_shape[0] * self.in_shape[1],) + self.in_shape[2:])
        self.sess.bind_stream()
        check(self.lib.alq_perturb_input(self.sess.ctx, ptr(t), ptr(out), n, H, W, Cc, mt['std'], int(seed), int(first_sample),
                                         int(mt['angle'] is not None), float(mt['angle'] or 0.)))
        return out

    def _mt_pass(self, t, n, y, keep_prob, seed, input_weights, want_grad, feed):
        """_objective_pass of a mean-teacher model: loss = L + cons_coeff * cons read as the vector [n], so
        the gradient is n grad L + cons_coeff sum_i grad cons_i.  Per cut of max_batch: perturb the cut, the teacher's forward
        pass at its own keep_prob, alq_param_grads_loss_mt.  `feed`: dict(kp = the teacher's keep_prob, px = a fed
        perturbed_x or None).  The labelled scale is n / (non-zero weights of the whole batch), the consistency scale
        cons_coeff 2 / (c V) per voxel (L2; CE adds to the value only).  An AU_4U model takes the _au entry points: the
        consistency value of a voxel is div exp(-a) + AU_log_rel_coeff a / 2 and its log-variance column has the scale
        cons_coeff / V under both measures.  Returns (gradient or None, loss) and leaves (L, mean_i cons_i, cons_coeff) in
        self._mt['last']."""
        from . import losses, mteach
        torch = self.sess.torch
        self.sess.bind_stream()
        mt, T = self._mt, self.teacher
        obj = self._obj or dict(q=0.7, gamma=None, class_w=None)          # (no hypers: the plain voxel-wise cross-entropy)
        c, V = self.nclass, self.out_voxels
        ns = n * V
        t = t.reshape(n, -1)
        lab, labd, counts, _, sw, swd, cw, gamma = self._label_feed(y, ns, input_weights, obj, losses.CE)
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        tkp, tarr, tnl, tseed = T._drop_args(feed.get('kp', 1.), None)            # the second draw of the seed stream
        px = feed.get('px')
        nseed = int(np.random.randint(0, 2 ** 31 - 1)) if (px is None and mt['std'] > 0) else 0      # ... and the third
        if px is not None:
            px, npx = self._as_device_batch(px)
            if npx != n:
                raise ValueError('perturbed_x holds %d patches, x %d' % (npx, n))
            px = px.reshape(n, -1)
        self._mt_shadow()
        coeff = mteach.cons_coeff(self.global_step, mt['rampup'], mt['max_coeff'])
        kscale = coeff * 2. / (c * V) if mt['measure'] == mteach.L2 else 0.
        au_on, kappa = self.AU_4U, self.AU_log_rel_coeff
        cuts = list(self._cuts(n))
        spec = lambda a: LossT(losses.CE, -1. if gamma is None else gamma, obj['q'], 1., cw.data_ptr() if cw is not None else None,
                               swd.data_ptr() + a * V * 4 if swd is not None else None, None, None)

        def teacher_post(a, b):
            pin = px[a:b] if px is not None else (self.perturb_device(t[a:b], b - a, nseed, a) if (mt['std'] > 0 or mt['angle'] is not None)
                                                  else t[a:b])
            tq = self.sess.empty((c, (b - a) * V), torch.float32)
            check(self.lib.alq_forward_dropout(T._m, self._patch_ptr(pin, 0), b - a, tkp, tseed, a, tarr, tnl, ptr(tq), None))
            return tq

        def student_post(a, b, want_au=False):
            pb = self.sess.empty((c, (b - a) * V), torch.float32)
            if want_au:
                au = self.sess.empty(((b - a) * V,), torch.float32)
                check(self.lib.alq_forward_au(self._m, self._patch_ptr(t, a), b - a, kp, seed, a, arr, nl, ptr(pb), None, ptr(au), None))
                return pb, au
            check(self.lib.alq_forward_dropout(self._m, self._patch_ptr(t, a), b - a, kp, seed, a, arr, nl, ptr(pb), None))
            return pb

        stats = torch.zeros((len(cuts), 3), dtype=torch.float64, device=self.sess.device)
        gsum = None
        if want_grad:
            if gamma is None:
                cnt = float(self._nonzero_count(lab, cw, sw, counts))
            else:      # the focal weight can vanish (pt == 1): the count comes from a statistics pass first
                for k, (a, b) in enumerate(cuts):
                    pb, L = student_post(a, b), spec(a)
                    check(self.lib.alq_loss_stats(self.sess.ctx, ptr(pb), c, (b - a) * V, ptr(labd, a * V * 4), C.byref(L), ptr(stats, k * 24)))
                cnt = float(stats[:, 1].sum().item())
            s = n / cnt if cnt else 0.
            gsum = torch.zeros((self.num_params,), dtype=torch.float32, device=self.sess.device)
        for k, (a, b) in enumerate(cuts):
            tq, L = teacher_post(a, b), spec(a)
            labp, statp = ptr(labd, a * V * 4), ptr(stats, k * 24)
            if want_grad:
                g = self.sess.empty((self.num_params,), torch.float32)
                head = (self._m, self._patch_ptr(t, a), b - a, labp, C.byref(L), float(s), ptr(tq), mt['measure'], float(kscale))
                tail = (kp, seed, a, arr, nl, ptr(g), None, statp)
                if au_on:
                    check(self.lib.alq_param_grads_loss_mt_au(*head, float(coeff / V), kappa, *tail))
                else:
                    check(self.lib.alq_param_grads_loss_mt(*head, *tail))
                gsum += g
            elif au_on:
                pb, au = student_post(a, b, True)
                check(self.lib.alq_mt_stats_au(self.sess.ctx, ptr(pb), ptr(tq), ptr(au), c, (b - a) * V, labp, C.byref(L), kappa,
                                               mt['measure'], statp))
            else:
                pb = student_post(a, b)
                check(self.lib.alq_mt_stats(self.sess.ctx, ptr(pb), ptr(tq), c, (b - a) * V, labp, C.byref(L), mt['measure'], statp))
        st = stats.cpu().numpy()
        cnt = st[:, 1].sum()
        labelled = float(st[:, 0].sum() / cnt) if cnt else 0.
        cons = float(st[:, 2].sum() / ns)
        mt['last'] = (labelled, cons, coeff)
        return gsum, labelled + coeff * cons

    def _train_mask(self):
        """1 on the parameters of `train_layers` (all when empty), flat order."""
        if not self.train_layers:
            return None
        mask = np.zeros(self.num_params, dtype=np.float32)
        for name, (off, nw, nb) in zip(self.var_names, self._param_offsets()):
            if name in self.train_layers:
                mask[off:off + nw + nb] = 1.
        return mask

    # -- partial fine-tuning (PFT_bflag / par_placeholders, NN_extended.py:1441-1449) ------------
    def _flat_mask(self, mask):
        """A PFT mask - list [MW, Mb, ...] in variable shapes (grads_vars order) or a flat vector / device tensor [P] - as
        (float32 device tensor [P], layers with a non-zero entry)."""
        torch = self.sess.torch
        if isinstance(mask, torch.Tensor):
            if int(mask.numel()) != self.num_params:
                raise ValueError('mask of %d entries for %d parameters' % (int(mask.numel()), self.num_params))
            md = mask.to(device=self.sess.device, dtype=torch.float32).reshape(-1).contiguous()
        else:
            if isinstance(mask, (list, tuple)):
                if len(mask) != 2 * self.L:
                    raise ValueError('expected %d mask arrays (W, b per layer), got %d' % (2 * self.L, len(mask)))
                for q, (nme, wshape, bshape) in enumerate(self.param_shapes):
                    for a_, shp in ((mask[2 * q], wshape), (mask[2 * q + 1], bshape)):
                        if int(np.size(a_)) != int(np.prod(shp)):
                            raise ValueError('layer %s: mask of %d entries for a variable of shape %s' % (nme, np.size(a_), shp))
                mask = np.concatenate([np.asarray(a_, dtype=np.float32).ravel() for a_ in mask])
            mask = np.asarray(mask, dtype=np.float32).ravel()
            if mask.size != self.num_params:
                raise ValueError('mask of %d entries for %d parameters' % (mask.size, self.num_params))
            md = self.sess.to_device(mask, torch.float32)
        # which layers train: L flags cross to the host, not the mask
        flags = torch.stack([(md[o:o + nw + nb] != 0).any() for o, nw, nb in self._param_offsets()]).cpu().numpy()
        return md, [q for q in range(self.L) if flags[q]]

    def set_PFT_mask(self, mask):
        """Partial fine-tuning: every later train step multiplies the summed gradient by `mask` before the optimiser step (on
        top of `train_layers`).  `mask`: list in variable shapes, flat vector or flat device tensor [P] (pft_mask_device);
        None clears it.  Sets `PFT_bflag`.  The mask multiplies the gradient, as in the reference: under SGD a masked-out
        parameter does not move; under Adam it does not move if the mask held since the optimiser's first step, and otherwise
        goes on moving on the moments it has (they are not reset), as a TF variable would."""
        if mask is None:
            self.PFT_bflag, self._pft_mask, self._pft_layers = False, None, None
            return
        self._pft_mask, self._pft_layers = self._flat_mask(mask)
        self.PFT_bflag = True

    def get_par_placeholders(self):
        """NN_extended.py:1441-1449: one mask placeholder per variable in grads_vars order (W_0, b_0, W_1, ...); masks fed under
        them in `sess.run(model.train_step, feed_dict)` hold for that step."""
        self.par_placeholders = []
        for nme, wshape, bshape in self.param_shapes:
            for part, shp in (('W', wshape), ('b', bshape)):
                self.par_placeholders.append(Handle('par_placeholder_%s_%s' % (nme, part), shp))
        return self.par_placeholders

    def pft_mask_device(self, diagF_flat, k=None, thr=None):
        """The binary mask of partial fine-tuning from a flat float64 device vector (diagonal_fisher_device): k given - 1 on
        the k largest entries, ties at the k-th value to the lower index (alq_topk_mask; keep_k_largest_from_LoV); thr given -
        1 where the entry >= thr (alq_threshold_mask; threshold_LoV).  float32 device tensor of the same length."""
        torch = self.sess.torch
        if (k is None) == (thr is None):
            raise ValueError('give exactly one of k and thr')
        v = diagF_flat
        check_tensor(v, torch.float64, device=self.sess.device)
        self.sess.bind_stream()
        n = int(v.numel())
        mask = self.sess.empty((n,), torch.float32)
        if k is not None:
            work = self.sess.empty((self.lib.alq_topk_mask_work_bytes(n),), torch.uint8)
            check(self.lib.alq_topk_mask(self.sess.ctx, ptr(v), n, int(k), ptr(mask), ptr(work)))
        else:
            check(self.lib.alq_threshold_mask(self.sess.ctx, ptr(v), n, float(thr), ptr(mask)))
        return mask

    def _onehot(self, labels, n):
        lab = np.asarray(labels).astype(np.int64).reshape(n)
        y = np.zeros((self.nclass, n), dtype=np.float32)
        ok = (lab >= 0) & (lab < self.nclass)
        y[lab[ok], np.nonzero(ok)[0]] = 1.
        return y

    @staticmethod
    def _is_device_labels(y):
        from .datasets.utils import DeviceLabels
        return isinstance(y, DeviceLabels)

    def _device_label_feed(self, dl, ns, want_host):
        """The label feed of a dense objective from a datasets.DeviceLabels: (host labels [ns] - only when per-voxel weights
        need them -, the int32 device labels [ns], the class counts).  No one-hot, no argmax, no upload."""
        torch = self.sess.torch
        if not self.dense:
            raise TypeError('DeviceLabels feed a fully-convolutional model; an fc-head model takes one-hot columns')
        if dl.C != self.nclass or int(dl.labels.numel()) != ns:
            raise ValueError('labels must be [%d, %d] columns, got DeviceLabels of %r' % (self.nclass, ns, dl.shape))
        labd = dl.labels.to(device=self.sess.device, dtype=torch.int32).contiguous().reshape(ns)
        return (labd.cpu().numpy() if want_host else None), labd, dl.counts

    def _label_feed(self, y, ns, input_weights, obj, kind):
        """What an objective pass over ns samples reads beside the patches: (host labels [ns] or None, int32 device labels, class
        counts or None, device soft targets [c, ns] or None, host and device sample weights or None, device class weights or None,
        the focal gamma in effect or None).  y: one-hot columns [c, ns] (soft targets unless `kind` is CE) or a DeviceLabels."""
        from . import losses
        torch = self.sess.torch
        c = self.nclass
        counts = tgd = None
        if self._is_device_labels(y):
            if kind != losses.CE:
                raise TypeError('DeviceLabels are class ids: the objective reads soft targets')
            lab, labd, counts = self._device_label_feed(y, ns, input_weights is not None)
        else:
            y = np.asarray(y)
            if y.shape != (c, ns):
                raise ValueError('labels must be [%d, %d] columns, got %r' % (c, ns, y.shape))
            lab = np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)
            labd = self.sess.to_device(lab, torch.int32)
            tgd = self.sess.to_device(y.astype(np.float32), torch.float32) if kind != losses.CE else None
        sw = None if input_weights is None else np.asarray(input_weights, dtype=np.float32).reshape(ns)
        swd = None if sw is None else self.sess.to_device(sw, torch.float32)
        gamma = obj['gamma'] if (obj['gamma'] is not None and obj['gamma'] > 0) else None
        return lab, labd, counts, tgd, sw, swd, obj['class_w'], gamma

    def _nonzero_count(self, lab, cw, sw, counts):
        """device_host.nonzero_weight_count of a batch under this model's class weights (lab None: from the class counts)."""
        return nonzero_weight_count(self.nclass, self.hypers['bin_class_weights'] if cw is not None else None, lab, sw, counts)

    def _count_from_class_counts(self, counts, cw):
        return self._nonzero_count(None, cw, None, counts)

    def _objective_pass(self, t, n, y, keep_prob, seed, input_weights, lwf, want_grad=True, mt_feed=None):
        """The model's objective (set_hypers; the batch-mean cross-entropy with divisor n when none is set) on n device patches
        over passes of max_batch: (gradient of the loss, float32 device [P] - None without `want_grad` - and the loss).
        y [c, n]: one-hot columns (all zero: unlabelled) or, for CE_softclasses / GCE, the soft targets; input_weights [n];
        lwf = (old logits [c, n], lambda_o, T) adds lambda_o * mean_n l'_n (model_utils.get_LwF).
        The weighted cross-entropy divides by the number of non-zero weights of the WHOLE batch (TF's SUM_BY_NONZERO_WEIGHTS):
        without the focal term that count is known on the host from labels and weights; with it the passes run unscaled and
        the summed gradient is divided by the count on the device (no read in between); focal with LwF - two terms with two
        divisors - takes the count from forward passes + alq_loss_stats first.  One read of the statistics at the end."""
        from . import losses
        if self._mt is not None and getattr(self, 'teacher', None) is not None:      # (before get_optimizer(): the labelled loss alone)
            if lwf is not None:
                raise NotImplementedError('MT_SSL with learning without forgetting')
            return self._mt_pass(t, n, y, keep_prob, seed, input_weights, want_grad, mt_feed or {})
        torch = self.sess.torch
        self.sess.bind_stream()
        # (a dense model: V samples per patch, always the non-zero-weight divisor of get_FCN_loss, NN_extended.py:1285-1335)
        obj = self._obj or dict(kind=losses.CE, divisor='nonzero' if self.dense else 'N', q=0.7, gamma=None, class_w=None)
        kind, c, V = obj['kind'], self.nclass, self.out_voxels
        ns = n * V
        lab, labd, counts, tgd, sw, swd, cw, gamma = self._label_feed(y, ns, input_weights, obj, kind)
        old, lam, T = None, 0., 1.
        if lwf is not None:
            old = self.sess.to_device(np.asarray(lwf[0], dtype=np.float32).reshape(c, ns), torch.float32)
            lam, T = float(lwf[1]), float(lwf[2])
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        cuts = list(self._cuts(n))

        def spec(a, b):
            keep = [None if v is None else v[:, a * V:b * V].contiguous() for v in (tgd, old)]
            L = LossT(kind, -1. if gamma is None else gamma, obj['q'], T, cw.data_ptr() if cw is not None else None,
                      swd.data_ptr() + a * V * 4 if swd is not None else None, keep[0].data_ptr() if keep[0] is not None else None,
                      keep[1].data_ptr() if keep[1] is not None else None)
            return L, keep

        def stats_only(dst):
            for k, (a, b) in enumerate(cuts):
                pb = self.sess.empty((c, (b - a) * V), torch.float32)
                check(self.lib.alq_forward_dropout(self._m, self._patch_ptr(t, a), b - a, kp, seed, a, arr, nl, ptr(pb), None))
                L, keep = spec(a, b)
                check(self.lib.alq_loss_stats(self.sess.ctx, ptr(pb), c, (b - a) * V, ptr(labd, a * V * 4), C.byref(L), ptr(dst, k * 24)))
                del keep

        stats = torch.zeros((len(cuts), 3), dtype=torch.float64, device=self.sess.device)
        post_scale = False
        if kind == losses.CE_SOFT:
            s = 1. / ns
        elif kind == losses.GCE:
            s = 1.           # reduce_mean over the classes leaves a vector over samples: the optimiser differentiates its sum
        elif obj['divisor'] == 'N':
            s = 1. / ns
        elif gamma is None:
            cnt = self._nonzero_count(lab, cw, sw, counts)
            s = 1. / cnt if cnt else 0.
        elif want_grad and lwf is not None:
            stats_only(stats)
            cnt = float(stats[:, 1].sum().item())
            s = 1. / cnt if cnt else 0.
        else:
            s, post_scale = 1., True
        gsum = None
        if want_grad:
            gsum = torch.zeros((self.num_params,), dtype=torch.float32, device=self.sess.device)
            for k, (a, b) in enumerate(cuts):
                g = self.sess.empty((self.num_params,), torch.float32)
                L, keep = spec(a, b)
                check(self.lib.alq_param_grads_loss(self._m, self._patch_ptr(t, a), b - a, ptr(labd, a * V * 4), C.byref(L), float(s),
                                                    lam / ns, kp, seed, a, arr, nl, ptr(g), None, ptr(stats, k * 24)))
                gsum += g
                del keep
            if post_scale:
                cnt_d = stats[:, 1].sum()
                gsum *= torch.where(cnt_d > 0, 1. / cnt_d.clamp(min=1.), torch.zeros_like(cnt_d)).to(torch.float32)
        else:
            stats_only(stats)
        st = stats.cpu().numpy()
        if kind == losses.CE and obj['divisor'] == 'N':
            loss = 0.
            for (a, b), row in zip(cuts, st):          # the arithmetic of the default step: per-pass means, weighted
                loss += float(row[0] / ((b - a) * V)) * ((b - a) * V) / ns
        elif kind == losses.CE:
            cnt = st[:, 1].sum()
            loss = float(st[:, 0].sum() / cnt) if cnt else 0.
        else:
            loss = float(st[:, 0].sum() / ns)      # GCE: the mean of the reference's per-sample loss vector
        if lwf is not None:
            loss = loss + lam * float(st[:, 2].sum() / ns)
        return gsum, loss

    def lwf_loss(self, x, y_onehot, lwf, keep_prob=1., seed=None, input_weights=None):
        """`sess.run(model.LwF_loss, ...)`: the value LwF_train_step minimises, loss + lambda_o * mean_n l'_n, without a step
        (forward passes + alq_loss_stats).  lwf = (old logits [c, n], lambda_o, T)."""
        self._check_input_weights(input_weights)
        t, n = self._as_device_batch(x)
        return self._objective_pass(t, n, y_onehot, keep_prob, seed, input_weights, lwf, want_grad=False)[1]

    def train_on_batch(self, x, y_onehot, keep_prob=1., seed=None, pft_mask=None, input_weights=None, lwf=None, mt_feed=None):
        """One `sess.run(model.train_step, {x, y_, keep_prob})`: gradient of the batch-mean cross-entropy (summed over
        device passes of max_batch patches), one optimiser step on the device, weights repacked.  y_onehot: [c, n]
        like the reference's hot_labels (PW_AL.py:1064-1067); an all-zero column is an unlabelled sample.
        A PFT mask (set_PFT_mask, or `pft_mask` for this step only) multiplies the summed gradient before the step.
        With hypers (set_hypers) or `lwf` = (old logits [c, n], lambda_o, T) the gradient and the loss are those of the model's
        objective (_objective_pass; alq_param_grads_loss); per-sample `input_weights` [n] need hypers (ValueError without).
        Returns the batch-mean loss before the step."""
        if self._opt is None:
            raise RuntimeError('get_optimizer() has not been called (NN.py:1354)')
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        if self._is_device_labels(y_onehot):          # (a dense model's labels from datasets: checked where they are read)
            if not self.dense:
                raise TypeError('DeviceLabels feed a fully-convolutional model; an fc-head model takes one-hot columns')
            y = y_onehot
        else:
            y = np.asarray(y_onehot)
            if y.shape != (self.nclass, n * self.out_voxels):
                raise ValueError('labels must be [%d, %d] one-hot columns, got %r' % (self.nclass, n * self.out_voxels, y.shape))
        self._check_input_weights(input_weights)
        if self._obj is not None or lwf is not None or self.dense:
            gsum, loss = self._objective_pass(t, n, y, keep_prob, seed, input_weights, lwf, mt_feed=mt_feed)
        else:
            lab = np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)
            kp, _, _, seed = self._drop_args(keep_prob, seed)
            labd = self.sess.to_device(lab, torch.int32)
            gsum = torch.zeros((self.num_params,), dtype=torch.float32, device=self.sess.device)
            loss = 0.
            for a, b in self._cuts(n):
                g, _, l = self.param_grads_device(t[a:b], b - a, 1, labels=labd[a:b], loss_scale=1. / n, keep_prob=kp,
                                                  seed=seed, first_sample=a, per_sample=False, want_loss=True)
                gsum += g
                loss += float(l.item()) * (b - a) / n
        self._optimizer_step(gsum, pft_mask)
        return loss

    def _optimizer_step(self, gsum, pft_mask=None):
        """The second half of a train step: `gsum` (float32 device [P], masked in place by `train_layers` and the PFT mask) through
        one SGD / Adam / RMSProp step on the optimiser's flat device vector; the layers that can have moved are repacked from it."""
        torch = self.sess.torch
        o = self._opt
        fresh = o['theta'] is None
        if fresh or o.get('version') != self._weights_version:
            # the TF variables are the single state of the reference: weights loaded or assigned since the last step
            # (set_weights / load_weights / perform_assign_ops) are what the next step updates; Adam's slots persist
            o['theta'] = self.sess.to_device(self.flat_params(), torch.float32)
        if fresh:
            o['m'] = torch.zeros_like(o['theta'])
            o['v'] = torch.zeros_like(o['theta'])
            if o['name'] == 'RMSProp':                  # TF 1.x: the rms slot starts at ones, the momentum slot at zeros
                o['ms'] = torch.ones_like(o['theta'])
                o['mom'] = torch.zeros_like(o['theta'])
            tm = self._train_mask()
            o['mask'] = self.sess.to_device(tm, torch.float32) if tm is not None else None
        if o.get('mask') is not None:
            gsum *= o['mask']
        pmask, players = (self._pft_mask, self._pft_layers) if pft_mask is None else self._flat_mask(pft_mask)
        if pmask is not None:
            gsum *= pmask
            # The mask multiplies the gradient only (NN_extended.py:1441-1449): Adam's moments persist, so a layer whose mask is all
            # zero still moves unless its m and v are all zero BEFORE this step (then m stays 0 and the step is 0 / eps = 0) - the
            # case when the mask held since the optimiser's first step; likewise RMSProp's momentum slot (momentum 0: mom = lr * 0 /
            # sqrt(.) = 0, the layer stays).  L flags cross to the host.
            slots = {'Adam': ('m', 'v'), 'RMSProp': ('mom',) if o['momentum'] != 0. else ()}.get(o['name'], ())
            if slots and len(players) < self.L:
                still = torch.stack([torch.stack([(o[s][a_:a_ + nw + nb] == 0).all() for s in slots]).all()
                                     for a_, nw, nb in self._param_offsets()]).cpu().numpy()
                players = [q for q in range(self.L) if q in players or not still[q]]
        if o.get('schedule') is not None:
            o['lr'] = float(o['schedule'](o['t']))          # the step count before this step: 0 at the first
        o['t'] += 1
        P = self.num_params
        self.sess.bind_stream()
        if o['name'] == 'SGD':
            check(self.lib.alq_sgd_step(self.sess.ctx, ptr(o['theta']), ptr(gsum), P, o['lr']))
        elif o['name'] == 'RMSProp':
            check(self.lib.alq_rmsprop_step(self.sess.ctx, ptr(o['theta']), ptr(gsum), ptr(o['ms']), ptr(o['mom']), P, o['lr'],
                                            o['decay'], o['momentum'], o['epsilon']))
        else:
            # a parameter masked out since the first step keeps m = v = 0: its step is 0 / eps = 0
            check(self.lib.alq_adam_step(self.sess.ctx, ptr(o['theta']), ptr(gsum), ptr(o['m']), ptr(o['v']), P, o['lr'],
                                         o.get('beta1', 0.9), o.get('beta2', 0.999), 1e-8, o['t']))
        if self._host_repack:
            self.set_flat_params(o['theta'].cpu().numpy())
        else:
            # the model is fed from the device vector; a layer outside `train_layers` kept its weights (masked gradient: SGD
            # subtracts 0, Adam's m = v = 0 step is 0 / eps = 0) and its packed forms.  A layer whose PFT mask is all zero is
            # left out only where this step provably did not move it: SGD, or Adam with that layer's moments all zero (`players`)
            only = [t for t, nme in enumerate(self.var_names) if nme in self.train_layers] if self.train_layers else None
            if pmask is not None:
                only = [t for t in (range(self.L) if only is None else only) if t in players]
            self.set_weights_device(o['theta'], only=only)
        o['version'] = self._weights_version
        if self._mt is not None:
            from . import mteach
            self.cons_coeff = mteach.cons_coeff(o['t'], self._mt['rampup'], self._mt['max_coeff'])
