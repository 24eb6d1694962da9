"""`sess.run(fetch, feed_dict)` of the reference over a device model: one dispatcher for fc-head and fully-convolutional
models.  DeviceSession.run delegates here."""
import numpy as np

from .device_host import onehot_to_labels


def _pft_masks(model, feed_dict):
    """The masks fed under model.par_placeholders, which hold for this step (NN_extended.py:1441-1449); None when none is fed."""
    ph = getattr(model, 'par_placeholders', None)
    fed = [h in feed_dict for h in ph] if ph else []
    if any(fed) and not all(fed):
        raise KeyError('a PFT step needs a mask for every entry of par_placeholders')
    return [feed_dict[h] for h in ph] if any(fed) else None


def _lwf_feed(model, feed_dict):
    """(old logits, lambda_o, T) of model_utils.get_LwF."""
    return feed_dict[model.y__], float(feed_dict[model.lambda_o]), float(feed_dict[model.T])


def run(fetch, feed_dict=None):
    """`sess.run(fetch, feed_dict={model.x: batch, model.keep_prob: p, model.y_: labels})` for the fetches the
    reference's query / fine-tune code uses: `model.posteriors`, `.prediction`, `.feature_layer` (PW_NN.py:522),
    `model.grad_posts[str(j)]` (PW_NNAL.py:773-807: list of 2L' gradient arrays of log posteriors[j, 0]) and
    `model.train_step` (PW_AL.py:1075-1080, :1140-1146); of the influence functions (Influence.py): `model.loss` (scalar
    mean cross-entropy, needs `model.y_`), `model.loss_grad` (NN.add_loss_grad) and `model.hess_vecp` with the entries of
    `model.v_placeholder` in the feed (Influence.get_hess_vec_product).  Per-sample loss weights fed under
    `model.input_weights` (or an `input_vox_weights` attribute of the model; the reference tests for one name and reads the
    other, NN_extended.py:1252-1255) multiply the weights of the cross-entropy; `model.LwF_train_step` (model_utils.get_LwF)
    takes `model.y__`, `model.lambda_o` and `model.T` as well; `model.labels` / `model.pt` are the label vector and the
    posterior of each sample's label as the two-class focal term reads them (NN_extended.py:1228-1231)."""
    model = getattr(fetch, 'model', None)
    if isinstance(fetch, list):
        model = getattr(fetch[0], 'model', None) if fetch else None
        if model is None:
            raise KeyError('unknown fetch list')
        x = feed_dict[model.x]
        kp = float(feed_dict.get(model.keep_prob, 1.))
        j = fetch[0].cls
        return model.grad_log_post(x, j, keep_prob=kp)
    if model is None:
        raise KeyError('unknown fetch %r' % (fetch,))
    if fetch.name == 'ema_apply':          # (NN_extended.py:1006-1008: run without a feed)
        return model.apply_ema()
    x = feed_dict[model.x]
    kp = float(feed_dict.get(model.keep_prob, 1.))
    iw = None
    for h in (getattr(model, 'input_weights', None), getattr(model, 'input_vox_weights', None)):
        if h is not None and h in feed_dict:
            iw = feed_dict[h]
    if getattr(model, 'dense', False):
        return _run_dense(model, fetch, feed_dict, x, kp, iw)
    if fetch.name == 'LwF_train_step':
        return model.train_on_batch(x, feed_dict[model.y_], keep_prob=kp, input_weights=iw, lwf=_lwf_feed(model, feed_dict))
    if fetch.name == 'LwF_loss':
        return model.lwf_loss(x, feed_dict[model.y_], _lwf_feed(model, feed_dict), keep_prob=kp, input_weights=iw)
    if fetch.name in ('labels', 'pt'):
        lab = onehot_to_labels(feed_dict[model.y_], model.nclass)
        if fetch.name == 'labels':
            return lab
        post = model.forward(x, want=('posteriors',), keep_prob=kp)['posteriors']
        return np.where(lab == 1, post[1], post[0])
    if fetch.name == 'train_step':
        masks = _pft_masks(model, feed_dict)
        return model.train_on_batch(x, feed_dict[model.y_], keep_prob=kp, pft_mask=masks, input_weights=iw)
    if fetch.name in ('loss', 'loss_grad', 'hess_vecp'):
        # the training-time graph nodes of the influence functions (NN.py:583-588, :862-871; Influence.py:126-166)
        if kp != 1.:
            raise NotImplementedError('%s at keep_prob < 1' % fetch.name)
        model._check_input_weights(iw)
        if model._obj is not None:
            # an NN_extended objective: soft targets are read as they are fed
            if fetch.name == 'hess_vecp':
                model._require_default_objective('hess_vecp')
            if fetch.name == 'loss':
                return model.mean_loss(x, None, targets=feed_dict[model.y_], input_weights=iw)
            return model.mean_loss_grad(x, None, fetch.layers, targets=feed_dict[model.y_], input_weights=iw)
        lab = onehot_to_labels(feed_dict[model.y_], model.nclass)
        if fetch.name == 'loss':
            return model.mean_loss(x, lab)
        if fetch.name == 'loss_grad':
            return model.mean_loss_grad(x, lab, fetch.layers)
        from .device_model import DeviceModel
        v = [feed_dict[h] for h in model.v_placeholder]
        return DeviceModel.hess_vecp(model, x, lab, v, layers=model.Hess_layers)
    res = model.forward(x, want=(fetch.name,), keep_prob=kp)
    return res[fetch.name]


def _run_dense(model, fetch, feed_dict, x, kp, iw):
    """sess.run of a dense model: `posteriors` [n, *spatial, c], `prediction` [n, *spatial], `feature_layer`, `loss` and
    `train_step` with `y_` one-hot [n, *spatial, c] (an all-zero row: unlabelled voxel, NN_extended.py:1291-1293) and
    `input_vox_weights` [n, *spatial].  A datasets.DeviceLabels under `y_` (labels [n, *spatial] built on the device) is read in
    place: no one-hot, no argmax, no upload; the non-zero-weight count comes from its class counts."""
    name = fetch.name
    if name in ('posteriors', 'prediction'):
        t, n = model._as_device_batch(x)
        maps, pred = model.forward_maps_device(t, n, kp, want_pred=name == 'prediction')
        return (pred if name == 'prediction' else maps.contiguous()).cpu().numpy()
    if name == 'feature_layer':
        return model.forward(x, want=(name,), keep_prob=kp)[name]
    if name in ('AU_vals', 'output') and model.AU_4U:
        t, n = model._as_device_batch(x)
        au, out = model.forward_au_device(t, n, kp, want_output=name == 'output')
        return (au if name == 'AU_vals' else out).cpu().numpy()
    mt_on = model._mt is not None and getattr(model, 'teacher', None) is not None
    if name not in ('loss', 'train_step') + (('labeled_loss', 'cons_loss') if mt_on else ()):
        raise NotImplementedError('sess.run(model.%s) is not defined for a fully-convolutional model (1x1 conv head)' % name)
    y = feed_dict[model.y_]
    on_device = model._is_device_labels(y)          # datasets.DeviceLabels: the labels stay where they are
    y = y if on_device else np.asarray(y)
    n = int(np.asarray(x).shape[0]) if not isinstance(x, model.sess.torch.Tensor) else int(x.shape[0])
    if tuple(y.shape) != (n,) + model.out_map_shape + (model.nclass,):
        raise ValueError('y_ must be one-hot %r, got %r' % ((n,) + model.out_map_shape + (model.nclass,), tuple(y.shape)))
    ycols = y if on_device else np.ascontiguousarray(y.reshape(-1, model.nclass).T)
    if iw is not None:
        iw = np.asarray(iw)
        if tuple(iw.shape) != (n,) + model.out_map_shape:
            raise ValueError('input_vox_weights must be %r, got %r' % ((n,) + model.out_map_shape, tuple(iw.shape)))
        iw = iw.reshape(-1)
    mt_feed = dict(kp=float(feed_dict.get(model.teacher.keep_prob, 1.)), px=feed_dict.get(model.perturbed_x)) if mt_on else None
    if name in ('loss', 'labeled_loss', 'cons_loss'):
        t, n = model._as_device_batch(x)
        loss = model._objective_pass(t, n, ycols, kp, None, iw, None, want_grad=False, mt_feed=mt_feed)[1]
        return loss if name == 'loss' else model._mt['last'][name == 'cons_loss']
    masks = _pft_masks(model, feed_dict)
    return model.train_on_batch(x, ycols, keep_prob=kp, pft_mask=masks, input_weights=iw, mt_feed=mt_feed)
