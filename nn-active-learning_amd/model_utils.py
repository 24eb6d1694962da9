"""The functions of the reference's model_utils.py behind partial fine-tuning: the diagonal Fisher (which reuses the scoring
kernels) and the binary masks made from it."""
import numpy as np

from .NN import LLFC_grads, LLFC_hess, PW_LLFC_grads  # noqa: F401  (the reference keeps a copy of each, model_utils.py:137-292)


def diagonal_Fisher(model, sess, batch_dat):
    """model_utils.diagonal_Fisher (model_utils.py:294-330): per parameter, the mean over the samples of the squared
    gradient of the sample's loss (= the squared gradient of log posteriors[label]); `batch_dat` = (x [N, ...],
    one-hot labels [c, N]).  Returns the arrays in variable order and TF shapes, like the reference's list.
    The reference runs one sess.run per sample; here a device pass squares and sums its samples' gradients without writing
    them out (alq_diag_fisher).  Masks the model may hold (set_PFT_mask) play no part: the reference feeds ones here
    (model_utils.py:308-315)."""
    x, y = batch_dat
    y = np.asarray(y)
    labels = np.where(y.sum(0) > 0, y.argmax(0), -1)
    if (labels < 0).any():
        raise ValueError('every sample needs a label (one-hot column)')
    return model.diagonal_fisher(np.asarray(x), labels)


def extend_weights_to_aleatoric_mode(weights_path, out_channels, last_layer_name='last'):
    """model_utils.extend_weights_to_aleatoric_mode (model_utils.py:14-48): a copy of the weight file whose last layer has
    `out_channels` output channels, the new ones zero, every other layer as it was; written next to the file as
    '<name>_extended' + its suffix (.npz, or .h5 with h5py) and its path returned.  A last layer that already has that many:
    nothing is written, None.  The reference always doubles the channels (the AU_4L layout) and reads `out_channels` only
    for that check; for out_channels = 2 c the files agree.  The added log-variance channel sits at x == 0, where ReluGrad
    is 0: it trains only once its bias is made positive, in the reference as here."""
    import os
    from . import weights_io
    pars = weights_io.read_weights(weights_path, weights_io.layer_names(weights_path))
    W, b = (np.asarray(v) for v in pars[last_layer_name])
    c = W.shape[-1]
    if c == int(out_channels):
        print('The weights already match the extended shape.')
        return None
    if int(out_channels) < c:
        raise ValueError('the last layer has %d output channels, more than %d' % (c, out_channels))
    ext_W = np.zeros(W.shape[:-1] + (int(out_channels),), dtype=W.dtype)
    ext_W[..., :c] = W
    ext_b = np.zeros((int(out_channels),) + b.shape[1:], dtype=b.dtype)
    ext_b[:c] = b
    pars[last_layer_name] = [ext_W, ext_b]
    root, ext = os.path.splitext(str(weights_path))
    new_path = root + '_extended' + ext
    weights_io.write_weights(new_path, pars)
    return new_path


def keep_k_largest_from_LoV(LoV, k):
    """model_utils.keep_k_largest_from_LoV (model_utils.py:54-83): a binary mask with the structure of the list of
    variables `LoV`, 1 on the k largest values over all of them, and the positions in the list that hold a 1.
    The reference arg-sorts the negated values and leaves the order of equal values open; here entries equal to the
    k-th largest value are taken in flat order (variables in list order, each raveled), the rule of alq_topk_mask.
    Returns (bmask, non_empty_locs)."""
    LoV = [np.asarray(v) for v in LoV]
    Ls = [int(v.size) for v in LoV]
    flat = np.concatenate([v.ravel() for v in LoV]) if LoV else np.zeros(0)
    k = int(k)
    if k < 0 or k > flat.size:
        raise ValueError('k = %d outside [0, %d]' % (k, flat.size))
    sort_inds = np.argsort(-flat, kind='stable')[:k]
    fmask = np.zeros(flat.size)
    fmask[sort_inds] = 1
    ends = np.cumsum(Ls)
    bmask = [fmask[e - n:e].reshape(v.shape) for e, n, v in zip(ends, Ls, LoV)]
    non_empty_locs = np.where(np.array([m.any() for m in bmask], dtype=bool))[0]
    return bmask, non_empty_locs


def threshold_LoV(LoV, thr):
    """model_utils.threshold_LoV (model_utils.py:85-96): 1 where a variable's value is >= thr, 0 elsewhere."""
    bmask = [np.zeros(np.shape(v)) for v in LoV]
    for m, v in zip(bmask, LoV):
        m[np.asarray(v) >= thr] = 1
    return bmask


def get_LwF(model):
    """model_utils.get_LwF (model_utils.py:98-135): learning without forgetting on top of the loss the model has.  Creates the
    handles `lambda_o`, `T`, `y__` (the previous model's logits [c, n]), `LwF_loss` and `LwF_train_step`;
    `sess.run(model.LwF_train_step, {x, y_, y__, lambda_o, T, keep_prob})` takes one optimiser step on
    loss + lambda_o * mean_n CE(softmax(y__ / T), softmax(output / T)), the mean over all n columns, labelled or not
    (alq_param_grads_loss with old logits), and returns that loss.  Needs get_optimizer() beforehand, like the reference.
    Under `train_layers` the reference calls `minimize(model.LwF, ...)`, an AttributeError (the attribute is `LwF_loss`); here
    the step minimises `LwF_loss` over those layers."""
    from .device import Handle
    if getattr(model, '_opt', None) is None:
        raise RuntimeError('get_LwF needs model.get_optimizer() to be called beforehand')
    model.lambda_o = Handle('lambda_o')
    model.T = Handle('T')
    model.y__ = Handle('y__')
    model.LwF_loss = Handle('LwF_loss')              # sess.run(model.LwF_loss, ...): the same value, no step
    model.LwF_train_step = Handle('LwF_train_step')
    model.LwF_loss.model = model.LwF_train_step.model = model
