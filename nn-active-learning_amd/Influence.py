"""Influence functions on the device (reference: Influence.py).

The reference builds the Hessian-vector product as a TF sub-graph (`hessian_vector_product`, Influence.py:64-123: the
Pearlmutter double-backward) and hands evaluators of `1/2 t'Ht - g't`, its gradient and `H t` to scipy's Newton-CG
(`PW_sample_influence`, Influence.py:369-453).  Here the product is one device call (alq_hess_vecp, csrc/hvp.hip); the
names, arguments and the flat-vector conventions are the reference's.

Two things differ on purpose:
  * `get_f_evaluator`'s inner function is named for what it returns (the objective; the reference calls it `eval_fprime`);
  * the evaluators and `PW_sample_influence` take `whole_set=False`.  False is the reference's literal behaviour: its
    `batch_eval(..., 'hess_vecp')` overwrites the result in every batch (PW_NN.py:532-533), so H is the Hessian of the LAST
    batch of `tr_inds`.  True is what the method means: the Hessian of the mean loss over all of `tr_inds`, accumulated over
    the batches on the device.
The reference's `pdb.set_trace()` in front of the solve (Influence.py:444) is dropped.
"""
import numpy as np

from . import NN, PW_NN, patch_utils
from .device import Handle, MethodHandle


def hessian_vector_product(model, x, labels, v, layers='all', loss_scale=None):
    """Influence.hessian_vector_product (Influence.py:64-123) as one device call: the product of the Hessian of the
    mean cross-entropy of the labelled batch (`loss_scale` None; else of loss_scale * the summed loss) with respect to
    the variables of `layers` with `v` (a list [VW, Vb, ...] in their shapes, or a flat vector); list of float64 arrays."""
    return model.hess_vecp(x, labels, v, layers=layers, loss_scale=loss_scale)


def get_hess_vec_product(model, layers):
    """Influence.get_hess_vec_product (Influence.py:126-166): sets `model.Hess_layers`, the vector placeholders
    `model.v_placeholder` (W and b per layer, with the variables' shapes) and the fetch `model.hess_vecp`."""
    if isinstance(layers, str) and layers == 'all':
        layers = list(model.var_dict.keys())
    model.Hess_layers = list(layers)
    shapes = {name: (wshape, bshape) for name, wshape, bshape in model.param_shapes}
    v_placeholder = []
    for layer in model.Hess_layers:
        wshape, bshape = shapes[layer]
        v_placeholder += [Handle('v_%s_W' % layer, wshape), Handle('v_%s_b' % layer, bshape)]
    model.v_placeholder = v_placeholder
    model.hess_vecp = MethodHandle('hess_vecp')      # still callable as DeviceModel.hess_vecp
    model.hess_vecp.model = model


def eval_loss_grad_q(model, sess, padded_imgs, mask, test_ind, patch_shape, batch_size, stats):
    """Gradient of the loss with respect to one test sample (Influence.py:168-201)."""
    q_patch, q_label = patch_utils.get_patches(padded_imgs, [test_ind], patch_shape, True, mask)
    m = q_patch.shape[-1]
    for j in range(m):
        q_patch[:, :, :, j] = (q_patch[:, :, :, j] - stats[j][0]) / stats[j][1]
    q_hot_label = np.zeros((2, 1))
    q_hot_label[0, q_label[0] == 0] = 1
    q_hot_label[1, q_label[0] == 1] = 1
    return sess.run(model.loss_grad, feed_dict={model.x: q_patch, model.y_: q_hot_label, model.keep_prob: 1.})


def _hessp(model, sess, padded_imgs, mask, tr_inds, patch_shape, batch_size, stats, vec, whole_set):
    tensors_list = unravel_vec(model, vec)
    x_feed_dict = {}
    for i in range(len(tensors_list)):
        x_feed_dict.update({model.v_placeholder[i]: tensors_list[i]})
    kw = {'_whole_set': True} if whole_set else {}
    return PW_NN.batch_eval(model, sess, padded_imgs, tr_inds, patch_shape, batch_size, stats, 'hess_vecp', mask, x_feed_dict,
                            **kw)[0]


def get_f_evaluator(model, sess, padded_imgs, mask, tr_inds, Lq_grad, patch_shape, batch_size, stats, whole_set=False):
    """Evaluator of the Hessian-product objective `1/2 t^T H t - v^T t` (Influence.py:204-241)."""

    def eval_f(t):
        hessp = _hessp(model, sess, padded_imgs, mask, tr_inds, patch_shape, batch_size, stats, t, whole_set)
        return 0.5 * np.dot(t, ravel_tensors(hessp)) - np.dot(ravel_tensors(Lq_grad), t)

    return eval_f


def get_fprime_evaluator(model, sess, padded_imgs, mask, tr_inds, Lq_grad, patch_shape, batch_size, stats, whole_set=False):
    """Evaluator of the objective's gradient `H t - v` (Influence.py:244-281)."""

    def eval_fprime(t):
        hessp = _hessp(model, sess, padded_imgs, mask, tr_inds, patch_shape, batch_size, stats, t, whole_set)
        return ravel_tensors(hessp) - ravel_tensors(Lq_grad)

    return eval_fprime


def get_hessp_evaluator(model, sess, padded_imgs, mask, tr_inds, patch_shape, batch_size, stats, whole_set=False):
    """Evaluator of the Hessian-vector product `H vec` (Influence.py:283-317); `t`, the point, is not used: the objective
    is quadratic."""

    def eval_hessp(t, vec):
        return ravel_tensors(_hessp(model, sess, padded_imgs, mask, tr_inds, patch_shape, batch_size, stats, vec, whole_set))

    return eval_hessp


def ravel_tensors(tensors_list):
    """Flattens a list of arrays into one vector (Influence.py:320-329)."""
    return np.concatenate([np.ravel(tensor) for tensor in tensors_list])


def unravel_vec(model, vec):
    """Cuts a flat vector into the variable shapes of `model.Hess_layers`, W then b per layer (Influence.py:331-366)."""
    tensor_list = []
    cnt = 0
    for layer in model.Hess_layers:
        for k in (0, 1):
            var_shape = model.var_dict[layer][k].shape
            var_shape = [int(getattr(d, 'value', d)) for d in var_shape]
            size = int(np.prod(var_shape))
            tensor_list += [np.reshape(vec[cnt:cnt + size], var_shape)]
            cnt += size
    return tensor_list


def PW_sample_influence(model, sess, tr_padded_imgs, tr_mask, tr_inds, tr_stats, q_padded_imgs, q_mask, q_ind, q_stats,
                        patch_shape, batch_size, layers='all', whole_set=False):
    """Influence.PW_sample_influence (Influence.py:369-453): Newton-CG solve of `H t = grad L(query sample)`, H the Hessian
    of the training loss over the voxels `tr_inds` - of their LAST batch of `batch_size` like the reference (see the module
    docstring), of all of them with `whole_set=True`.  Returns scipy's solution vector over `model.Hess_layers`."""
    from scipy.optimize import fmin_ncg
    if getattr(model, '_obj', None) is not None:      # before anything is evaluated: H exists for NN.py's loss only
        model._require_default_objective('PW_sample_influence')
    if not hasattr(model, 'v_placeholder'):      # (the reference tests for `hess_vecp`, which is also a method here)
        model.Hess_layers = layers
        get_hess_vec_product(model, layers)
    if not hasattr(model, 'loss_grad'):
        pars = [] if (isinstance(layers, str) and layers == 'all') else list(layers)
        NN.add_loss_grad(model, pars)
    Lq_grad = eval_loss_grad_q(model, sess, q_padded_imgs, q_mask, q_ind, patch_shape, batch_size, q_stats)
    f = get_f_evaluator(model, sess, tr_padded_imgs, tr_mask, tr_inds, Lq_grad, patch_shape, batch_size, tr_stats, whole_set)
    fprime = get_fprime_evaluator(model, sess, tr_padded_imgs, tr_mask, tr_inds, Lq_grad, patch_shape, batch_size, tr_stats,
                                  whole_set)
    hessp = get_hessp_evaluator(model, sess, tr_padded_imgs, tr_mask, tr_inds, patch_shape, batch_size, tr_stats, whole_set)
    soln = fmin_ncg(f=f, x0=ravel_tensors(Lq_grad), fprime=fprime, fhess_p=hessp, avextol=1e-8, maxiter=10)
    return soln
