"""`NN_extended.CNN`-schema models on the device (reference: NN_extended.py:20-295): layer dict
``{name: [type, specs, op_order]}`` with conv / conv_transpose / pool / fc in 2-D or 3-D, 'con'
skip connections, fc head (the form `get_gradients` is defined for, NN_extended.py:1025) or the 1x1
conv head of the reference's FCN branch (NN_extended.py:262-294: posteriors [N, *spatial, c], the
voxel-wise objective of get_FCN_loss, :1285-1335, with `input_vox_weights`), and the
training hyper-parameters of `set_hypers` (NN_extended.py:24-63) that the device step knows:
losses CE / CE_softclasses / GCE with class, focal and per-sample weights, optimisers SGD / Adam /
RMSProp, learning-rate schedules."""
import numpy as np

from .device import DeviceModel, default_session


# ---- schedules (NN_extended.py:1462-1527), NumPy: evaluated on the host once per step ------------
def sigmoid_rampup(global_step, rampup_length):
    global_step, rampup_length = float(global_step), float(rampup_length)
    if global_step < rampup_length:
        phase = 1.0 - max(0.0, global_step) / rampup_length
        return float(np.exp(-5.0 * phase * phase))
    return 1.0


def sigmoid_rampdown(global_step, rampdown_length, training_length):
    global_step, rampdown_length, training_length = float(global_step), float(rampdown_length), float(training_length)
    if global_step >= training_length - rampdown_length:
        phase = 1.0 - max(0.0, training_length - global_step) / rampdown_length
        return float(np.exp(-12.5 * phase * phase))
    return 1.0


def sigmoid_schedule(global_step, max_lr, rampup_length, rampdown_length, train_length):
    return sigmoid_rampup(global_step, rampup_length) * sigmoid_rampdown(global_step, rampdown_length, train_length) * float(max_lr)


def exponential_decay(init_lr, global_step, decay_rate):
    return float(init_lr) * float(np.exp(-float(global_step) * float(decay_rate)))


class CNN(DeviceModel):
    """NN_extended.CNN(x, layer_dict, name, skips, feature_layer, dropout, probes, **kwargs) with
    `x` replaced by the placeholder SHAPE ((H,W,C) or (D,H,W,C)).  A model built without keywords
    trains as an `NN.CNN` does (batch-mean cross-entropy, `get_optimizer(lr, layers, name)`); any
    of the training keywords below makes it the reference's `get_loss` objective, whose weighted
    cross-entropy divides by the number of non-zero weights."""

    # the entries of the reference's DEFAULT_HYPERS that a device step reads
    DEFAULT_HYPERS = {
        'activation': 'ReLU',
        'loss_name': 'CE',
        'optimizer_name': 'SGD',
        'lr_schedule': lambda t: exponential_decay(1e-3, t, 0.1),
        'learning_rate': None,
        'bin_class_weights': None,
        'focal_gamma': None,
        'q': 0.7,
        'beta1': 0.9,
        'beta2': 0.999,
        'decay': 0.9,
        'momentum': 0.,
        'epsilon': 1e-10,
    }

    def __init__(self, in_shape, layer_dict, name, skips=[], feature_layer=None, dropout=None,
                 probes=[[], []], sess=None, max_batch=256, **kwargs):
        for key in kwargs:
            if key == 'activation':
                if kwargs[key] != 'ReLU':
                    raise NotImplementedError('activation %r: the device layers are ReLU' % (kwargs[key],))
            elif key not in self.DEFAULT_HYPERS:
                raise NotImplementedError('hyper-parameter %r (regularisers, batch-norm, aleatoric uncertainty and mean-teacher '
                                          'training are outside the device step)' % key)
        hypers = dict(self.DEFAULT_HYPERS)
        hypers.update(kwargs)
        if hypers['loss_name'] not in ('CE', 'CE_softclasses', 'GCE'):
            raise ValueError('loss_name %r' % (hypers['loss_name'],))
        if hypers['optimizer_name'] not in ('SGD', 'Adam', 'RMSProp'):
            raise ValueError('optimizer_name %r' % (hypers['optimizer_name'],))
        if hypers['loss_name'] == 'GCE' and float(hypers['q']) == 0:
            raise ValueError('q cannot be equal to zero.')
        bcw = hypers['bin_class_weights']
        if bcw is not None and np.size(bcw) != 2:
            raise ValueError('bin_class_weights holds two weights')
        if hypers['lr_schedule'] is not None and not callable(hypers['lr_schedule']):
            raise ValueError('lr_schedule is a callable of the step count')
        training = [k for k in kwargs if k != 'activation']
        last = list(layer_dict.values())[-1]
        nclass = int(last[1][0]) if isinstance(last[0], str) else int(last[0])          # either layer-dict schema
        if isinstance(last[0], str) and last[0] == 'conv' and hypers['loss_name'] != 'CE':
            # a fully-convolutional model trains on get_FCN_loss (NN_extended.py:1285-1335), the only FCN loss the reference defines
            raise ValueError('loss_name %r on a fully-convolutional model: its objective is the voxel-wise cross-entropy (CE)'
                             % (hypers['loss_name'],))
        if (bcw is not None or hypers['focal_gamma'] is not None) and nclass != 2:
            raise ValueError('bin_class_weights / focal_gamma need a two-class net (where(labels == 1, .[1], .[0])), got %d classes'
                             % nclass)
        super(CNN, self).__init__(sess or default_session(), layer_dict, in_shape, skips, feature_layer,
                                  dropout, max_batch, name)
        if training or self.dense:      # (a dense model always trains on get_FCN_loss: non-zero-weight divisor, voxel weights)
            self.set_hypers(hypers)
