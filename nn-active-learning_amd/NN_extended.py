"""`NN_extended.CNN`-schema models on the device (reference: NN_extended.py:20-295): layer dict
``{name: [type, specs, op_order]}`` with conv / conv_transpose / pool / fc in 2-D or 3-D, 'con'
skip connections, fc head (the form `get_gradients` is defined for, NN_extended.py:1025) or the 1x1
conv head of the reference's FCN branch (NN_extended.py:262-294: posteriors [N, *spatial, c], the
voxel-wise objective of get_FCN_loss, :1285-1335, with `input_vox_weights`), and the
training hyper-parameters of `set_hypers` (NN_extended.py:24-63) that the device step knows:
losses CE / CE_softclasses / GCE with class, focal and per-sample weights, optimisers SGD / Adam /
RMSProp, learning-rate schedules; mean-teacher consistency training (`MT_SSL`, NN_extended.py:913-926, :1337-1396) of a
fully-convolutional model, with the aleatoric-uncertainty head for unlabelled voxels (`AU_4U`, :265-288, :1376-1383,
:1551-1554), and the training loop `train` (:928-1009)."""
import os

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
    # mean-teacher training (NN_extended.py:56-62); the decay schedule is a callable of the step count (the reference's default
    # takes no argument and is called with one)
    MT_HYPERS = {
        'MT_SSL': False,
        'MT_ema_decay_schedule': lambda t: 0.999,
        'rotation_angle': None,
        'Gaussian_noise_std': None,
        'output_perturbation_measure': 'CE',
        'max_cons_coeff': 1e-3,
        'rampup_length': 5000,
    }
    # aleatoric uncertainty (NN_extended.py:42-45): AU_4U is built; AU_4L reads an undefined model.MC_probs in the reference
    # (:1562-1578) and stays refused
    AU_HYPERS = {'AU_4U': False, 'AU_4L': False, 'AU_log_rel_coeff': 0.1}
    REFUSED_WITH_MT = ('AU_4L', 'regularizer')

    def __init__(self, in_shape, layer_dict, name, skips=[], feature_layer=None, dropout=None,
                 probes=[[], []], sess=None, max_batch=256, **kwargs):
        last = list(layer_dict.values())[-1]
        dense_head = isinstance(last[0], str) and last[0] == 'conv'
        mt = {k: kwargs.pop(k) for k in list(kwargs) if k in self.MT_HYPERS}
        au = dict(self.AU_HYPERS, **{k: kwargs.pop(k) for k in list(kwargs) if k in self.AU_HYPERS})
        if au['AU_4L']:
            raise NotImplementedError('AU_4L: the reference\'s corrupt_output_wAU_4L_FCN reads an undefined model.MC_probs')
        if au['AU_4U']:
            if not dense_head:
                raise NotImplementedError('AU_4U on an fc-head model: the log-variance is a channel of an output map')
            if int(last[1][0]) < 3:
                raise NotImplementedError('AU_4U on a head of %d channels: one is the log-variance, and the device head has 2 .. 7 '
                                          'classes beside it' % int(last[1][0]))
        if mt.get('MT_SSL'):
            for key in self.REFUSED_WITH_MT:
                if kwargs.get(key):
                    raise NotImplementedError('MT_SSL with %s' % key)
            if not dense_head:
                raise NotImplementedError('MT_SSL on an fc-head model: mean-teacher training is defined for fully-convolutional '
                                          'models (the reference reduces over the axes of an output map)')
        for key in kwargs:          # (the mean-teacher keywords of a model without MT_SSL are not read, as in the reference)
            if key == 'activation':
                if kwargs[key] != 'ReLU':
                    raise NotImplementedError('activation %r: the device layers are ReLU' % (kwargs[key],))
            elif key not in self.DEFAULT_HYPERS:
                raise NotImplementedError('hyper-parameter %r (regularisers and batch-norm are outside the device step)' % key)
        hypers = dict(self.DEFAULT_HYPERS)
        hypers.update(kwargs)
        if mt.get('MT_SSL'):
            from . import mteach
            mt = dict(self.MT_HYPERS, **mt)
            if mt['output_perturbation_measure'] not in mteach.MEASURES:
                raise ValueError('output_perturbation_measure %r (L2 or CE)' % (mt['output_perturbation_measure'],))
            if not callable(mt['MT_ema_decay_schedule']):
                raise ValueError('MT_ema_decay_schedule is a callable of the step count')
            if mt['rotation_angle'] is not None and len(in_shape) != 3:
                raise ValueError('rotation_angle on a 3-D model: tf.contrib.image.rotate turns images [N, H, W, C]')
            if mt['Gaussian_noise_std'] is not None and float(mt['Gaussian_noise_std']) < 0:
                raise ValueError('Gaussian_noise_std %r' % (mt['Gaussian_noise_std'],))
            if float(mt['rampup_length']) <= 0:
                raise ValueError('rampup_length %r' % (mt['rampup_length'],))
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
        nclass = int(last[1][0]) if isinstance(last[0], str) else int(last[0])          # either layer-dict schema
        nclass -= 1 if au['AU_4U'] else 0
        if dense_head and hypers['loss_name'] != 'CE':
            # a fully-convolutional model trains on get_FCN_loss (NN_extended.py:1285-1335), the only FCN loss the reference defines
            raise ValueError('loss_name %r on a fully-convolutional model: its objective is the voxel-wise cross-entropy (CE)'
                             % (hypers['loss_name'],))
        if (bcw is not None or hypers['focal_gamma'] is not None) and nclass != 2:
            raise ValueError('bin_class_weights / focal_gamma need a two-class net (where(labels == 1, .[1], .[0])), got %d classes'
                             % nclass)
        super(CNN, self).__init__(sess or default_session(), layer_dict, in_shape, skips, feature_layer,
                                  dropout, max_batch, name, aleatoric=bool(au['AU_4U']), au_log_rel_coeff=float(au['AU_log_rel_coeff']))
        self.AU_4L = False
        if training or self.dense:      # (a dense model always trains on get_FCN_loss: non-zero-weight divisor, voxel weights)
            self.set_hypers(hypers)
        self.MT_SSL = bool(mt.get('MT_SSL'))
        if self.MT_SSL:
            self.set_mean_teacher(mt)

    def train(self, sess, global_step_limit, train_gen, metric_gens=[], eval_step=100, save_path=None):
        """The reference's training loop (NN_extended.py:928-1009).  `metric_gens`: a list of [metric names, data generator,
        iterations (, the metric whose maximum keeps the max_* files)] lists.  Every `eval_step` steps, before the
        step: eval_metrics into `valid_metrics_<i>`, '<metric>_<i>.txt', and - past step 0 - 'model_pars' / 'teacher_pars'
        (.npz, or .h5 where h5py is importable) and the max_* files.  Each iteration: train_step, then ema_apply with MT_SSL."""
        from . import weights_io
        from .eval_utils import eval_metrics
        ext = '.h5' if weights_io.have_h5py() else '.npz'
        if len(metric_gens) > 0 and not isinstance(metric_gens[0], list):
            metric_gens = [metric_gens]
        for i, mg in enumerate(metric_gens):
            valid = {}
            for metric in mg[0]:
                path = os.path.join(save_path, '%s_%d.txt' % (metric, i)) if save_path is not None else None
                valid[metric] = list(np.atleast_1d(np.loadtxt(path))) if path is not None and os.path.exists(path) else []
            setattr(self, 'valid_metrics_%d' % i, valid)
        teacher = getattr(self, 'teacher', None)
        while self.global_step < global_step_limit:
            step = self.global_step
            batch_X, batch_Y = train_gen()
            if step % eval_step == 0:
                for i, mg in enumerate(metric_gens):
                    eval_metrics(self, sess, mg[1], mg[2], True, 'valid_metrics_%d' % i)
                    if save_path is None:
                        continue
                    for metric in mg[0]:
                        np.savetxt(os.path.join(save_path, '%s_%d.txt' % (metric, i)), getattr(self, 'valid_metrics_%d' % i)[metric])
                    if step > 0:
                        self.save_weights(os.path.join(save_path, 'model_pars' + ext))
                        if teacher is not None:
                            teacher.save_weights(os.path.join(save_path, 'teacher_pars' + ext))
                        if len(metric_gens[0]) == 4:
                            V = np.asarray(self.valid_metrics_0[metric_gens[0][3]])
                            if np.all(V[-1] > V[:-1]):
                                np.savetxt(os.path.join(save_path, 'max_valid_iter.txt'), [step])
                                self.save_weights(os.path.join(save_path, 'max_model_pars' + ext))
                                if teacher is not None:
                                    teacher.save_weights(os.path.join(save_path, 'max_teacher_pars' + ext))
            # (a model without dropout layers carries dropout_rate = 1, NN.py's convention: nothing is dropped)
            feed_dict = {self.x: batch_X, self.y_: batch_Y, self.keep_prob: 1. - self.dropout_rate if len(self.dropout_layers) else 1.}
            if teacher is not None:
                feed_dict[teacher.keep_prob] = 1. - teacher.dropout_rate if len(teacher.dropout_layers) else 1.
            sess.run(self.train_step, feed_dict=feed_dict)
            if getattr(self, 'MT_SSL', False):
                sess.run(self.ema_apply)
