"""Fully-convolutional models on the device (csrc/dense.hip: the 1x1 conv head, its backward and the voxel-wise objective)
against an fp64 torch graph over oracle.tfops (tests/dense_ref.py; GPU box).

Inputs: the first N samples of a seeded stream whose fp64 evaluation has no ReLU input or pool near-tie within
ref64.DEFAULT_EPS (scanned on the CPU, asserted here, none dropped afterwards).  Seeds: those for which the fp32 torch
restatement's posteriors stay within 1e-6 of fp64 - measured on the CPU over every case below: at most 4.6e-7 (net_c_dense at 8x12x20; asserted per case).

Bars: posteriors 2e-6 absolute (the project's bar for scores against fp64), prediction equal wherever fp64's top two
posteriors differ by more than 4e-6 (at most 1 % of the voxels exempt), loss rtol 1e-6, every gradient array
2e-4 * max|g64| + 1e-9 (tests.test_gpu_train._close).  Each case prints e_dev / e_32, its gradient error against that of the
fp32 restatement (recorded in DESIGN.md)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dense_ref  # noqa: E402
from tests.test_gpu_losses import _TorchStep, _objective, _weights_close  # noqa: E402
from tests.test_gpu_train import _close  # noqa: E402

CW = [0.3, 1.7]
DROP_KEEP, DROP_SEED = 0.5, 20251
HEAD_SHAPES = {'5x7': ((5, 7, 1), 3), '12x20': ((12, 20, 1), 5), '4x6x5': ((4, 6, 5, 1), 2)}


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _head_net(ci, c, nd):
    from collections import OrderedDict
    return OrderedDict([('c1', ['conv', [ci, [3] * nd], 'MA']), ('last', ['conv', [c, [1] * nd], 'M'])]), []


def _labels(rs, shape, c, unlabelled=0.):
    """One-hot [N, *spatial, c]; a fraction of the voxels all zero."""
    lab = rs.randint(0, c, size=shape)
    y = (lab[..., None] == np.arange(c)).astype(np.float32)
    if unlabelled:
        y[rs.rand(*shape) < unlabelled] = 0
    return y


def _rel_err(dev, ref):
    return max(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-30) for a, b in zip(dev, ref))


def _check_case(sess, tag, ld, sk, in_shape, N, c, seed, max_batch):
    """Posteriors, prediction, and loss + gradients of the three objective variants of one model against fp64."""
    import torch
    from nnal_amd import NN_extended, netspec, ref64
    pars = netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05)
    g64 = dense_ref.DenseGraph(ld, in_shape, pars, sk, torch.float64)
    g32 = dense_ref.DenseGraph(ld, in_shape, pars, sk, torch.float32)
    x, drawn = dense_ref.select_inputs(g64, in_shape, N, seed + 1000, ref64.DEFAULT_EPS)
    with torch.no_grad():
        g64.maps(g64._as_input(x), eps=ref64.DEFAULT_EPS)
    assert g64.fragile == 0 and x.shape[0] == N
    p64 = g64.posteriors(x)
    d32 = np.abs(g32.posteriors(x).astype(np.float64) - p64).max()
    assert d32 <= 1e-6, 'seed condition: fp32 restatement %.3e from fp64' % d32

    m = NN_extended.CNN(in_shape, ld, tag, list(sk), dropout=[[0], 1. - DROP_KEEP], sess=sess, max_batch=max_batch)
    m.set_weights(pars)
    assert m.dense and m.out_voxels == int(np.prod(in_shape[:-1])) and m.out_map_shape == tuple(in_shape[:-1])
    post = sess.run(m.posteriors, feed_dict={m.x: x, m.keep_prob: 1.})
    pred = sess.run(m.prediction, feed_dict={m.x: x, m.keep_prob: 1.})
    assert post.shape == p64.shape and pred.shape == p64.shape[:-1]
    e_post = np.abs(post.astype(np.float64) - p64).max()
    print('%s: %d samples of %d drawn, |post - post64| = %.3e (fp32 restatement %.3e)' % (tag, N, drawn, e_post, d32))
    assert e_post <= 2e-6
    top2 = np.sort(p64, axis=-1)
    firm = (top2[..., -1] - top2[..., -2]) > 4e-6
    assert (~firm).mean() <= 0.01
    assert np.array_equal(pred[firm], p64.argmax(-1)[firm])

    rs = np.random.RandomState(seed + 7)
    shape = (N,) + tuple(in_shape[:-1])
    worst_ratio = 0.
    variants = [('plain', {'loss_name': 'CE'}, 0., False, 1.),
                ('weighted', dict(bin_class_weights=CW, focal_gamma=2.) if c == 2 else {'loss_name': 'CE'}, 0.3, True, 1.),
                ('dropout', {'loss_name': 'CE'}, 0., False, DROP_KEEP)]
    for name, hy, unl, weights, kp in variants:
        y = _labels(rs, shape, c, unl)
        vw = (0.25 + rs.rand(*shape)).astype(np.float32) if weights else None
        if weights:
            vw[rs.rand(*shape) < 0.05] = 0
        ycols = np.ascontiguousarray(y.reshape(-1, c).T)
        m.set_hypers(dict(NN_extended.CNN.DEFAULT_HYPERS, **hy))
        refs = []
        for g in (g64, g32):
            g.drop = dict(layers=[0], keep_prob=kp, seed=DROP_SEED, first_sample=0) if kp < 1. else None
            z = g._graph(g._as_input(x))['output']
            val, diff = _objective(hy, z, ycols, None if vw is None else vw.reshape(-1))
            refs.append((float(val.detach()), dense_ref.flat_grads(g, diff)))
            g.drop = None
        (l64, gr64), (_, gr32) = refs
        t, n = m._as_device_batch(x)
        gsum, l_dev = m._objective_pass(t, n, ycols, kp, DROP_SEED, None if vw is None else vw.reshape(-1), None)
        gdev = m.unflatten(gsum.cpu().numpy())
        if kp == 1.:          # the same figures through the reference's call shapes
            fd = {m.x: x, m.y_: y, m.keep_prob: 1.}
            if vw is not None:
                fd[m.input_vox_weights] = vw
            assert sess.run(m.loss, feed_dict=fd) == l_dev
            g2 = m.mean_loss_grad(x, None, 'all', targets=ycols, input_weights=None if vw is None else vw.reshape(-1))
            assert all(np.array_equal(a, b) for a, b in zip(g2, gdev))
        e_dev, e_32 = _rel_err(gdev, gr64), _rel_err(gr32, gr64)
        worst_ratio = max(worst_ratio, e_dev / max(e_32, 1e-30))
        print('%s %s: loss %.9g vs %.9g (rel %.2e), gradients e_dev %.3e e_32 %.3e e_dev / e_32 = %.2f'
              % (tag, name, l_dev, l64, abs(l_dev - l64) / abs(l64), e_dev, e_32, e_dev / max(e_32, 1e-30)))
        assert abs(l_dev - l64) <= 1e-6 * abs(l64), (name, l_dev, l64)
        _close(gdev, gr64, name='%s %s' % (tag, name))
    _reproducible(sess, m, x, ycols)
    m.close()
    return worst_ratio


def _reproducible(sess, m, x, ycols):
    """Two identical alq_param_grads_loss calls: identical bits of d_grads and d_post."""
    from nnal_amd._lib import LossT, check
    torch = sess.torch
    n = min(x.shape[0], m.max_batch)
    V, c = m.out_voxels, m.nclass
    t = sess.to_device(x[:n].reshape(n, -1), torch.float32)
    lab = sess.to_device(np.where(ycols.sum(0) > 0, ycols.argmax(0), -1).astype(np.int32)[:n * V], torch.int32)
    L = LossT(0, -1., 0.7, 1., None, None, None, None)
    outs = []
    for _ in range(2):
        g = torch.full((m.num_params,), float('nan'), dtype=torch.float32, device=t.device)
        p = torch.full((c, n * V), float('nan'), dtype=torch.float32, device=t.device)
        st = sess.empty((3,), torch.float64)
        sess.bind_stream()
        check(m.lib.alq_param_grads_loss(m._m, C.c_void_p(t.data_ptr()), n, C.c_void_p(lab.data_ptr()), C.byref(L), 1. / (n * V), 0., 1., 0, 0,
                                         None, 0, C.c_void_p(g.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(st.data_ptr())))
        outs.append((g.cpu().numpy(), p.cpu().numpy()))
    assert not np.isnan(outs[0][0]).any() and not np.isnan(outs[0][1]).any()
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()


@pytest.mark.parametrize('c', [2, 3, 8])
@pytest.mark.parametrize('ci', [4, 8, 12, 16, 20, 64])
@pytest.mark.parametrize('shape', sorted(HEAD_SHAPES))
def test_head_alone_vs_fp64(sess, shape, ci, c):
    """conv(Ci, 3x3, ReLU) + the 1x1 head.  5x7 with N = 3: 105 voxels, under one workgroup and no multiple of 4 (the guarded
    one-voxel path); 12x20 with N = 5 at max_batch 4: 16-byte path, two passes; 3-D 4x6x5.  Ci = 12 and 20: 3 and 5 16-byte
    pieces a row, so the backward workgroup sweeps 85 and 51 rows with lanes idle (the kernels on their own:
    tests/test_gpu_dense_head.py)."""
    in_shape, N = HEAD_SHAPES[shape]
    ld, sk = _head_net(ci, c, len(in_shape) - 1)
    _check_case(sess, 'head %s Ci=%d c=%d' % (shape, ci, c), ld, sk, in_shape, N, c, seed=300 + ci + c, max_batch=4)


NETS = {
    '2d_c2': ('net_c_2d_dense', 2, (16, 16, 1), 3, 44),
    '2d_c3': ('net_c_2d_dense', 3, (16, 16, 1), 3, 44),
    '3d_8': ('net_c_dense', 2, (8, 8, 8, 1), 2, 53),
    '3d_ragged': ('net_c_dense', 2, (8, 12, 20, 1), 2, 53),      # ragged slabs
}


@pytest.mark.parametrize('net', sorted(NETS))
def test_whole_nets_vs_fp64(sess, net):
    from nnal_amd import netspec
    fn, c, in_shape, N, seed = NETS[net]
    ld, sk = getattr(netspec, fn)(c)
    _check_case(sess, 'net %s' % net, ld, sk, in_shape, N, c, seed=seed, max_batch=8)


@pytest.mark.parametrize('opt', ['SGD', 'Adam'])
def test_three_train_steps_vs_numpy_stepper(sess, opt):
    """sess.run(model.train_step) with y_ [N, 16, 16, c] and input_vox_weights against tests.test_gpu_losses._TorchStep on
    the fp32 graph, with that file's bounds for fc-head models (loss 2e-5, weights 2e-5 under SGD and 5e-4 under Adam)."""
    import torch
    from nnal_amd import NN_extended, netspec
    ld, sk = netspec.net_c_2d_dense(2)
    in_shape = (16, 16, 1)
    lr, bound = (0.003, 2e-5) if opt == 'SGD' else (0.002, 5e-4)
    hy = dict(bin_class_weights=CW, optimizer_name=opt, learning_rate=lr, beta1=0.8, beta2=0.99)
    pars = netspec.he_init(ld, in_shape, seed=74, skips=sk, bias_std=0.05)
    m = NN_extended.CNN(in_shape, ld, 'train', list(sk), sess=sess, max_batch=8, **hy)
    m.set_weights(pars)
    m.get_optimizer()
    g32 = dense_ref.DenseGraph(ld, in_shape, pars, sk, torch.float32)
    ref = _TorchStep(g32, hy, lr)
    for step in range(3):
        rs = np.random.RandomState(30 + step)
        x = rs.randn(6, *in_shape).astype(np.float32)
        y = _labels(rs, (6, 16, 16), 2, 0.3)
        vw = (0.25 + rs.rand(6, 16, 16)).astype(np.float32)
        l_dev = sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1., m.input_vox_weights: vw})
        l_ref = ref.step(x, np.ascontiguousarray(y.reshape(-1, 2).T), vw.reshape(-1))
        assert abs(l_dev - l_ref) <= 2e-5 * max(1., abs(l_ref)), (step, l_dev, l_ref)
    _weights_close(m, g32, bound, lr, 'dense %s' % opt)
    m.close()


def _null_args(name):
    from nnal_amd import _lib
    out = []
    for ty in _lib._SIGNATURES[name][1][1:]:
        out.append(None if ty is C.c_void_p or hasattr(ty, 'contents') else ty(0))
    return out


def test_refusals(sess):
    """fc-only entry points return ALQ_EUNSUPPORTED (-4) on a dense model and the Python methods raise; unsupported heads are
    refused at creation; an fc-head model reports one output voxel."""
    from nnal_amd import PW_NNAL, device, netspec
    from nnal_amd._lib import AlqError
    ld, sk = netspec.net_c_2d_dense(2)
    m = device.DeviceModel(sess, ld, (16, 16, 1), sk, max_batch=4)
    m.set_weights(netspec.he_init(ld, (16, 16, 1), seed=3, skips=sk))
    for name in ('alq_fisher', 'alq_fisher_rows', 'alq_forward_rows', 'alq_param_grads', 'alq_grad_sqnorms', 'alq_class_layer_sums',
                 'alq_diag_fisher', 'alq_hess_vecp'):
        assert getattr(m.lib, name)(m._m, *_null_args(name)) == -4, name
        assert name.encode() in m.lib.alq_last_error(), name
    x = np.zeros((2, 16, 16, 1), np.float32)
    for call in (lambda: m.fisher(x), lambda: m.grad_log_post(x, 0), lambda: m.hess_vecp(x, [0, 0], None), lambda: m.diagonal_fisher(x),
                 lambda: m.shrunk_class_gradients(x), lambda: m.fisher_classes(x, None, None), lambda: m.llfc_grads_device(None, None, None),
                 lambda: m.grad_sqnorms_device(None, 2), lambda: m.get_gradients(['last']), lambda: PW_NNAL.committee_holder(None, m, sess),
                 lambda: sess.run(m.grad_posts['0'], feed_dict={m.x: x})):
        with pytest.raises(NotImplementedError):
            call()
    m.close()
    from collections import OrderedDict
    base = [('c1', ['conv', [8, [3, 3]], 'MA']), ('c2', ['conv', [8, [3, 3]], 'MA'])]
    bad = {
        '3x3 head': (base + [('last', ['conv', [2, [3, 3]], 'M'])], []),
        'relu head': (base + [('last', ['conv', [2, [1, 1]], 'MA'])], []),
        'c = 9': (base + [('last', ['conv', [9, [1, 1]], 'M'])], []),
        'concat head': (base + [('last', ['conv', [2, [1, 1]], 'M'])], [[0, [2], 'con']]),
    }
    for tag, (layers, skips) in bad.items():
        with pytest.raises(AlqError, match='error -4'):
            device.DeviceModel(sess, OrderedDict(layers), (8, 8, 1), skips, max_batch=2)
    ldf, skf = netspec.net_c_2d(2)
    mf = device.DeviceModel(sess, ldf, (16, 16, 1), skf, max_batch=2)
    assert mf.lib.alq_model_out_voxels(mf._m) == 1 and mf.out_voxels == 1 and not mf.dense
    mf.close()


EVAL_SEED = 19


def test_full_slice_segment_and_post_processing(sess):
    """eval_utils.full_slice_segment on a 16x16x6 volume: 'posterior' and 'prediction' equal per-batch sess.run results placed
    by hand; get_full_segs(post_process=True) equals the host post-processing (regions.py) of the same prediction."""
    from nnal_amd import NN_extended, eval_utils, netspec, regions
    ld, sk = netspec.net_c_2d_dense(2)
    m = NN_extended.CNN((16, 16, 1), ld, 'seg', list(sk), sess=sess, max_batch=8)
    m.set_weights(netspec.he_init(ld, (16, 16, 1), seed=EVAL_SEED, skips=sk, bias_std=0.05))
    vol = np.random.RandomState(EVAL_SEED).randn(16, 16, 6).astype(np.float32)
    want_post, want_pred = np.zeros((2, 16, 16, 6)), np.zeros((16, 16, 6))
    np.random.seed(11)
    for batch in eval_utils.gen_batch_inds(6, 4):
        inds = np.sort(batch)
        P = sess.run(m.posteriors, feed_dict={m.x: np.moveaxis(vol[:, :, inds], -1, 0)[..., None], m.keep_prob: 1.})
        for k, zi in enumerate(inds):
            want_post[:, :, :, zi] = np.moveaxis(P[k], -1, 0)
            want_pred[:, :, zi] = P[k].argmax(-1)
    np.random.seed(11)
    post = eval_utils.full_slice_segment(m, sess, vol, None, 'posterior')
    np.random.seed(11)
    pred = eval_utils.full_slice_segment(m, sess, [vol], None, 'prediction')
    assert post.shape == (2, 16, 16, 6) and np.array_equal(post, want_post)
    assert pred.shape == (16, 16, 6) and np.array_equal(pred, want_pred)
    assert pred[0, 0, 0] == 0 and 0 < pred.sum() < pred.size          # a foreground to post-process, the origin in the background

    class Dat(object):
        mods = ['T1']
        img_addrs = {'T1': [vol]}
        mask_addrs = [np.zeros((16, 16, 6))]
        mask_reader = staticmethod(lambda a: a)
        reader = None
    np.random.seed(11)
    segs = eval_utils.get_full_segs({'(16, 16)': m}, sess, Dat(), post_process=True)
    host = regions.fill_holes_host(regions.keep_largest_host(pred))
    assert len(segs) == 1 and np.array_equal(segs[0], host)
    m.close()
