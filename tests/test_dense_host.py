"""Host side of the fully-convolutional models (no GPU): layer translation of the dense nets, the keyword checks of a dense
NN_extended.CNN, the F1 scores of eval_utils and full_slice_segment over a stub model."""
import numpy as np
import pytest

import nnal_amd  # noqa: F401
from nnal_amd import NN_extended, device, eval_utils, netspec
from nnal_amd._lib import ALQ_CONV, ALQ_CONVT, ALQ_POOL


@pytest.mark.parametrize('fn,in_shape,nd', [('net_c_dense', (8, 8, 8, 1), 3), ('net_c_2d_dense', (16, 16, 1), 2)])
@pytest.mark.parametrize('nclass', [2, 3])
def test_dense_netspecs_translate(fn, in_shape, nd, nclass):
    ld, sk = getattr(netspec, fn)(nclass)
    ld_fc, sk_fc = getattr(netspec, fn[:-len('_dense')])(nclass)
    assert list(ld.keys())[:-1] == list(ld_fc.keys())[:-1] and sk == sk_fc
    assert ld['last'] == ['conv', [nclass, [1] * nd], 'M']
    layers = device.translate_layers(ld, in_shape, sk)
    assert all(d['type'] in (ALQ_CONV, ALQ_CONVT, ALQ_POOL) for d in layers)
    head = layers[-1]
    assert head['type'] == ALQ_CONV and head['relu'] == 0 and head['k'] == [1, 1, 1] and head['s'] == [1, 1, 1]
    assert head['cout'] == nclass and head['skip_src'] == -1
    shapes = device.tf_param_shapes(layers, in_shape)
    assert shapes[-1] == ('last', (1,) * nd + (8, nclass), (nclass,))
    assert shapes == netspec.param_shapes(ld, in_shape, sk)
    trunk = netspec.param_shapes(ld_fc, in_shape, sk_fc)[:-1]
    n_par = sum(int(np.prod(w)) + int(np.prod(b)) for _, w, b in trunk) + 8 * nclass + nclass
    assert netspec.count_params(netspec.he_init(ld, in_shape, seed=1, skips=sk)) == n_par
    assert device.out_map_shape(layers, in_shape) == tuple(in_shape[:-1])


def test_dense_cnn_keyword_checks_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was opened')
    monkeypatch.setattr(device, 'default_session', no_device)
    monkeypatch.setattr(NN_extended, 'default_session', no_device)
    ld, sk = netspec.net_c_2d_dense(2)
    for name in ('GCE', 'CE_softclasses'):
        with pytest.raises(ValueError, match='fully-convolutional'):
            NN_extended.CNN((16, 16, 1), ld, 'm', sk, loss_name=name)
    with pytest.raises(NotImplementedError):
        NN_extended.CNN((16, 16, 1), ld, 'm', sk, regularizer='L2')
    ld3, sk3 = netspec.net_c_2d_dense(3)
    with pytest.raises(ValueError):
        NN_extended.CNN((16, 16, 1), ld3, 'm', sk3, focal_gamma=2.)
    with pytest.raises(AssertionError, match='the device was opened'):      # a valid dense model goes on to the device
        NN_extended.CNN((16, 16, 1), ld, 'm', sk, loss_name='CE')


# ------------------------------------------------------------------------------------------ F1 scores
def _brute_f1(p, t, j):
    tp = sum(1 for a, b in zip(p, t) if a == j and b == j)
    fp = sum(1 for a, b in zip(p, t) if a == j and b != j)
    fn = sum(1 for a, b in zip(p, t) if a != j and b == j)
    return (2. * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) else 0.), tp + fn


@pytest.mark.parametrize('C,absent', [(2, None), (3, None), (4, 2), (5, 4)])
def test_multi_f1_vs_brute_force_and_sklearn(C, absent):
    rs = np.random.RandomState(10 + C)
    t, p = rs.randint(0, C, size=(3, 7, 5)), rs.randint(0, C, size=(3, 7, 5))
    if absent is not None:          # a class with no true and no predicted voxel
        t[t == absent] = 0
        p[p == absent] = 0
    scores, av = eval_utils.multi_F1_score(p, t, C)
    brute = [_brute_f1(p.ravel(), t.ravel(), j) for j in range(1, C)]
    assert np.allclose(scores, [b[0] for b in brute], rtol=0, atol=1e-15)
    sup = np.array([b[1] for b in brute], dtype=np.float64)
    assert abs(av - float((sup * [b[0] for b in brute]).sum() / sup.sum())) <= 1e-15
    if absent is not None:
        assert scores[absent - 1] == 0.
    try:
        from sklearn.metrics import f1_score
    except ImportError:
        return
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.allclose(scores, f1_score(t.ravel(), p.ravel(), labels=np.arange(1, C), average=None), rtol=0, atol=1e-12)
        assert abs(av - f1_score(t.ravel(), p.ravel(), labels=np.arange(1, C), average='weighted')) <= 1e-12


def test_multi_f1_default_class_count_and_no_support():
    t = np.array([0, 0, 2, 2, 1])
    p = np.array([0, 2, 2, 1, 1])
    s3, a3 = eval_utils.multi_F1_score(p, t)
    assert np.allclose(s3, eval_utils.multi_F1_score(p, t, 3)[0]) and a3 == eval_utils.multi_F1_score(p, t, 3)[1]
    s, a = eval_utils.multi_F1_score(np.array([1, 0]), np.array([0, 0]), 3)
    assert list(s) == [0., 0.] and a == 0.


def test_binary_f1():
    rs = np.random.RandomState(3)
    t, p = rs.randint(0, 2, size=(6, 6, 4)), rs.randint(0, 2, size=(6, 6, 4))
    assert abs(eval_utils.binary_F1_score(p, t) - _brute_f1(p.ravel(), t.ravel(), 1)[0]) <= 1e-15
    assert eval_utils.binary_F1_score(np.zeros((4, 4)), np.zeros((4, 4))) == 0.          # P + TPFP == 0
    assert eval_utils.binary_F1_score(np.ones(5), np.ones(5)) == 1.


# ------------------------------------------------------------------------------------------ full_slice_segment
class _Stub(object):
    """model + sess in one: posteriors are a known function of the input, each run is logged."""
    dense = False
    class_num = 2
    dropout_rate = 0.25

    def __init__(self, in_shape):
        self.in_shape = in_shape
        self.x, self.keep_prob, self.y_ = device.Handle('x'), device.Handle('keep_prob'), device.Handle('y_')
        self.posteriors, self.loss = device.Handle('posteriors'), device.Handle('loss')
        self.log = []
        self.calls = 0

    @staticmethod
    def p1(x):
        return 1. / (1. + np.exp(-(x * np.arange(1, x.shape[-1] + 1)).sum(-1)))

    def run(self, fetch, feed_dict=None):
        x, kp = feed_dict[self.x], feed_dict[self.keep_prob]
        self.log.append((fetch.name, x.shape, kp))
        if fetch.name == 'loss':
            return float(x[..., 0].mean())
        p1 = self.p1(x)
        if kp < 1.:          # "dropout": pass t of a batch adds t to class 1
            p1 = p1 + self.calls
            self.calls += 1
        return np.stack([1. - p1, p1], axis=-1)


def test_full_slice_segment_on_a_stub_model():
    h, w, z = 5, 6, 10
    rs = np.random.RandomState(0)
    vols = [rs.randn(h, w, z), rs.randn(h, w, z)]
    st = _Stub((h, w, 2))
    x_all = np.stack(vols, axis=-1)                       # (h, w, z, m)
    want_p1 = _Stub.p1(x_all)                             # (h, w, z)
    np.random.seed(4)
    post = eval_utils.full_slice_segment(st, st, vols, None, 'posterior')
    assert post.shape == (2, h, w, z)
    assert np.array_equal(post[1], want_p1) and np.array_equal(post[0], 1. - want_p1)      # slice order, multi-modal stacking
    assert [e[1][0] for e in st.log] == [4, 4, 2] and all(e[1][1:] == (h, w, 2) and e[2] == 1. for e in st.log)      # a last short batch
    pred = eval_utils.full_slice_segment(st, st, vols, None, 'prediction')
    assert pred.shape == (h, w, z) and np.array_equal(pred, (want_p1 > 0.5).astype(np.float64))
    # paths through the reader, one modality
    st1 = _Stub((h, w, 1))
    got = eval_utils.full_slice_segment(st1, st1, 'vol0', lambda path: vols[0], 'posterior')
    assert np.array_equal(got[1], _Stub.p1(vols[0][..., None]))
    # 'loss': the slice-weighted running mean of the per-batch values = the mean over all slices
    np.random.seed(5)
    batches = eval_utils.gen_batch_inds(z, 4)
    assert sorted(i for b in batches for i in b) == list(range(z)) and [len(b) for b in batches] == [4, 4, 2]
    np.random.seed(5)
    loss = eval_utils.full_slice_segment(st, st, vols, None, 'loss')
    vals = [vols[0][:, :, np.sort(b)].mean() for b in batches]
    run, cnt = 0., 0
    for b, v in zip(batches, vals):
        run = (len(b) * v + cnt * run) / (cnt + len(b))
        cnt += len(b)
    assert loss == run and abs(loss - vols[0].mean()) <= 1e-12
    # 'MC-posterior': keep_prob = 1 - dropout_rate, 10 passes per batch, their running mean
    st.log, st.calls = [], 0
    mc = eval_utils.full_slice_segment(st, st, vols, None, 'MC-posterior')
    assert len(st.log) == 30 and all(e[2] == 0.75 for e in st.log)
    # pass t of the run adds t: batch k (in run order) holds mean(10 k .. 10 k + 9) = 10 k + 4.5 above p1
    extra = mc[1] - want_p1
    per_slice = extra.reshape(-1, z)
    assert np.allclose(per_slice, per_slice[0], atol=1e-9)
    assert np.allclose(sorted(per_slice[0]), sorted(np.repeat([4.5, 14.5, 24.5], [4, 4, 2])), atol=1e-9)
    # the shape assertion, the ops that are not built
    with pytest.raises(AssertionError, match='Shape of data and model.x should match'):
        eval_utils.full_slice_segment(_Stub((h + 1, w, 2)), st, vols, None, 'posterior')
    for op in ('output', 'AU_vals', 'sigma', 'MC-sigma'):
        with pytest.raises(NotImplementedError):
            eval_utils.full_slice_segment(st, st, vols, None, op)


def test_eval_metrics_on_a_stub_model():
    st = _Stub((5, 6, 2))
    st.valid_metrics = {'av_acc': [], 'F1': [], 'av_loss': []}
    rs = np.random.RandomState(1)
    batches = []

    def gen():
        x = rs.randn(3, 5, 6, 2)
        lab = rs.randint(0, 2, size=(3, 5, 6))
        batches.append((x, lab))
        return x, (lab[..., None] == np.arange(2)).astype(np.float32)
    eval_utils.eval_metrics(st, st, gen, iters=4)
    preds = np.concatenate([(_Stub.p1(x) > 0.5).astype(int) for x, _ in batches])
    labs = np.concatenate([lab for _, lab in batches])
    assert st.valid_metrics['av_acc'] == [float((preds == labs).mean())]
    assert st.valid_metrics['F1'] == [eval_utils.binary_F1_score(preds, labs)]
    assert abs(st.valid_metrics['av_loss'][0] - np.mean([x[..., 0].mean() for x, _ in batches])) <= 1e-12
    res = eval_utils.eval_metrics(st, st, gen, iters=1, update=False)
    assert set(res) == {'av_loss', 'accs', 'F1s'} and len(st.valid_metrics['F1']) == 1
