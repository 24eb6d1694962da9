"""Host side of the aleatoric-uncertainty head (AU_4U): the fp64 statement of the cotangent (nnal_amd.mteach.evaluate_au) against
central differences and against the plain mean-teacher statement, the keyword checks of NN_extended.CNN, full_slice_segment's
four aleatoric ops on a stub model, extend_weights_to_aleatoric_mode and the declared symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

from nnal_amd import NN_extended, device, eval_utils, model_utils, mteach, netspec, weights_io
from tests import aleatoric_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('alq_dense_head_fwd_au', 'alq_model_set_aleatoric', 'alq_forward_au', 'alq_mt_cotangent_au', 'alq_mt_stats_au',
               'alq_param_grads_loss_mt_au', 'alq_mt_au_trip_voxels')


def _posteriors(rs, c, R):
    z = rs.randn(c, R) * 2.
    e = np.exp(z - z.max(0))
    return e / e.sum(0)


@pytest.mark.parametrize('measure', [mteach.L2, mteach.CE])
@pytest.mark.parametrize('c', [2, 3, 7])
def test_evaluate_au_against_central_differences(c, measure):
    """rows = dF / dz of F = s sum l + k sum (div e + kappa a / 2) at the c + 1 logits, through softmax and ReLU (cons_scale =
    2 k / c, au_scale = k).  CE: TF does not differentiate the labels, so only the log-variance column is F's gradient."""
    R, h, s, k, kappa = 50, 1e-6, 0.7, 0.9, 0.1
    z, seed = aleatoric_ref.draw_logits(R, c, 100 * c + measure)
    assert np.abs(z[:, c]).min() > 1e-3          # no voxel within the step of the ReLU's kink: none is excluded
    rs = np.random.RandomState(seed + 1)
    tpost = _posteriors(rs, c, R)
    labels = rs.randint(-1, c, size=R)           # -1: unlabelled
    post, a = aleatoric_ref.split(z)
    ev = mteach.evaluate_au(post, tpost, a, labels, measure, loss_scale=s, cons_scale=2. * k / c, au_scale=k, kappa=kappa)
    num = aleatoric_ref.central_differences(z, h, tpost, labels, measure, s, k, kappa)
    cols = slice(None) if measure == mteach.L2 else slice(c, c + 1)
    err = np.abs(ev['rows'] - num)[:, cols].max()
    scale = np.abs(ev['rows']).max()
    print('c=%d measure=%d seed=%d: worst |rows - central difference| %.3e on rows of size %.3e' % (c, measure, seed, err, scale))
    assert err <= 1e-7 * scale
    assert (ev['rows'][a == 0, c] == 0).all() and (a == 0).any() and (a > 0).any()
    assert ev['stats'][2] == pytest.approx(float((ev['div'] * np.exp(-a) + 0.5 * np.float32(kappa) * a).sum()), rel=1e-15)


@pytest.mark.parametrize('measure', [mteach.L2, mteach.CE])
@pytest.mark.parametrize('c', [2, 3, 7])
def test_zero_variance_is_the_mean_teacher_statement(c, measure):
    R = 60
    rs = np.random.RandomState(5 + c)
    p, q = _posteriors(rs, c, R).astype(np.float32), _posteriors(rs, c, R).astype(np.float32)
    labels = rs.randint(-1, c, size=R)
    sw = (0.25 + rs.rand(R)).astype(np.float32)
    kw = dict(class_w=np.asarray([0.3, 1.7], np.float32), focal_gamma=2.) if c == 2 else {}
    a = mteach.evaluate_au(p, q, np.zeros(R, np.float32), labels, measure, 0.3, 0.04, 0.5, 0., sample_w=sw, **kw)
    b = mteach.evaluate(p, q, labels, measure, 0.3, 0.04, sample_w=sw, **kw)
    assert np.array_equal(a['rows'][:, :c], b['rows']) and not a['rows'][:, c].any()
    assert a['rows'].shape == (R, c + 1) and a['labelled_rows'].shape == (R, c + 1) and a['cons_rows'].shape == (R, c + 1)
    assert tuple(a['stats']) == tuple(b['stats']) and np.array_equal(a['div'], b['div'])


def test_aleatoric_keyword_checks_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was opened')
    monkeypatch.setattr(device, 'default_session', no_device)
    monkeypatch.setattr(NN_extended, 'default_session', no_device)
    ld3, sk3 = netspec.net_c_2d_dense(3)
    ld2, sk2 = netspec.net_c_2d_dense(2)
    with pytest.raises(AssertionError, match='the device was opened'):      # a valid aleatoric mean-teacher model goes on to the device
        NN_extended.CNN((16, 16, 1), ld3, 'm', sk3, MT_SSL=True, AU_4U=True, AU_log_rel_coeff=0.2, output_perturbation_measure='L2')
    with pytest.raises(AssertionError, match='the device was opened'):      # ... and one without MT_SSL: it builds and evaluates
        NN_extended.CNN((16, 16, 1), ld3, 'm', sk3, AU_4U=True)
    with pytest.raises(NotImplementedError, match='AU_4L'):
        NN_extended.CNN((16, 16, 1), ld3, 'm', sk3, MT_SSL=True, AU_4L=True)
    with pytest.raises(NotImplementedError, match='AU_4L'):
        NN_extended.CNN((16, 16, 1), ld3, 'm', sk3, AU_4U=True, AU_4L=True)
    with pytest.raises(NotImplementedError, match='fc-head'):
        NN_extended.CNN((8, 8, 1), {'c1': ['conv', [4, [3, 3]], 'MA'], 'f': ['fc', [3]]}, 'm', AU_4U=True)
    for kw in (dict(MT_SSL=True), {}):
        with pytest.raises(NotImplementedError, match='2 channels'):
            NN_extended.CNN((16, 16, 1), ld2, 'm', sk2, AU_4U=True, **kw)
    ld4, sk4 = netspec.net_c_2d_dense(4)
    with pytest.raises(ValueError):          # class weights read the classes beside the log-variance: three of them here
        NN_extended.CNN((16, 16, 1), ld4, 'm', sk4, AU_4U=True, MT_SSL=True, bin_class_weights=[0.3, 1.7])
    assert 'AU_4U' not in NN_extended.CNN.REFUSED_WITH_MT and 'AU_4L' in NN_extended.CNN.REFUSED_WITH_MT


# ------------------------------------------------------------------------------------------ full_slice_segment
class _AUStub(object):
    """model + sess in one: output is a known function of the input; a run at keep_prob < 1 adds the count of such runs so far to
    the raw log-variance channel."""
    dense = False
    AU_4U = True
    class_num = 2
    dropout_rate = 0.25

    def __init__(self, in_shape):
        self.in_shape = in_shape
        for nme in ('x', 'keep_prob', 'y_', 'posteriors', 'loss', 'AU_vals', 'output'):
            setattr(self, nme, device.Handle(nme))
        self.log, self.calls = [], 0

    @staticmethod
    def raw(x):
        """[..., m] -> [..., 3]: two class logits and the raw log-variance channel, negative on about half the voxels."""
        s = (x * np.arange(1, x.shape[-1] + 1)).sum(-1)
        return np.stack([s, -s, np.sin(3. * s)], axis=-1)

    def run(self, fetch, feed_dict=None):
        x, kp = feed_dict[self.x], feed_dict[self.keep_prob]
        self.log.append((fetch.name, x.shape, kp))
        out = self.raw(x)
        if kp < 1.:
            out[..., 2] += self.calls
            self.calls += 1
        return np.maximum(out[..., 2], 0.) if fetch.name == 'AU_vals' else out


def test_full_slice_segment_aleatoric_ops_on_a_stub_model():
    h, w, z = 5, 6, 10
    rs = np.random.RandomState(0)
    vols = [rs.randn(h, w, z), rs.randn(h, w, z)]
    st = _AUStub((h, w, 2))
    want = _AUStub.raw(np.stack(vols, axis=-1))          # (h, w, z, 3)
    assert (want[..., 2] < 0).any() and (want[..., 2] > 0).any()
    au = eval_utils.full_slice_segment(st, st, vols, None, 'AU_vals')
    assert au.shape == (h, w, z) and np.array_equal(au, np.maximum(want[..., 2], 0.))
    assert [e[0] for e in st.log] == ['AU_vals'] * 3 and [e[1][0] for e in st.log] == [4, 4, 2] and all(e[2] == 1. for e in st.log)
    out = eval_utils.full_slice_segment(st, st, vols, None, 'output')
    assert out.shape == (3, h, w, z) and np.array_equal(out, np.moveaxis(want, -1, 0))
    sig = eval_utils.full_slice_segment(st, st, vols, None, 'sigma')
    assert sig.shape == (2, h, w, z)          # the one raw channel, broadcast over the c planes as the reference's assignment does
    assert np.array_equal(sig[0], want[..., 2]) and np.array_equal(sig[1], want[..., 2])
    st.log, st.calls = [], 0
    mc = eval_utils.full_slice_segment(st, st, vols, None, 'MC-sigma')
    assert mc.shape == (2, h, w, z) and np.array_equal(mc[0], mc[1])
    assert len(st.log) == 30 and all(e[0] == 'output' and e[2] == 0.75 for e in st.log)          # 10 runs a batch at 1 - dropout_rate
    per_slice = (mc[0] - want[..., 2]).reshape(-1, z)          # batch k of the run holds mean(10 k .. 10 k + 9) above the raw channel
    assert np.allclose(per_slice, per_slice[0], atol=1e-9)
    assert np.allclose(sorted(per_slice[0]), sorted(np.repeat([4.5, 14.5, 24.5], [4, 4, 2])), atol=1e-9)
    st.AU_4U = False          # any other model keeps the refusal
    for op in ('output', 'AU_vals', 'sigma', 'MC-sigma'):
        with pytest.raises(NotImplementedError):
            eval_utils.full_slice_segment(st, st, vols, None, op)


# ------------------------------------------------------------------------------------------ extend_weights_to_aleatoric_mode
def test_extend_weights_to_aleatoric_mode_on_an_npz(tmp_path, capsys):
    rs = np.random.RandomState(2)
    pars = {'c1': (rs.randn(3, 3, 1, 4).astype(np.float32), rs.randn(4).astype(np.float32)),
            'last': (rs.randn(1, 1, 4, 2).astype(np.float32), rs.randn(2).astype(np.float32))}
    path = str(tmp_path / 'pars.npz')
    weights_io.write_weights(path, pars)
    new = model_utils.extend_weights_to_aleatoric_mode(path, 3)
    assert new == str(tmp_path / 'pars_extended.npz') and sorted(os.listdir(str(tmp_path))) == ['pars.npz', 'pars_extended.npz']
    got = weights_io.read_weights(new, ['c1', 'last'])
    W, b = got['last']
    assert W.shape == (1, 1, 4, 3) and b.shape == (3,) and W.dtype == np.float32 and b.dtype == np.float32
    assert W[..., :2].tobytes() == pars['last'][0].tobytes() and b[:2].tobytes() == pars['last'][1].tobytes()
    assert not W[..., 2].any() and b[2] == 0
    assert got['c1'][0].tobytes() == pars['c1'][0].tobytes() and got['c1'][1].tobytes() == pars['c1'][1].tobytes()
    assert weights_io.layer_names(new) == ['c1', 'last']
    # out_channels = 2 c: the reference's doubling
    four = weights_io.read_weights(model_utils.extend_weights_to_aleatoric_mode(path, 4, last_layer_name='last'), ['last'])['last']
    assert four[0].shape == (1, 1, 4, 4) and not four[0][..., 2:].any() and not four[1][2:].any()
    os.remove(new)
    assert model_utils.extend_weights_to_aleatoric_mode(path, 2) is None          # the shape already matches: nothing written
    assert 'already match' in capsys.readouterr().out and sorted(os.listdir(str(tmp_path))) == ['pars.npz']


# ------------------------------------------------------------------------------------------ the C interface
def test_new_symbols_are_declared_and_exported():
    from nnal_amd import _lib
    names = _lib.exported_names()
    header = open(os.path.join(ROOT, 'include', 'alq.h')).read()
    for sym in NEW_SYMBOLS:
        assert sym in names, sym
        assert re.search(r'^(int|int64_t) %s\(' % sym, header, re.M), sym
