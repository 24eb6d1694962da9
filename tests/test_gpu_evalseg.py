"""Segmentation evaluation on the device (GPU box): eval_utils.eval_metrics / eval_confusion of a dense model fed
(device X, DeviceLabels) against the host path fed the same batches as arrays; eval_full_segs_* with a session against the
reference's doubles (tests/golden/evalseg.npz) and against their NumPy path; alq_cc_sizes / alq_cc_relabel against sizes from
regions.cc_label_host; the lesion functions against the reference under the tie condition of tests/evalseg_cases.py and against
the stable restatement exactly.  Integer and double equalities."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import evalseg_cases as ec  # noqa: E402
from tests import postproc_cases as pc  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


@pytest.fixture(scope='module')
def g():
    return ec.golden()


# ------------------------------------------------------------------------------------------------ eval_metrics
def _model(sess, tag, c):
    from nnal_amd import NN_extended, netspec
    ld, sk = netspec.net_c_2d_dense(c)
    m = NN_extended.CNN((16, 16, 2), ld, tag, list(sk), sess=sess, max_batch=8, learning_rate=0.01)
    m.set_weights(netspec.he_init(ld, (16, 16, 2), seed=91 + c, skips=sk, bias_std=0.05))
    return m


def _batches(sess, c, iters=4, b=3):
    """[(device X, DeviceLabels)]: 20 % of the label voxels at -1."""
    from nnal_amd.datasets import DeviceLabels
    torch = sess.torch
    rs = np.random.RandomState(500 + c)
    out = []
    for _ in range(iters):
        X = rs.randn(b, 16, 16, 2).astype(np.float32)
        lab = rs.randint(0, c, size=(b, 16, 16)).astype(np.int32)
        lab[rs.rand(b, 16, 16) < 0.2] = -1
        counts = [int(np.sum(lab == k)) for k in range(c)] + [int(np.sum(lab == -1))]
        out.append((sess.to_device(X, torch.float32), DeviceLabels(sess.to_device(lab, torch.int32), c, counts)))
    return out


def _cycle(items):
    state = {'k': 0}

    def gen():
        item = items[state['k'] % len(items)]
        state['k'] += 1
        return item
    return gen


@pytest.mark.parametrize('c', [2, 3])
def test_eval_metrics_on_the_device_equals_the_host_path(sess, c, monkeypatch):
    from nnal_amd import eval_utils
    from nnal_amd.datasets import DeviceLabels
    m = _model(sess, 'evalseg_c%d' % c, c)
    dev = _batches(sess, c)
    host = [(X.cpu().numpy(), np.asarray(Y)) for X, Y in dev]
    assert host[0][1].shape == (3, 16, 16, c) and np.any(host[0][1].sum(axis=-1) == 0)          # all-zero rows: unlabelled voxels

    # the host path, fed arrays
    m.valid_metrics = {'acc': [], 'F1': [], 'av_loss': []}
    with monkeypatch.context() as mp:
        mp.setattr(eval_utils, '_on_device', lambda model: False)
        eval_utils.eval_metrics(m, sess, _cycle(host), iters=4)
        M_host = eval_utils.eval_confusion(m, sess, _cycle(host), iters=4)
    want = {k: list(v) for k, v in m.valid_metrics.items()}
    # ... which is the reference's arithmetic on the concatenated maps
    preds = np.concatenate([np.argmax(sess.run(m.posteriors, feed_dict={m.x: X, m.keep_prob: 1.}), axis=-1) for X, _ in host])
    masks = np.concatenate([np.argmax(Y, axis=-1) for _, Y in host])
    assert want['acc'] == [float(np.sum(preds == masks)) / preds.size]
    TP, den = np.sum(preds * masks), np.sum(masks) + np.sum(preds)
    assert want['F1'] == [2 * TP / den if c == 2 else eval_utils.multi_F1_score(preds, masks, c)[1]]
    assert 0 < want['acc'][0] < 1 and 0 < want['F1'][0] < 1

    # the device path: no one-hot from DeviceLabels, no posterior map through sess.run
    m.valid_metrics = {'acc': [], 'F1': [], 'av_loss': []}
    with monkeypatch.context() as mp:
        def no_array(self, *a, **k):
            raise AssertionError('DeviceLabels.__array__ on the device path')
        run = sess.run

        def guarded_run(fetch, feed_dict=None):
            assert fetch is not m.posteriors, 'sess.run(model.posteriors) on the device path'
            return run(fetch, feed_dict)
        mp.setattr(DeviceLabels, '__array__', no_array)
        mp.setattr(sess, 'run', guarded_run)
        eval_utils.eval_metrics(m, sess, _cycle(dev), iters=4)
        M_dev = eval_utils.eval_confusion(m, sess, _cycle(dev), iters=4)
        res = eval_utils.eval_metrics(m, sess, _cycle(dev), iters=4, update=False)
    got = m.valid_metrics
    print('c=%d device %r host %r' % (c, got, want))
    assert got['acc'] == want['acc'] and got['F1'] == want['F1'] and got['av_loss'] == want['av_loss']
    assert set(res) == {'av_loss', 'accs', 'F1s'} and res['accs'] == want['acc'][0] and res['F1s'] == want['F1'][0]

    # eval_confusion: np.int64 [C, C], [true, predicted], the NumPy confusion of the host predictions
    assert M_dev.dtype == np.int64 and M_dev.shape == (c, c)
    np.testing.assert_array_equal(M_dev, eval_utils.confusion_matrix(preds, masks, c))
    np.testing.assert_array_equal(M_dev, M_host)
    assert M_dev.sum() == preds.size
    # a host one-hot fed to the device path: reduced to ids and uploaded, the same matrix
    np.testing.assert_array_equal(eval_utils.eval_confusion(m, sess, _cycle(host), iters=4), M_dev)
    m.close()


# ------------------------------------------------------------------------------------------------ whole-volume scores
def test_full_segs_with_a_session_equal_the_reference(sess, g, capsys):
    from nnal_amd import eval_utils
    segs, masks = [g['ep_seg_0'], g['ep_seg_1']], [g['ep_mask_0'], g['ep_mask_1']]
    calls = []
    counting = sess.confusion_counts

    def spy(*a, **k):
        calls.append(k)
        return counting(*a, **k)
    sess.confusion_counts = spy
    try:
        overall, parts = eval_utils.eval_full_segs_explicit_partitions(segs, masks, g['ep_list'].tolist(), sess=sess)
        np.testing.assert_array_equal(overall, g['ep_list_overall'])
        np.testing.assert_array_equal(parts, g['ep_list_parts'])
        overall, parts = eval_utils.eval_full_segs_explicit_partitions(segs, masks, np.array(g['ep_array']), sess=sess)
        np.testing.assert_array_equal(overall, g['ep_array_overall'])
        np.testing.assert_array_equal(parts, g['ep_array_parts'])
        assert len(calls) == 4 and all(k['inner'] == 1 and k['groups'] == 24 for k in calls)          # one launch per subject
        segs, masks = [g['lp_seg_0'], g['lp_seg_1']], [g['lp_mask_0'], g['lp_mask_1']]
        overall, parts = eval_utils.eval_full_segs_label_percentage(segs, masks, int(g['lp_label']), float(g['lp_percentage']), sess=sess)
        np.testing.assert_array_equal(overall, g['lp_overall'])
        np.testing.assert_array_equal(parts, g['lp_parts'])
        assert 'more than one gap' in capsys.readouterr().out
        with pytest.raises(IndexError):
            eval_utils.eval_full_segs_label_percentage([g['lp_nogap_seg']], [g['lp_nogap_mask']], 1, 0.25, sess=sess)
        assert len(calls) == 7
    finally:
        del sess.confusion_counts


def test_full_segs_with_a_session_equal_the_numpy_path(sess):
    """21 x 19 x 70, values in {0, 1, 2}: more slices than a wave has lanes."""
    from nnal_amd import eval_utils
    rs = np.random.RandomState(61)
    H, W, Z = pc.BOX
    mask = np.zeros(pc.BOX, dtype=np.uint8)
    mask[3:15, 2:16, 12:55] = 1
    mask[6:11, 5:12, 25:40] = 2
    mask[:3, :, :] = 1                                   # a seventh of every slice: the thin slices still hold label 1
    seg = mask.copy()
    flip = rs.rand(*pc.BOX) < 0.1
    seg[flip] = rs.randint(0, 3, size=int(flip.sum()))
    for s, m in ((seg, mask), (seg.astype(np.float64), mask.astype(np.float64))):
        for parts in ([[20, 45]], np.array([[1, 2, 69]]), [[0, 70]], [[-5, 33]]):
            a = eval_utils.eval_full_segs_explicit_partitions([s], [m], parts, sess=sess)
            b = eval_utils.eval_full_segs_explicit_partitions([s], [m], parts)
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
        a = eval_utils.eval_full_segs_label_percentage([s], [m], 1, 0.3, sess=sess)
        b = eval_utils.eval_full_segs_label_percentage([s], [m], 1, 0.3)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert np.all(a[1] > 0)
        # the reference's statement on the slices themselves
        label_num = np.sum(m == 1, axis=(0, 1))
        thr = np.where(label_num / (H * W) < 0.3)[0]
        gap = np.where((thr[1:] - thr[:-1]) > 1)[0]
        e1, e2 = thr[gap[0]], thr[gap[0] + 1]
        sp, mp_ = s[:, :, e1:e2].astype(np.int64), m[:, :, e1:e2].astype(np.int64)
        assert a[1][0, 1] == 2 * np.sum(sp * mp_) / (np.sum(mp_) + np.sum(sp))


# ------------------------------------------------------------------------------------------------ sizes and relabelling
def _host_sizes(lab):
    """sizes [n] at the roots from host labels"""
    flat = lab.reshape(-1)
    sizes = np.zeros(flat.size, dtype=np.int32)
    roots, counts = np.unique(flat[flat >= 0], return_counts=True)
    sizes[roots] = counts
    return sizes.reshape(lab.shape)


def _check_sizes_and_relabel(sess, seg, lab):
    """`lab`: the expected labels of `seg` (26-connected)"""
    torch = sess.torch
    d_lab = sess.cc_label(sess.to_device(np.asarray(seg, dtype=np.uint8), torch.uint8), seg.shape, 26)
    np.testing.assert_array_equal(d_lab.cpu().numpy().reshape(seg.shape), lab)
    sizes = sess.cc_sizes(d_lab)
    assert sizes.dtype == torch.int32 and sizes.shape == d_lab.shape
    want = _host_sizes(lab)
    np.testing.assert_array_equal(sizes.cpu().numpy().reshape(seg.shape), want)
    assert want.sum() == np.count_nonzero(seg)
    flat_l, flat_s = lab.reshape(-1), want.reshape(-1)
    for thr in (0, 1, 2, 5, int(want.max()), int(want.max()) + 1):
        mask = sess.cc_relabel(d_lab, sizes=sizes, min_size=thr)
        assert mask.dtype == torch.uint8
        np.testing.assert_array_equal(mask.cpu().numpy().reshape(-1), (flat_l >= 0) & (flat_s[np.maximum(flat_l, 0)] >= thr))
    table = np.random.RandomState(7).randint(1, 1 << 30, size=flat_l.size).astype(np.int32)
    img = sess.cc_relabel(d_lab, table=sess.to_device(table.reshape(lab.shape), torch.int32).reshape(d_lab.shape))
    assert img.dtype == torch.int32
    np.testing.assert_array_equal(img.cpu().numpy().reshape(-1), np.where(flat_l >= 0, table[np.maximum(flat_l, 0)], 0))


@pytest.mark.parametrize('shape', [pc.BOX, pc.SMALL, pc.FLAT])
def test_sizes_and_relabel_random_volumes(sess, shape):
    for d in pc.DENSITIES:
        _check_sizes_and_relabel(sess, np.array(pc.random_volume(shape, d)), pc.host_labels(shape, d, 26, False))


def test_sizes_on_built_volumes(sess):
    """One component across lanes 63 / 64 of a wave, a run that ends a row where the next row starts another component, the
    serpentine (one component in many runs), all ones, all zero."""
    names = []
    for name, seg, exp in pc.built_label_cases():
        if name.startswith('pair'):
            continue
        names.append(name)
        _check_sizes_and_relabel(sess, seg, exp[26])
    assert {'lane 63/64', 'row end on lane 63', 'serpentine', 'all ones', 'all zero'} <= set(names)


def test_sizes_and_relabel_refused_calls(sess):
    torch = sess.torch
    L = sess.lib
    lab = sess.to_device(np.array([0, 0, -1, 3], dtype=np.int32), torch.int32)
    out32 = sess.to_device(np.full(4, 77, dtype=np.int32), torch.int32)
    out8 = sess.to_device(np.full(4, 77, dtype=np.uint8), torch.uint8)
    tab = sess.to_device(np.arange(4, dtype=np.int32), torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    sess.bind_stream()
    assert L.alq_cc_sizes(sess.ctx, None, 4, p(out32)) == -1 and L.alq_cc_sizes(sess.ctx, p(lab), 4, None) == -1
    assert L.alq_cc_sizes(sess.ctx, p(lab), -1, p(out32)) == -1 and L.alq_cc_sizes(sess.ctx, p(lab), 2 ** 31, p(out32)) == -1
    assert L.alq_last_error().decode().startswith('alq_cc_sizes')
    for args in ((None, 4, p(tab), None, 0, p(out32), None), (p(lab), 4, p(tab), p(tab), 0, p(out32), p(out8)),
                 (p(lab), 4, p(tab), p(tab), 0, None, None), (p(lab), -1, p(tab), None, 0, p(out32), None),
                 (p(lab), 4, None, p(tab), 0, p(out32), None), (p(lab), 4, p(tab), None, 0, None, p(out8))):
        assert L.alq_cc_relabel(sess.ctx, *args) == -1, args
        assert L.alq_last_error().decode().startswith('alq_cc_relabel')
    torch.cuda.synchronize()
    assert out32.cpu().tolist() == [77] * 4 and out8.cpu().tolist() == [77] * 4
    assert L.alq_cc_sizes(sess.ctx, p(lab), 4, p(out32)) == 0 and out32.cpu().tolist() == [2, 0, 0, 1]
    with pytest.raises(ValueError):
        sess.cc_relabel(lab)


# ------------------------------------------------------------------------------------------------ lesions
def test_lesions_against_the_reference(sess, g):
    from nnal_amd.datasets import lesion_utils
    mask = g['lesion_mask']
    got = lesion_utils.find_lesion_components(mask, sess=sess)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == mask.shape
    assert ec.assert_ranks_match_reference(got, g['lesion_ranks']) == int(g['lesion_unique_volumes']) >= 5
    np.testing.assert_array_equal(got, ec.stable_ranks(mask))                    # the library's own tie rule, exactly
    for thr in g['lesion_thresholds']:
        drop = lesion_utils.drop_lesions_with_threshold(mask, int(thr), sess=sess)
        assert isinstance(drop, np.ndarray) and drop.dtype == np.uint8
        np.testing.assert_array_equal(drop, g['lesion_drop_%d' % thr])
    np.testing.assert_array_equal(lesion_utils.drop_lesions_with_threshold(mask, 7.5, sess=sess), ec.stable_drop(mask, 7.5))


@pytest.mark.parametrize('shape', [pc.BOX, pc.SMALL, pc.FLAT])
def test_lesions_equal_the_stable_restatement(sess, shape):
    from nnal_amd.datasets import lesion_utils
    for d in (0.05, 0.12):
        mask = np.array(pc.random_volume(shape, d))
        np.testing.assert_array_equal(lesion_utils.find_lesion_components(mask, sess=sess), ec.stable_ranks(mask))
        np.testing.assert_array_equal(lesion_utils.find_lesion_components(mask, sess=sess), lesion_utils.find_lesion_components_host(mask))
        for thr in (2, 4):
            np.testing.assert_array_equal(lesion_utils.drop_lesions_with_threshold(mask, thr, sess=sess), ec.stable_drop(mask, thr))
    img = np.array(pc.random_volume(pc.FLAT, 0.2))[:, :, 0]                      # a 2-D mask: 8-connected
    got = lesion_utils.find_lesion_components(img, sess=sess)
    assert got.shape == img.shape
    np.testing.assert_array_equal(got, ec.stable_ranks(img))


def test_lesions_device_tensor_in_device_tensor_out(sess, g):
    from nnal_amd.datasets import lesion_utils
    torch = sess.torch
    mask = np.array(g['lesion_mask'])
    d_mask = sess.to_device(mask, torch.uint8)
    ranks = lesion_utils.find_lesion_components(d_mask, sess=sess)
    assert isinstance(ranks, torch.Tensor) and ranks.is_cuda and ranks.dtype == torch.int32 and tuple(ranks.shape) == mask.shape
    np.testing.assert_array_equal(ranks.cpu().numpy(), ec.stable_ranks(mask))
    drop = lesion_utils.drop_lesions_with_threshold(d_mask.reshape(-1), 8, sess=sess, shape=mask.shape)
    assert isinstance(drop, torch.Tensor) and drop.is_cuda and drop.dtype == torch.uint8 and tuple(drop.shape) == mask.shape
    np.testing.assert_array_equal(drop.cpu().numpy(), g['lesion_drop_8'])
    np.testing.assert_array_equal(d_mask.cpu().numpy(), mask)                    # the input is left alone


def test_lesions_origin_set_and_non_binary(sess):
    from nnal_amd.datasets import lesion_utils
    torch = sess.torch
    mask = np.array(pc.random_volume(pc.SMALL, 0.2))
    mask[0, 0, 0] = 1
    want = lesion_utils.find_lesion_components_host(mask)
    assert want[0, 0, 0] == 0 and want[mask == 0].max() == 1                     # the zero set is the largest "lesion"
    np.testing.assert_array_equal(lesion_utils.find_lesion_components(mask, sess=sess), want)
    got = lesion_utils.find_lesion_components(sess.to_device(mask, torch.uint8), sess=sess)
    assert got.is_cuda and got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(lesion_utils.drop_lesions_with_threshold(mask, 3, sess=sess),
                                  lesion_utils.drop_lesions_with_threshold_host(mask, 3))
    bad = mask.copy()
    bad[2, 2, 2] = 2
    for fn in (lesion_utils.find_lesion_components, lambda m_, sess: lesion_utils.drop_lesions_with_threshold(m_, 2, sess=sess)):
        with pytest.raises(ValueError):
            fn(bad, sess=sess)
        with pytest.raises(ValueError):
            fn(sess.to_device(bad, torch.uint8), sess=sess)
