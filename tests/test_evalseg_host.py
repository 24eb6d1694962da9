"""Segmentation evaluation, host side (no GPU): the NumPy paths of eval_utils.eval_full_segs_explicit_partitions /
_label_percentage against the doubles the reference recorded (tests/golden/evalseg.npz), the confusion-matrix F1 helper against
the reference's statements of binary_F1_score / multi_F1_score, confusion_counts_host against element-by-element loops, the
host statement of the lesion functions against the reference's outputs, the C ABI's declarations, and the two plain ports
simple_eval_model / models_dict_for_different_sizes on stub models.  Integer and double EQUALITIES throughout."""
import os
import re

import numpy as np
import pytest

import nnal_amd  # noqa: F401
from nnal_amd import _lib, eval_utils
from nnal_amd.datasets import lesion_utils
from tests import evalseg_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def g():
    return ec.golden()


# ------------------------------------------------------------------------------------------------ whole-volume scores
def test_explicit_partitions_equal_the_reference(g):
    segs, masks = [g['ep_seg_0'], g['ep_seg_1']], [g['ep_mask_0'], g['ep_mask_1']]
    overall, parts = eval_utils.eval_full_segs_explicit_partitions(segs, masks, g['ep_list'].tolist())
    assert parts.shape == (2, 3)
    np.testing.assert_array_equal(overall, g['ep_list_overall'])
    np.testing.assert_array_equal(parts, g['ep_list_parts'])
    overall, parts = eval_utils.eval_full_segs_explicit_partitions(segs, masks, np.array(g['ep_array']))
    np.testing.assert_array_equal(overall, g['ep_array_overall'])
    np.testing.assert_array_equal(parts, g['ep_array_parts'])
    assert np.all(parts > 0) and len(np.unique(parts)) == parts.size          # six different scores: no range was mixed up


def test_explicit_partitions_float_maps_and_large_values(g):
    """float64 volumes (what full_slice_segment returns) count like the integers they hold; values above 15 keep NumPy's
    matrix, a non-integer map - and uint8 maps whose product wraps - the reference's own sums."""
    segs, masks = [g['ep_seg_1'].astype(np.float64)], [g['ep_mask_1'].astype(np.float64)]
    overall, parts = eval_utils.eval_full_segs_explicit_partitions(segs, masks, [[6, 15]])
    want_o, want_p = eval_utils.eval_full_segs_explicit_partitions([g['ep_seg_1']], [g['ep_mask_1']], [[6, 15]])
    np.testing.assert_array_equal(overall, want_o)
    np.testing.assert_array_equal(parts, want_p)
    for scale, dtype in ((20, np.int64), (0.5, np.float64), (20, np.uint8)):
        s, m = (g['ep_seg_1'] * scale).astype(dtype), (g['ep_mask_1'] * scale).astype(dtype)
        overall, parts = eval_utils.eval_full_segs_explicit_partitions([s], [m], [[6, 15]])
        TP, den = np.sum(s * m), np.sum(m) + np.sum(s)
        assert overall[0] == 2 * TP / den
        assert parts[0, 1] == 2 * np.sum(s[:, :, 6:15] * m[:, :, 6:15]) / (np.sum(m[:, :, 6:15]) + np.sum(s[:, :, 6:15]))


def test_label_percentage_equals_the_reference(g, capsys):
    segs, masks = [g['lp_seg_0'], g['lp_seg_1']], [g['lp_mask_0'], g['lp_mask_1']]
    overall, parts = eval_utils.eval_full_segs_label_percentage(segs, masks, int(g['lp_label']), float(g['lp_percentage']))
    np.testing.assert_array_equal(overall, g['lp_overall'])
    np.testing.assert_array_equal(parts, g['lp_parts'])
    assert np.all(parts[0] > 0) and np.all(parts[1] == 0) and overall[1] > 0          # the skipped subject: its row stays zero
    assert 'There are more than one gap for slice-wise label volume of image 1' in capsys.readouterr().out


def test_label_percentage_without_a_gap_raises_index_error(g):
    with pytest.raises(IndexError) as e:
        eval_utils.eval_full_segs_label_percentage([g['lp_nogap_seg']], [g['lp_nogap_mask']], 1, 0.25)
    assert str(e.value) == str(g['lp_nogap_error']) == 'index 0 is out of bounds for axis 0 with size 0'


def test_readers_are_used_for_paths(g):
    table = {'a': g['ep_seg_0'], 'b': g['ep_mask_0']}
    overall, parts = eval_utils.eval_full_segs_explicit_partitions(['a'], ['b'], [[8, 16]], dat_reader=table.__getitem__,
                                                                   mask_reader=table.__getitem__)
    np.testing.assert_array_equal(overall, g['ep_list_overall'][:1])
    np.testing.assert_array_equal(parts, g['ep_list_parts'][:1])


# ------------------------------------------------------------------------------------------------ F1 from a matrix
def _reference_binary(preds, labels):
    """eval_utils.binary_F1_score of the reference, its four lines."""
    TP = np.sum(preds * labels)
    P = np.sum(labels)
    TPFP = np.sum(preds)
    return 2 * TP / (P + TPFP) if P + TPFP != 0. else 0.


def _brute_multi(p, t, C):
    scores, support = np.zeros(C - 1), np.zeros(C - 1)
    for j in range(1, C):
        tp = np.sum((p == j) & (t == j))
        den = np.sum(t == j) + np.sum(p == j)
        scores[j - 1] = 2. * tp / den if den else 0.
        support[j - 1] = np.sum(t == j)
    return scores, (float(np.sum(scores * support) / support.sum()) if support.sum() else 0.)


@pytest.mark.parametrize('C', [2, 3, 5])
def test_matrix_F1_equals_the_map_scores(C):
    rs = np.random.RandomState(40 + C)
    for case in ('random', 'absent class', 'all zero'):
        p, t = rs.randint(0, C, size=(6, 9, 7)), rs.randint(0, C, size=(6, 9, 7))
        if case == 'absent class':
            t[t == C - 1] = 0                                   # no support; still predicted (C > 2) or not at all
            if C == 2:
                p[:] = 0
        if case == 'all zero':
            p[:], t[:] = 0, 0
        M = eval_utils.confusion_matrix(p, t, C)
        assert M.sum() == p.size and M[1, 0] == np.sum((t == 1) & (p == 0))          # [true, predicted]
        binary, scores, av = eval_utils.F1_from_confusion(M, C)
        assert binary == _reference_binary(p, t) == eval_utils.binary_F1_score(p, t)
        want_s, want_av = _brute_multi(p, t, C)
        got_s, got_av = eval_utils.multi_F1_score(p, t, C)
        np.testing.assert_array_equal(scores, want_s)
        np.testing.assert_array_equal(got_s, want_s)
        assert av == want_av == got_av
        if case == 'all zero':
            assert binary == 0. and av == 0. and not scores.any()


def test_F1_equals_the_reference_doubles(g):
    assert eval_utils.binary_F1_score(g['f1_bin_pred'], g['f1_bin_lab']) == float(g['f1_bin'])
    assert eval_utils.binary_F1_score(np.zeros((30, 28), np.uint8), np.zeros((30, 28), np.uint8)) == float(g['f1_bin_zero']) == 0.
    scores, av = eval_utils.multi_F1_score(g['f1_multi_pred'], g['f1_multi_lab'], 3)
    assert scores[1] == 0. and g['f1_multi_scores'][1] == 0.          # the class without support
    np.testing.assert_allclose(scores, g['f1_multi_scores'], rtol=0, atol=2e-16)      # scikit-learn's rounding of the same quotient
    assert abs(av - float(g['f1_multi_av'])) <= 2e-16
    M = eval_utils.confusion_matrix(g['f1_multi_pred'], g['f1_multi_lab'], 3)
    assert eval_utils.F1_from_confusion(M, 3)[2] == av


# ------------------------------------------------------------------------------------------------ confusion_counts_host
@pytest.mark.parametrize('pattern', ['whole', 'per sample', 'per slice', 'packed', 'offset'])
def test_confusion_counts_host_equals_loops(pattern):
    rs = np.random.RandomState(77)
    n, C = 60, 3
    inner, groups, first = {'whole': (n, 1, 0), 'per sample': (20, 3, 0), 'per slice': (1, 7, 0), 'packed': (12, 5, 0),
                            'offset': (4, 3, 11)}[pattern]
    pred = rs.randint(0, C, size=n)
    lab = rs.randint(0, C, size=n)
    lab[rs.rand(n) < 0.15] = -1
    pred[rs.rand(n) < 0.05] = C
    for fill in (-1, 0, C - 1, C):
        want, skipped = ec.confusion_loops(pred, lab, C, inner, groups, first, fill)
        got, got_skipped = eval_utils.confusion_counts_host(pred, lab, C, inner=inner, groups=groups, first=first, fill=fill,
                                                            want_skipped=True)
        assert got.dtype == np.int64 and got.shape == (groups, C, C)
        np.testing.assert_array_equal(got, want)
        assert got_skipped == skipped and want.sum() + skipped == n
        np.testing.assert_array_equal(ec.confusion_numpy(pred, lab, C, inner, groups, first, fill)[0], want)
    if pattern == 'whole':
        np.testing.assert_array_equal(eval_utils.confusion_counts_host(pred, lab, C)[0], eval_utils.confusion_matrix(pred, lab, C))


def test_chunked_host_calls_equal_one():
    rs = np.random.RandomState(78)
    pred, lab = rs.randint(0, 4, size=50), rs.randint(0, 4, size=50)
    whole = eval_utils.confusion_counts_host(pred, lab, 4, inner=3, groups=5)
    parts = sum(eval_utils.confusion_counts_host(pred[a:b], lab[a:b], 4, inner=3, groups=5, first=a) for a, b in ((0, 17), (17, 18), (18, 50)))
    np.testing.assert_array_equal(parts, whole)


# ------------------------------------------------------------------------------------------------ lesions, host statement
def test_lesion_host_statement_against_the_reference(g):
    mask = g['lesion_mask']
    got = lesion_utils.find_lesion_components_host(mask)
    assert got.dtype == np.float64
    assert ec.assert_ranks_match_reference(got, g['lesion_ranks']) == int(g['lesion_unique_volumes']) >= 5
    np.testing.assert_array_equal(got, ec.stable_ranks(mask))          # the tie rule, exactly
    for thr in g['lesion_thresholds']:
        drop = lesion_utils.drop_lesions_with_threshold_host(mask, int(thr))
        assert drop.dtype == np.uint8
        np.testing.assert_array_equal(drop, g['lesion_drop_%d' % thr])
        np.testing.assert_array_equal(drop, ec.stable_drop(mask, int(thr)))


def test_lesion_host_statement_with_the_origin_set():
    """mask[0, 0, 0] != 0: the origin's component is the background and the zero set a ranked "lesion"."""
    mask = np.zeros((4, 5, 6), dtype=np.uint8)
    mask[0, 0, 0:2] = 1                  # the origin's component: 2 voxels, ranked nowhere
    mask[2, 2, 1:4] = 1                  # 3 voxels
    mask[3, 4, 5] = 1                    # 1 voxel
    got = lesion_utils.find_lesion_components_host(mask)
    want = np.where(mask == 0, 1., 0.)   # the zero set, 114 voxels, is the largest
    want[2, 2, 1:4] = 2
    want[3, 4, 5] = 3
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(lesion_utils.drop_lesions_with_threshold_host(mask, 2), (want > 0) & (want < 3))
    np.testing.assert_array_equal(lesion_utils.drop_lesions_with_threshold_host(mask, 4), mask == 0)
    # a tie between the zero set and a component: label 0 comes first
    tie = np.array([1, 0, 0, 1, 1], dtype=np.uint8).reshape(1, 1, 5)
    np.testing.assert_array_equal(lesion_utils.find_lesion_components_host(tie).reshape(-1), [0, 1, 1, 2, 2])


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_and_listed():
    hdr = open(os.path.join(ROOT, 'include', 'alq.h')).read()
    for sym in ('alq_confusion_counts', 'alq_confusion_window', 'alq_cc_sizes', 'alq_cc_relabel'):
        assert re.search(r'\b%s\(' % sym, hdr) and sym in _lib.exported_names(), sym
    assert re.search(r'enum \{ ALQ_IDS_U8 = 0, ALQ_IDS_I32 = 1, ALQ_IDS_I64 = 2 \};', hdr)
    assert re.search(r'int alq_confusion_counts\(alq_ctx \*ctx, const void \*d_pred, int pred_type, const void \*d_lab, int lab_type,\s+'
                     r'int64_t n, int64_t first,\s+int64_t inner, int64_t groups, int C, int fill, int64_t \*d_counts, int64_t \*d_skipped\);', hdr)
    _lib.build()
    L = _lib.lib()
    assert L.alq_confusion_window(0) == 0 and L.alq_confusion_window(17) == 0
    for C in range(1, 17):
        w = L.alq_confusion_window(C)
        assert w >= 1 and w * C * C <= 8192 < (w + 1) * C * C          # as many groups as the histogram holds
    assert L.alq_confusion_window(16) == 32 and L.alq_confusion_window(3) == 910


# ------------------------------------------------------------------------------------------------ the plain ports
class _Handle(object):
    def __init__(self, name):
        self.name = name


class _StubModel(object):
    def __init__(self, dropout_rate):
        self.dropout_rate = dropout_rate
        self.x, self.keep_prob, self.prediction = _Handle('x'), _Handle('keep_prob'), _Handle('prediction')


class _StubSession(object):
    def __init__(self, model):
        self.model, self.feeds = model, []

    def run(self, fetch, feed_dict=None):
        assert fetch is self.model.prediction
        self.feeds.append(dict(feed_dict))
        return np.argmax(feed_dict[self.model.x], axis=0)


@pytest.mark.parametrize('dropout_rate', [None, 0.5])
def test_simple_eval_model(dropout_rate):
    rs = np.random.RandomState(5)
    model = _StubModel(dropout_rate)
    sess = _StubSession(model)
    batches = []
    for b in (4, 3, 5):
        X = rs.rand(3, b)
        Y = np.zeros((3, b))
        Y[rs.randint(0, 3, size=b), np.arange(b)] = 1          # class scores along the first axis, as the reference reads them
        batches.append((X, Y, None))
    acc, preds = eval_utils.simple_eval_model(model, sess, batches)
    want_p = np.concatenate([np.argmax(X, axis=0) for X, _, _ in batches])
    want_t = np.concatenate([np.argmax(Y, axis=0) for _, Y, _ in batches])
    np.testing.assert_array_equal(preds, want_p)
    assert acc == np.sum(want_p == want_t) / 12
    assert all((model.keep_prob in f) == (dropout_rate is not None) for f in sess.feeds)
    assert all(f[model.keep_prob] == 1. for f in sess.feeds if model.keep_prob in f)


def test_models_dict_for_different_sizes():
    class Dat(object):
        mods = ['T1', 'T2']
        img_addrs = {'T1': ['a', 'b', 'c', 'd'], 'T2': ['x'] * 4}
        table = {'a': np.zeros((12, 10, 6)), 'b': np.zeros((9, 11, 8)), 'c': np.zeros((12, 10, 7)), 'd': np.zeros((9, 11, 3))}

        def reader(self, path):
            return self.table[path]

    class WithOps(object):
        def __init__(self, shape, name):
            self.shape, self.name, self.assigned = shape, name, 0

        def add_assign_ops(self):
            self.assigned += 1

    built = []

    def builder(shape, name):
        built.append((shape, name))
        return WithOps(shape, name) if shape[0] == 12 else object()

    d = eval_utils.models_dict_for_different_sizes(builder, Dat())
    assert sorted(d) == ['(12, 10)', '(9, 11)'] and sorted(built) == [([9, 11], '9x11'), ([12, 10], '12x10')]
    assert d['(12, 10)'].assigned == 1 and not hasattr(d['(9, 11)'], 'add_assign_ops')
    assert '{}'.format(Dat.table['a'].shape[:2]) in d          # the key get_full_segs looks up
