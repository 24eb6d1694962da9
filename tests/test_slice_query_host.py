"""Host side of the slice queries (nnal_amd.slice_query; no GPU): the NumPy restatement of the two kernels against values known by
hand, the bookkeeping of the query on made-up score tables, and the refusals that are decided before any device call."""
import numpy as np
import pytest

from tests import slice_query_ref as ref


def _sq():
    import nnal_amd  # noqa: F401
    from nnal_amd import slice_query
    return slice_query


def test_one_hot_posteriors_score_exactly_zero():
    sq = _sq()
    rs = np.random.RandomState(1)
    P = ref.one_hot(rs, T=3, c=4, n=5, V=17)
    for kind in ('entropy', 'MC-entropy'):
        sums, counts, mag = sq.slice_scores_host(P[:1] if kind == 'entropy' else np.repeat(P[:1], 3, axis=0), kind)
        assert np.all(sums == 0.) and np.all(mag == 0.) and np.all(counts == 17)
    sums, _, _ = sq.slice_scores_host(np.repeat(P[:1], 3, axis=0), 'BALD')
    assert np.all(sums == 0.)


@pytest.mark.parametrize('c', [2, 3, 8])
def test_uniform_posteriors_score_n_log_c(c):
    sq = _sq()
    n, V = 4, 29
    P = np.full((2, c, n, V), 1. / c, dtype=np.float32)
    roi = np.zeros((n, V), dtype=np.uint8)
    roi[0, :] = 1
    roi[1, :7] = 3
    roi[3, 11] = 255
    cnt = np.array([V, 7, 0, 1])
    want = cnt * np.log(c)
    # the fp64 rounding of cnt * c terms, and 1 / c in fp32: p = (1 + d) / c gives -c p log p = (1 + d) (log c - log(1 + d))
    d = abs(c * np.float64(np.float32(1. / c)) - 1.)
    slack = ref.bound(cnt * c, want) + cnt * d * (1 + np.log(c))
    for kind in ('entropy', 'MC-entropy'):
        sums, counts, mag = sq.slice_scores_host(P, kind, roi=roi)
        assert np.array_equal(counts, [V, 7, 0, 1]) and counts.dtype == np.int64
        assert np.all(np.abs(sums - want) <= slack), (sums, want)
        assert sums[2] == 0. and mag[2] == 0.
        assert np.all(np.abs(mag - want) <= slack)          # every term of h has one sign here


def test_bald_of_identical_passes_is_zero_and_jensen_holds():
    sq = _sq()
    rs = np.random.RandomState(5)
    one = ref.softmax_posteriors(rs, 1, 3, 6, 41, 3.)
    sums, _, mag = sq.slice_scores_host(np.repeat(one, 1, axis=0), 'BALD')
    assert np.all(sums == 0.)          # T = 1: h(p / 1) - h(p) / 1, the same doubles
    sums, _, mag = sq.slice_scores_host(np.repeat(one, 4, axis=0), 'BALD')
    assert np.all(np.abs(sums) <= ref.bound(41 * (3 * 4 + 3), mag))
    for scale in (0.1, 3., 30.):
        P = ref.softmax_posteriors(rs, 10, 3, 6, 41, scale)
        sums, counts, mag = sq.slice_scores_host(P, 'BALD')
        assert np.all(sums >= -ref.bound(41 * (3 * 10 + 3), mag)), sums          # Jensen: h(mean) >= mean h
        assert np.all(counts == 41)
    assert sums.max() > 0.


def test_mean_kind_and_unknown_kind():
    sq = _sq()
    au = np.arange(12, dtype=np.float32).reshape(3, 4) - 5
    roi = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]])
    sums, counts, mag = sq.slice_scores_host(None, 'AU', roi=roi, au=au)
    assert np.array_equal(sums, [-5 + -3, 0, 3 + 4 + 5 + 6]) and np.array_equal(counts, [2, 0, 4]) and np.array_equal(mag, [8, 0, 18])
    with pytest.raises(ValueError):
        sq.slice_scores_host(au[None, None], 'variance')
    m, n = sq.mean_scores(sums, counts)
    assert np.array_equal(m, [-4., -np.inf, 4.5]) and n.dtype == np.int64


def test_pick_slices_ties_empty_slices_and_split():
    sq = _sq()
    scores = [np.array([0.5, 0.9, 0.5, 0.1]), np.array([]), np.array([0.9, 7., 0.5]), np.array([-np.inf, 0.2])]
    counts = [np.array([3, 3, 3, 3]), np.array([], dtype=int), np.array([1, 0, 2]), np.array([0, 5])]
    got = sq.pick_slices(scores, counts, 4)
    # 0.9 of subject 0 before 0.9 of subject 2; then the three 0.5: the lower (subject, slice) first; the 7. has no ROI voxel
    assert [g.tolist() for g in got] == [[0, 1, 2], [], [0], []]
    assert all(g.dtype == np.int64 for g in got)
    got = sq.pick_slices(scores, counts, 7)
    assert [g.tolist() for g in got] == [[0, 1, 2, 3], [], [0, 2], [1]]
    assert [g.tolist() for g in sq.pick_slices(scores, counts, 0)] == [[], [], [], []]
    with pytest.raises(ValueError):
        sq.pick_slices(scores, counts, 8)          # only 7 slices hold a ROI voxel
    with pytest.raises(ValueError):
        sq.pick_slices(scores, counts, 10)         # more than the pool


class _Dat(object):
    def __init__(self, depths, labelled):
        self.L_indic = np.array([1] * labelled + [0] * (len(depths) - labelled))
        self.tr_imgs = [[np.zeros((2, 2, z)), np.zeros((2, 2, z))] for z in depths]


def test_random_query_launches_nothing_and_k_too_large():
    sq = _sq()
    dat = _Dat([5, 3, 4, 6], labelled=1)
    np.random.seed(3)
    got = sq.query_slices(None, None, dat, 'random', 6)
    np.random.seed(3)
    want = np.sort(np.random.permutation(13)[:6])
    assert len(got) == 3 and sum(len(g) for g in got) == 6
    assert np.array_equal(np.concatenate([g + off for g, off in zip(got, (0, 3, 7))]), want)
    assert all(np.all(np.diff(g) > 0) for g in got)
    for method in ('random', 'entropy'):
        with pytest.raises(ValueError):
            sq.query_slices(None, None, dat, method, 14)


class _Model(object):
    dense, AU_4U, dropout_layers = True, False, []


def test_refusals_before_any_device_call():
    sq = _sq()
    vol = np.zeros((4, 4, 3), np.float32)
    fc = _Model()
    fc.dense = False
    for method in ('entropy', 'BALD', 'AU'):
        with pytest.raises(NotImplementedError):
            sq.slice_scores(fc, None, vol, method)
    with pytest.raises(NotImplementedError):
        sq.slice_scores(_Model(), None, vol, 'AU')
    for method in ('MC-entropy', 'BALD'):
        with pytest.raises(ValueError):
            sq.slice_scores(_Model(), None, vol, method)
    for m in (fc, _Model()):
        with pytest.raises(ValueError):
            sq.slice_scores(m, None, vol, 'margin')
    with pytest.raises(ValueError):
        sq.query_slices(_Model(), None, _Dat([3, 3], 1), 'margin', 1)


def test_symbols_are_declared():
    import nnal_amd  # noqa: F401
    from nnal_amd import _lib
    for name in ('alq_unc_accumulate', 'alq_slice_scores', 'alq_slice_scores_geometry'):
        assert name in _lib.exported_names()
