"""Host side of partial fine-tuning: the exported symbols of the fused diagonal Fisher and the masks, and the NumPy mask
functions of model_utils (model_utils.py:54-96)."""
import numpy as np
import pytest


def test_new_symbols_are_exported():
    from nnal_amd import _lib
    names = _lib.exported_names()
    for sym in ('alq_diag_fisher', 'alq_topk_mask', 'alq_topk_mask_work_bytes', 'alq_threshold_mask'):
        assert sym in names, sym


def _lov():
    rs = np.random.RandomState(3)
    LoV = [np.abs(rs.randn(3, 3, 2, 4)), np.abs(rs.randn(4)), np.abs(rs.randn(5, 7))]
    # planted duplicates: inside one variable, across variables, and a run of equal values at the top
    LoV[0][0, 1, 1, 2] = LoV[0][2, 0, 0, 1] = LoV[2][3, 3] = 0.75
    LoV[1][1] = LoV[1][3] = LoV[2][0, 0] = LoV[0][1, 1, 0, 0] = 9.0
    LoV[2][4, :] = 0.0
    return LoV


@pytest.mark.parametrize('k', [0, 1, 2, 3, 5, 40, 111])
def test_keep_k_largest_from_LoV(k):
    from nnal_amd import model_utils
    LoV = _lov()
    flat = np.concatenate([v.ravel() for v in LoV])
    total = flat.size
    assert total == 72 + 4 + 35
    bmask, locs = model_utils.keep_k_largest_from_LoV(LoV, k)
    assert len(bmask) == 3 and all(m.shape == v.shape for m, v in zip(bmask, LoV))
    fm = np.concatenate([m.ravel() for m in bmask])
    assert set(np.unique(fm)) <= {0.0, 1.0}
    assert int(fm.sum()) == k
    want = np.zeros(total)
    want[np.argsort(-flat, kind='stable')[:k]] = 1
    np.testing.assert_array_equal(fm, want)
    np.testing.assert_array_equal(locs, [i for i, m in enumerate(bmask) if m.any()])
    if k == total:
        assert fm.all()
    if k == 3:      # four entries tie at the top value: the three of lowest flat index are taken
        assert bmask[0][1, 1, 0, 0] == 1 and bmask[1][1] == 1 and bmask[1][3] == 1 and bmask[2][0, 0] == 0


def test_keep_k_largest_rejects_bad_k():
    from nnal_amd import model_utils
    with pytest.raises(ValueError):
        model_utils.keep_k_largest_from_LoV(_lov(), 112)
    with pytest.raises(ValueError):
        model_utils.keep_k_largest_from_LoV(_lov(), -1)


def test_threshold_LoV():
    from nnal_amd import model_utils
    LoV = _lov()
    for thr in (0.75, 9.0, 0.0, 0.3, 10.0):
        bmask = model_utils.threshold_LoV(LoV, thr)
        for m, v in zip(bmask, LoV):
            assert m.shape == v.shape
            np.testing.assert_array_equal(m, (v >= thr).astype(np.float64))
