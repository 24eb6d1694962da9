"""Host side of the region strategies (`ps-random`, super-pixels): the NumPy restatements of nnal_amd.regions against scipy, a
plain loop and the reference's own outputs (tests/golden/r9_regions.npz, make_golden_r9.py), the precondition of the variance
map and PW_AL.get_SuPix_inds.  No GPU."""
import os

import numpy as np
import pytest

import nnal_amd  # noqa: F401
from nnal_amd import PW_AL, regions


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'r9_regions.npz'))


def _scipy_vars_2d(img, d):
    """patch_utils.get_vars_2d (patch_utils.py:794-826), written out."""
    from scipy.signal import convolve2d
    img = np.uint64(img)
    kernel = np.ones((d, d))
    Ex = convolve2d(img, kernel, 'same') / float(d ** 2)
    ExP2 = convolve2d(img ** 2, kernel, 'same') / float(d ** 2)
    return ExP2 - Ex ** 2


@pytest.mark.parametrize('d', [1, 2, 5, 12, 13, 33])
def test_local_var2d_host_equals_scipy(d):
    rs = np.random.RandomState(100 + d)
    img = rs.randint(0, 4096, size=(19, 23)) + rs.rand(19, 23)
    np.testing.assert_array_equal(regions.local_var2d_host(img, d), _scipy_vars_2d(img, d))
    np.testing.assert_array_equal(regions.local_var2d_host(img.astype(np.float32), d), _scipy_vars_2d(img.astype(np.float32), d))


def test_local_var2d_host_volume_is_slice_by_slice():
    rs = np.random.RandomState(7)
    r = (2, 3, 1)
    vol = np.pad(rs.randint(0, 300, size=(11, 9, 4)) + rs.rand(11, 9, 4), [(a, a) for a in r], 'constant')
    got = regions.local_var2d_host(vol, 4, r)
    assert got.shape == (11, 9, 4)
    for z in range(4):
        np.testing.assert_array_equal(got[:, :, z], _scipy_vars_2d(vol[2:-2, 3:-3, 1 + z], 4))


def test_segment_min_host_against_loop():
    rs = np.random.RandomState(8)
    shape = (17, 13, 9)
    seg = rs.randint(0, 41, size=shape)
    seg[:, :, 2][seg[:, :, 2] > 10] = 0
    inds = rs.permutation(int(np.prod(shape)))[:900]
    inds = inds[(inds % 9 != 4) & (inds % 9 != 6)]
    scores = np.round(rs.rand(len(inds)), 1)
    scores[:5] = 0.
    scores[5:9] = 5e-324
    got = regions.segment_min_host(seg, inds, scores)
    want = np.full((9, 41), np.inf)
    ii, jj, zz = np.unravel_index(inds, shape)
    for z in range(9):
        for l in range(1, 41):
            m = (zz == z) & (seg[ii, jj, zz] == l)
            if m.any():
                want[z, l] = scores[m].min()
    np.testing.assert_array_equal(got, want)
    assert np.all(np.isinf(got[[4, 6]])) and np.all(np.isinf(got[:, 0]))
    # labels at or above n_labels are skipped
    np.testing.assert_array_equal(regions.segment_min_host(seg, inds, scores, 12), want[:, :12])


def test_golden_get_vars_2d(gold):
    vol = gold['vol'].astype(np.float64)
    for d in gold['gv_d']:
        want = gold['gv_var_%d' % d]
        for s_, z in enumerate(gold['gv_slices']):
            np.testing.assert_array_equal(regions.local_var2d_host(vol[:, :, z], int(d)), want[:, :, s_])


def test_golden_get_HV_inds_and_partition_restated(gold):
    """The reference's get_HV_inds / partition_2d_indices from the restated map (the device versions: tests/test_gpu_regions.py)."""
    vol = gold['vol'].astype(np.float64)
    pool = gold['hv_pool']
    for tag in 'ab':
        pshape = gold['hv_pshape_' + tag]
        d = int((pshape[0] - 1) / 2)
        vmap = regions.local_var2d_host(vol, d)
        np.testing.assert_array_equal(np.nonzero(vmap.reshape(-1)[pool] > 2.)[0], gold['hv_valid_' + tag])
    v = regions.local_var2d_host(vol[:, :, int(gold['part_slice'])], 5)
    v[v == 0] += 1e-1
    v = np.log(v).reshape(-1)
    masked = gold['part_mask'].reshape(-1) > 0
    np.testing.assert_array_equal(np.nonzero(masked)[0], gold['part_masked'])
    np.testing.assert_array_equal(np.nonzero((v > 2.) & ~masked)[0], gold['part_hvar'])
    np.testing.assert_array_equal(np.nonzero((v < 2.) & ~masked)[0], gold['part_lvar'])
    assert len(gold['part_hvar']) > 50 and len(gold['part_lvar']) > 50


def test_golden_superpix_scoring_and_SuPix_inds(gold):
    """PW_NNAL.superpix_scoring ran in the generator on a NumPy stand-in for skimage's regionprops (make_golden_r9.py)."""
    seg = gold['sp_seg'].astype(np.int64)
    table = regions.segment_min_host(seg, gold['sp_inds'], gold['sp_scores'])
    np.testing.assert_array_equal(table, gold['sp_table'])
    assert np.isinf(table).any() and np.isfinite(table).any()
    lists = PW_AL.get_SuPix_inds(seg, gold['sp_codes'])
    assert [len(l) for l in lists] == list(gold['sp_lens'])
    np.testing.assert_array_equal(np.concatenate(lists), gold['sp_vox'])
    with pytest.raises(ValueError):
        PW_AL.get_SuPix_inds(seg, np.array([[0], [200]]))


@pytest.mark.parametrize('bad', ['negative', 'nan', 'inf', 'range'])
def test_variance_precondition(bad):
    img = np.full((6, 5), 3.)
    d = 5
    if bad == 'negative':
        img[2, 2] = -1.
    elif bad == 'nan':
        img[0, 0] = np.nan
    elif bad == 'inf':
        img[0, 0] = np.inf
    else:
        img[1, 1] = 2. ** 26          # (2^26)^2 * 25 >= 2^53
    with pytest.raises(ValueError):
        regions.check_variance_input(img, d)
    ok = np.full((6, 5), 2. ** 24)    # 2^48 * 25 < 2^53
    regions.check_variance_input(ok, d)
    regions.check_variance_input(ok.astype(np.int64), d)
    for dd in (0, 66):
        with pytest.raises(ValueError):
            regions.check_variance_input(ok, dd)
