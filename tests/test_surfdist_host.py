"""nnal_amd.surfdist without a GPU: the NumPy statement of the surface-distance calls against brute force, scipy and closed
forms; nrrd_io.voxel_spacing; eval_utils.eval_full_segs_surface_distances without a session."""
import os

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial.distance import cdist

import nnal_amd  # noqa: F401
from nnal_amd import eval_utils, nrrd_io, surfdist

EPS = 2.0 ** -52
SPACINGS = [(1., 1., 1.), (0.7, 0.9, 2.2), (1.3, 1.3, 1.3), (0.5, 0.5, 3.)]


def _blobs(shape, seed, p=0.03, grow=2):
    rng = np.random.RandomState(seed)
    a = rng.rand(*shape) < p
    return ndimage.binary_dilation(a, iterations=grow) if grow else a


@pytest.mark.parametrize('spacing', SPACINGS)
def test_edt_is_the_brute_force_minimum_bit_for_bit(spacing):
    for shape, seed in (((13, 9, 17), 1), ((12, 11, 7), 2), ((1, 20, 33), 3), ((9, 14), 4), ((40, 37, 21), 5)):
        feat = np.random.RandomState(seed).rand(*shape) < (0.03 if seed < 5 else 0.005)
        feat.flat[seed] = True
        got = surfdist.edt_sq_host(feat, spacing[:len(shape)])
        np.testing.assert_array_equal(got, surfdist.edt_sq_brute(feat, spacing[:len(shape)]))
        assert got.shape == shape and got.dtype == np.float64
    np.testing.assert_array_equal(surfdist.edt_sq_host(np.zeros((3, 4, 5)), spacing), np.full((3, 4, 5), np.inf))


@pytest.mark.parametrize('spacing', SPACINGS)
def test_edt_against_scipy(spacing):
    """Within 8 * 2^-52 * d2: at most 3 roundings in scipy's sum, its square root, and the squaring here."""
    feat = np.random.RandomState(7).rand(40, 37, 21) < 0.01
    got = surfdist.edt_sq_host(feat, spacing)
    want = ndimage.distance_transform_edt(~feat, sampling=spacing) ** 2
    err = np.abs(got - want)
    bound = 8 * EPS * want
    print('worst error / bound: %.3f' % np.max(err[want > 0] / bound[want > 0]))
    assert np.all(err <= bound)


@pytest.mark.parametrize('shape', [(9, 8, 7), (9, 8, 1), (9, 1, 7), (1, 8, 7), (9, 1, 1), (1, 1, 7), (1, 8, 1), (9, 8)])
def test_surface_is_mask_minus_erosion(shape):
    for seed, label in ((0, None), (1, None), (2, 2), (3, -1)):
        rng = np.random.RandomState(seed)
        seg = (rng.rand(*shape) < 0.7).astype(np.uint8) * rng.randint(1, 4, size=shape).astype(np.uint8)
        fg = (seg != 0) if (label is None or label < 0) else (seg == label)
        sq = np.squeeze(fg)
        want = sq & ~ndimage.binary_erosion(sq, ndimage.generate_binary_structure(sq.ndim, 1), border_value=0)
        np.testing.assert_array_equal(np.squeeze(surfdist.surface_host(seg, label)), want)
    full = np.ones(shape, dtype=np.uint8)
    s = surfdist.surface_host(full)
    inner = tuple(slice(1, -1) if n > 1 else slice(None) for n in shape)
    want = np.ones(shape, dtype=bool)
    want[inner] = False
    np.testing.assert_array_equal(s, want)
    assert not surfdist.surface_host(np.ones((1, 1, 1))).any()


def test_select_and_stats_statements():
    rng = np.random.RandomState(5)
    d2 = np.concatenate([rng.rand(50), [0., np.inf, 5e-324, 1e300], np.full(9, 0.25)])
    mask = rng.rand(d2.size) < 0.6
    mask[50:] = True
    v = np.sort(d2[mask])
    ranks = [0, v.size - 1, v.size // 2, v.size, v.size + 5]
    got = surfdist.select_host(d2, mask, ranks)
    np.testing.assert_array_equal(got[:3], v[[0, v.size - 1, v.size // 2]])
    assert np.isnan(got[3]) and np.isnan(got[4])
    st = surfdist.dist_stats_host(d2, mask)
    assert st[0] == v.size and st[1] == np.inf and st[2] == np.inf and st[3] == 0.
    np.testing.assert_array_equal(surfdist.dist_stats_host(d2, np.zeros(d2.size)), [0., 0., -np.inf, np.inf])


@pytest.mark.parametrize('q', [0., 50., 95., 97.5, 100.])
@pytest.mark.parametrize('n', [1, 2, 7, 100])
def test_interpolated_percentile_against_numpy(n, q):
    """Within 8 * 2^-52 * hi of np.percentile: the two lerp formulas round at most 3 times each."""
    d2 = np.random.RandomState(n).rand(n) * 100.
    mask = np.ones(n, dtype=bool)
    lo, hi, frac = surfdist.percentile_ranks(n, q)
    sel = surfdist.select_host(d2, mask, [lo, hi])
    got = surfdist.interp_percentile(sel[0], sel[1], frac)
    want = np.percentile(np.sqrt(d2), q)
    assert abs(got - want) <= 8 * EPS * np.sqrt(sel[1])


def test_voxel_spacing_header_forms(tmp_path):
    assert nrrd_io.voxel_spacing({'dimension': 3, 'spacings': '1 0.5 2.5'}) == (1., 0.5, 2.5)
    assert nrrd_io.voxel_spacing({'dimension': 3, 'spacings': 'nan 0.5 2.5'}) == (1., 0.5, 2.5)
    got = nrrd_io.voxel_spacing({'dimension': 3, 'space directions': '(0.6,0,0.8) (0,2,0) (0,0,2.5)'})
    assert got == (1., 2., 2.5)
    assert nrrd_io.voxel_spacing({'dimension': 4, 'space directions': 'none (3,0,0) (0,4,0) (0,0,5)'}) == (1., 3., 4., 5.)
    assert nrrd_io.voxel_spacing({'dimension': 3}) == (1., 1., 1.)
    assert nrrd_io.voxel_spacing({'dimension': 3, 'space directions': [[1, 0, 0], [0, 3, 4], [0, 0, 2]]}) == (1., 5., 2.)
    path = str(tmp_path / 'v.nrrd')
    nrrd_io.write(path, np.zeros((2, 3, 4), dtype=np.uint8), fields={'spacings': '0.5 0.5 3'})
    data, header = nrrd_io.read(path)
    assert data.shape == (2, 3, 4) and nrrd_io.voxel_spacing(header) == (0.5, 0.5, 3.)


def _box(shape, lo, size):
    a = np.zeros(shape, dtype=np.uint8)
    a[tuple(slice(l, l + size) for l in lo)] = 1
    return a


def test_metric_closed_forms():
    a = _box((12, 10, 9), (2, 3, 2), 4)
    res = surfdist.surface_distances(a, a)
    assert all(res[k] == 0. for k in ('HD', 'HD95', 'ASSD', 'MHD')) and res['n_seg'] == res['n_mask'] == 56
    b = _box((12, 10, 9), (5, 3, 2), 4)
    res = surfdist.surface_distances(a, b, spacing=(2., 1., 1.))
    assert res['HD'] == 6.0 and res['max_seg_to_mask'] == 6.0 and res['max_mask_to_seg'] == 6.0
    assert 0 < res['ASSD'] <= res['MHD'] <= res['HD95'] <= res['HD']
    e = np.zeros_like(a)
    for x, y in ((a, e), (e, a)):
        res = surfdist.surface_distances(x, y)
        assert all(res[k] == np.inf for k in ('HD', 'HD95', 'ASSD', 'MHD'))
    res = surfdist.surface_distances(e, e)
    assert all(res[k] == 0. for k in ('HD', 'HD95', 'ASSD', 'MHD')) and res['n_seg'] == 0
    # an image is a one-slice volume, a 2-entry spacing is padded
    r2 = surfdist.surface_distances(a[:, :, 3], b[:, :, 3], spacing=(2., 1.))
    r3 = surfdist.surface_distances(a[:, :, 3:4], b[:, :, 3:4], spacing=(2., 1., 7.))
    assert r2 == r3 and r2['HD'] == 6.0


@pytest.mark.parametrize('spacing', SPACINGS)
def test_metrics_against_point_sets(spacing):
    seg, mask = _blobs((20, 18, 11), 11), _blobs((20, 18, 11), 12)
    res = surfdist.surface_distances(seg, mask, spacing)
    pa = np.argwhere(surfdist.surface_host(seg)) * np.asarray(spacing)
    pb = np.argwhere(surfdist.surface_host(mask)) * np.asarray(spacing)
    D = cdist(pa, pb)
    dab, dba = D.min(axis=1), D.min(axis=0)
    hd = max(dab.max(), dba.max())
    assert abs(res['HD'] - hd) <= 4 * EPS * hd
    assert res['n_seg'] == len(pa) and res['n_mask'] == len(pb)
    tol = 1e-12
    assert abs(res['ASSD'] - (dab.sum() + dba.sum()) / (len(pa) + len(pb))) <= tol * hd
    assert abs(res['MHD'] - max(dab.mean(), dba.mean())) <= tol * hd
    assert abs(res['HD95'] - max(np.percentile(dab, 95), np.percentile(dba, 95))) <= tol * hd


def test_eval_full_segs_surface_distances_on_arrays_and_files(tmp_path):
    rng = np.random.RandomState(3)
    segs, masks = [], []
    for i in range(3):
        m = _blobs((14, 12, 9), 20 + i).astype(np.uint8) * rng.randint(1, 3, size=(14, 12, 9)).astype(np.uint8)
        s = m.copy()
        s[rng.rand(*s.shape) < 0.05] = 1
        segs.append(s)
        masks.append(m)
    res = eval_utils.eval_full_segs_surface_distances(segs, masks)
    assert sorted(k for k in res if k.isupper()) == ['ASSD', 'HD', 'HD95', 'MHD'] and res['HD'].shape == (3,)
    for i in range(3):
        one = surfdist.surface_distances(segs[i], masks[i])
        for k, v in one.items():
            assert res[k][i] == v, k
    resl = eval_utils.eval_full_segs_surface_distances(segs, masks, spacings=(0.5, 0.5, 3.), labels=[1, 2], percentile=90.)
    assert resl['HD'].shape == (3, 2) and resl['n_seg'].dtype == np.int64
    for i in range(3):
        for j, lab in enumerate((1, 2)):
            one = surfdist.surface_distances(segs[i], masks[i], (0.5, 0.5, 3.), lab, 90.)
            for k, v in one.items():
                assert resl[k][i, j] == v, k
    # files: the spacing of each mask file is read from its header
    sp, mp = [], []
    for i in range(3):
        sp.append(str(tmp_path / ('seg_%d.nrrd' % i)))
        mp.append(str(tmp_path / ('mask_%d.nrrd' % i)))
        nrrd_io.write(sp[-1], segs[i])
        nrrd_io.write(mp[-1], masks[i], fields={'spacings': '0.5 0.5 %d' % (i + 1)} if i else None)
    resf = eval_utils.eval_full_segs_surface_distances(sp, mp)
    for i in range(3):
        one = surfdist.surface_distances(segs[i], masks[i], (0.5, 0.5, i + 1.) if i else (1., 1., 1.))
        for k, v in one.items():
            assert resf[k][i] == v, k
    assert os.path.exists(sp[0])
