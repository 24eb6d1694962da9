"""nnal_amd/slic.py, the NumPy statement of the SLIC over-segmentation (csrc/slic.hip equals it byte for byte: tests/test_gpu_slic.py):
against a plain-loop restatement at tiny sizes, its properties (a) to (e), and the situations the connectivity step exists for.
No GPU."""
import numpy as np
import pytest
from scipy import ndimage

import nnal_amd  # noqa: F401
from nnal_amd import regions, slic
from tests import slic_cases

CASES = slic_cases.cases()
_RESULTS = {}


def _run(name):
    if name not in _RESULTS:
        c = CASES[name]
        _RESULTS[name] = slic.slic_host(c['vol'], c['gh'], c['gw'], c['w'], c['T'], c['min_size'], c['mask'])
    return _RESULTS[name]


def _in_mask(c):
    mods = slic.as_modalities(c['vol'])
    return slic.quantise(mods, *slic.quant_range(mods, c['mask']), mask=c['mask'])[1]


# ------------------------------------------------------------------------------------------------ the plain-loop restatement
@pytest.mark.parametrize('name', ['tie', 'pixel_cells', 'one_cell', 'pocket', 'checkerboard'])
def test_equals_plain_loops(name):
    c = CASES[name]
    want = slic_cases.naive_slic(c['vol'], c['gh'], c['gw'], c['w'], c['T'], c['min_size'], c['mask'])
    got = _run(name)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize('T, min_size, masked', [(0, 0, False), (1, 3, True), (3, 0, True), (2, 5, False), (2, 1000, True)])
def test_equals_plain_loops_9x11(T, min_size, masked):
    """9 x 11 with a 2 x 3 grid, two modalities, noise enough for orphans; with a mask and a NaN."""
    rs = np.random.RandomState(31 + T)
    vol = [(np.add.outer(np.arange(9) // 4, np.arange(11) // 3)[:, :, None] + 0.8 * rs.randn(9, 11, 2)).astype(np.float32) for _ in range(2)]
    mask = None
    if masked:
        mask = rs.rand(9, 11, 2) > 0.2
        vol[1][4, 4, 0] = np.nan
    got = slic.slic_host(vol, 2, 3, 0.5, T, min_size, mask)
    want = slic_cases.naive_slic(vol, 2, 3, 0.5, T, min_size, mask)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32


# ------------------------------------------------------------------------------------------------------------- the properties
def test_a_pure_function():
    c = CASES['mask_nan']
    vol = [v.copy() for v in c['vol']]
    first = slic.slic_host(vol, c['gh'], c['gw'], c['w'], c['T'], c['min_size'], c['mask'])
    for v, v0 in zip(vol, c['vol']):
        np.testing.assert_array_equal(v, v0)              # NaN == NaN here
    again = slic.slic_host(vol, c['gh'], c['gw'], c['w'], c['T'], c['min_size'], c['mask'], threads=3)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize('name', sorted(CASES))
def test_b_c_connected_and_numbered(name):
    labels, counts = _run(name)
    inn = _in_mask(CASES[name])
    np.testing.assert_array_equal(labels == 0, ~inn)                                  # 0 exactly on out pixels
    for z in range(labels.shape[2]):
        L = labels[:, :, z]
        present = np.unique(L[L > 0])
        np.testing.assert_array_equal(present, np.arange(1, counts[z] + 1))          # 1 .. n_z, no gaps
        flat = L.reshape(-1)
        firsts = [int(np.flatnonzero(flat == l)[0]) for l in present]
        assert firsts == sorted(firsts)                                              # ordered by first pixel
        for l in present:
            assert ndimage.label(L == l)[1] == 1                                     # one 4-connected set (default structure)


def _touching_sizes(L):
    """sizes of the regions of a slice that are 4-adjacent to another region."""
    touch = set()
    for a, b in ((L[:, :-1], L[:, 1:]), (L[:-1, :], L[1:, :])):
        sel = (a > 0) & (b > 0) & (a != b)
        touch.update(a[sel].tolist())
        touch.update(b[sel].tolist())
    sizes = np.bincount(L.reshape(-1))
    return [int(sizes[l]) for l in touch]


@pytest.mark.parametrize('name', ['min_size', 'm3', 'mask_nan', 'rounds', 'all_small', 'one_slice'])
def test_d_no_small_region_touches_another(name):
    labels, _ = _run(name)
    assert CASES[name]['min_size'] > 0
    for z in range(labels.shape[2]):
        assert all(s >= CASES[name]['min_size'] for s in _touching_sizes(labels[:, :, z]))


def test_d_needs_the_threshold():
    """The same subject without the threshold has touching regions below it: the property is the threshold's doing."""
    c = dict(CASES['min_size'], min_size=0)
    labels, _ = slic.slic_host(c['vol'], c['gh'], c['gw'], c['w'], c['T'], 0, c['mask'])
    assert any(s < CASES['min_size']['min_size'] for z in range(labels.shape[2]) for s in _touching_sizes(labels[:, :, z]))


@pytest.mark.parametrize('H, W, gh, gw', [(9, 11, 2, 3), (20, 28, 3, 4), (6, 9, 6, 3), (5, 7, 1, 1)])
@pytest.mark.parametrize('T', [1, 4])
def test_e_constant_image_gives_the_home_cells(H, W, gh, gw, T):
    labels, counts = slic.slic_host(np.full((H, W, 2), 7.0), gh, gw, slic.spatial_weight(0.1, H, W, gh, gw), T)
    home = ((np.arange(H) * gh) // H)[:, None] * gw + ((np.arange(W) * gw) // W)[None, :] + 1
    np.testing.assert_array_equal(labels, np.repeat(home[:, :, None], 2, axis=2))
    np.testing.assert_array_equal(counts, [gh * gw] * 2)


def test_e_fails_where_a_row_ties_between_two_start_rows():
    """H = 4, gh = 2: the start rows are 1 and 3 and row 2 (home cell 1) is equidistant from both; the tie goes to the lower
    cluster, as the rule says, so the regions are rows 0-2 and row 3.  Stated in slic.py's docstring; pinned here."""
    labels, counts = slic.slic_host(np.full((4, 3, 1), 7.0), 2, 1, 1.0, T=2)
    np.testing.assert_array_equal(labels[:, 0, 0], [1, 1, 1, 2])
    assert counts[0] == 2


# ---------------------------------------------------------------------------------------------------------------- situations
def test_two_intensities_never_share_a_region():
    """A bright box and a slanted half plane, neither aligned with the 3 x 4 grid.  Every pixel has a start pixel of its own
    intensity among its nine candidates, and with w = 1e-6 (spatial term below 1e-2, an intensity step is 65535^2) it never
    takes a cluster of the other intensity: clusters are pure, and a pure cluster's pixels are the nearest of their intensity, so
    whatever the connectivity step moves stays within one intensity here (asserted, not assumed)."""
    img = np.zeros((24, 30, 2), dtype=np.float32)
    img[3:19, 5:26, 0] = 1.0
    img[:, :, 1] = (np.arange(24)[:, None] * 0.4 + np.arange(30)[None, :]) > 17
    labels, counts = slic.slic_host(img, 3, 4, 1e-6, T=5)
    assert counts.min() >= 12
    for z in range(2):
        for l in range(1, counts[z] + 1):
            assert len(np.unique(img[:, :, z][labels[:, :, z] == l])) == 1


def test_checkerboard_has_orphans_and_they_are_adopted():
    lab, inn, st = slic_cases.slice_stats(CASES['checkerboard'])
    assert inn.all() and st['orphans'] > 0 and st['rounds'] >= 1 and st['unadopted'] == 0
    labels, counts = _run('checkerboard')
    assert counts[0] <= 4                                 # at most one region per cluster once every orphan has been adopted


def test_more_than_one_adoption_round():
    assert slic_cases.slice_stats(CASES['rounds'])[2]['rounds'] >= 2


def test_wall_isolates_an_orphan():
    lab, inn, st = slic_cases.slice_stats(CASES['pocket'])
    assert st['orphans'] == 1 and st['unadopted'] == 1 and st['rounds'] == 0
    labels, counts = _run('pocket')
    L = labels[:, :, 0]
    pocket = L[2:4, 2:4]
    assert len(np.unique(pocket)) == 1 and pocket[0, 0] > 0
    assert np.count_nonzero(L == pocket[0, 0]) == 4       # a region of its own: the pocket and nothing else
    assert np.all(L[1:5, 1:5][~CASES['pocket']['mask'][1:5, 1:5, 0]] == 0)
    assert counts[0] == 5                                 # four home cells + the pocket


def test_two_walled_orphans_that_touch_merge():
    """Step 3b: a pocket that straddles two home cells holds two orphans; they touch each other and nothing else, and merge."""
    mask = np.ones((12, 12, 1), dtype=bool)
    mask[4:8, 0:4] = False
    mask[5:7, 1:3] = True                                 # rows 5 and 6: home cells 0 and 1 of a 2 x 2 grid over 12 rows
    labels, counts = slic.slic_host(np.ones((12, 12, 1)), 2, 2, 1.0, T=0, mask=mask)
    assert len(np.unique(labels[5:7, 1:3, 0])) == 1 and counts[0] == 5


def test_nan_pixel_is_out():
    labels, counts = _run('nan_only')
    assert labels[3, 5, 0] == 0 and labels[10, 20, 1] == 0 and labels[19, 27, 2] == 0
    assert np.count_nonzero(labels == 0) == 3


def test_empty_cluster_keeps_its_centre():
    c = CASES['empty_cluster']
    lab, inn, _ = slic_cases.slice_stats(c)
    assert 0 not in lab[inn] and not inn[:14, :14].any()
    assert _run('empty_cluster')[1][0] >= 1


def test_tie_case_has_an_exact_tie():
    """9 rows, 2 cells: start rows 2 and 6, row 4 is at distance 2 from both; the constant image makes d equal."""
    assert (4 - 9 // 4) == ((3 * 9) // 4 - 4)
    np.testing.assert_array_equal(_run('tie')[0][4, :, 0], _run('tie')[0][3, :, 0])


def test_refusals():
    v = np.zeros((4, 5, 1))
    for kw in (dict(gh=0, gw=1), dict(gh=5, gw=1), dict(gh=1, gw=6)):
        with pytest.raises(ValueError):
            slic.slic_host(v, w=1.0, **kw)
    for kw in (dict(w=-1.0), dict(w=np.nan), dict(w=1.0, T=-1), dict(w=1.0, min_size=-1), dict(w=1.0, mask=np.ones((4, 5, 2), bool))):
        with pytest.raises(ValueError):
            slic.slic_host(v, 1, 1, **kw)


# --------------------------------------------------------------------------------------------------- the skimage-like arguments
def test_grid_for_hand_values():
    assert slic.grid_for(100, 100, 100) == (10, 10)
    assert slic.grid_for(256, 256, 1000) == (32, 32)      # step = 8.095..., 256 / step = 31.6
    assert slic.grid_for(20, 80, 16) == (2, 8)            # step = 10
    assert slic.grid_for(3, 3, 1000) == (3, 3)            # clamped to the axis
    assert slic.grid_for(50, 50, 1) == (1, 1)


def test_spatial_weight_hand_values():
    assert slic.spatial_weight(0.1, 100, 100, 10, 10) == (0.1 * 65535) ** 2 / 100.0
    assert slic.spatial_weight(1.0, 20, 80, 2, 8) == 65535.0 ** 2 / 100.0
    assert slic.spatial_weight(0.0, 9, 9, 3, 3) == 0.0
    with pytest.raises(ValueError):
        slic.spatial_weight(-1.0, 9, 9, 3, 3)


def test_oversegment_without_a_session_is_slic_host():
    c = CASES['odd']
    gh, gw = slic.grid_for(20, 28, 12)
    want = slic.slic_host(c['vol'], gh, gw, slic.spatial_weight(0.05, 20, 28, gh, gw), 3, 2)
    got = regions.oversegment(c['vol'], n_segments=12, compactness=0.05, T=3, min_size=2, with_counts=True)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
