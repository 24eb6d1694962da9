"""The region primitives on the device (csrc/region.hip): alq_local_var2d and alq_segment_min bit for bit against their NumPy
restatements (nnal_amd.regions), get_HV_inds / partition_2d_indices against the reference's outputs
(tests/golden/r9_regions.npz), `ps-random` through both query functions and SuPix_query('entropy') against restatements
(GPU box)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from tests.test_committee_host import Expr  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'r9_regions.npz'))


BOX = (21, 19, 70)      # 70 slices: more than one wave along z and a partial one; 21 x 19: several row and column tiles, none whole


@pytest.fixture(scope='module')
def box_values():
    rs = np.random.RandomState(901)
    return rs.randint(0, 4096, size=BOX) + rs.rand(*BOX)


def _padded(vals, rads, dtype):
    return np.pad(vals.astype(dtype), [(r, r) for r in rads], 'constant')


# ------------------------------------------------------------------------------------------------ alq_local_var2d
@pytest.mark.parametrize('d', [1, 2, 5, 12, 13, 33])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('rads', [(12, 12, 0), (2, 2, 1)])
def test_whole_map_bit_exact(sess, box_values, rads, dtype, d):
    from nnal_amd import patch_utils, regions
    vol = _padded(box_values, rads, dtype)
    assert vol.shape == tuple(BOX[a] + 2 * rads[a] for a in range(3))
    got = patch_utils.DeviceVolumes(sess, [vol]).local_var(d, 0, None, rads).cpu().numpy()
    np.testing.assert_array_equal(got, regions.local_var2d_host(vol, d, rads))


def test_whole_map_single_slice(sess):
    from nnal_amd import patch_utils, regions
    rs = np.random.RandomState(902)
    vol = np.pad(rs.randint(0, 4096, size=(21, 19, 1)) + rs.rand(21, 19, 1), [(3, 3), (3, 3), (0, 0)], 'constant')
    for d in (3, 12):
        got = patch_utils.DeviceVolumes(sess, [vol]).local_var(d, 0, None, (3, 3, 0)).cpu().numpy()
        assert got.shape == (21, 19, 1)
        np.testing.assert_array_equal(got, regions.local_var2d_host(vol, d, (3, 3, 0)))


def test_whole_map_values_near_2_pow_20(sess):
    """d = 33: sums of up to 1089 values near 2^20 (S1 beyond 2^30, S2 near 2^50) - a 32-bit sum would overflow while
    trunc(max)^2 d^2 < 2^53 still holds."""
    from nnal_amd import patch_utils, regions
    rs = np.random.RandomState(903)
    vals = (2 ** 20 - rs.randint(1, 5000, size=(40, 37, 5))).astype(np.float64) + rs.rand(40, 37, 5)
    assert int(vals.max()) ** 2 * 33 ** 2 < 2 ** 53 and int(vals.max()) * 33 ** 2 > 2 ** 30
    for dtype in (np.float32, np.float64):
        vol = _padded(vals, (1, 0, 2), dtype)
        got = patch_utils.DeviceVolumes(sess, [vol]).local_var(33, 0, None, (1, 0, 2)).cpu().numpy()
        want = regions.local_var2d_host(vol, 33, (1, 0, 2))
        assert want.max() > 2. ** 20
        np.testing.assert_array_equal(got, want)


def test_whole_map_same_bits_for_every_row_tile(sess, box_values, monkeypatch):
    """The rows a lane sweeps (chosen from the volume and the device; ALQ_LVAR_ROWS overrides) never change a bit."""
    from nnal_amd import patch_utils, regions
    vol = _padded(box_values, (2, 2, 1), np.float32)
    want = regions.local_var2d_host(vol, 12, (2, 2, 1))
    dv = patch_utils.DeviceVolumes(sess, [vol])
    for rows in ('1', '5', '64'):
        monkeypatch.setenv('ALQ_LVAR_ROWS', rows)
        np.testing.assert_array_equal(dv.local_var(12, 0, None, (2, 2, 1)).cpu().numpy(), want)


def test_indexed_form_equals_whole_map(sess, box_values):
    from nnal_amd import patch_utils
    rs = np.random.RandomState(904)
    inds = rs.randint(0, int(np.prod(BOX)), size=3001)            # out of order, with repeats
    inds[:40] = inds[100:140]
    inds[-3:] = [0, int(np.prod(BOX)) - 1, 0]
    for dtype, rads, d in ((np.float32, (12, 12, 0), 12), (np.float64, (2, 2, 1), 5), (np.float32, (2, 2, 1), 33)):
        dv = patch_utils.DeviceVolumes(sess, [_padded(box_values, rads, dtype)])
        whole = dv.local_var(d, 0, None, rads).cpu().numpy()
        got = dv.local_var(d, 0, inds, rads).cpu().numpy()
        np.testing.assert_array_equal(got, whole.reshape(-1)[inds])
    with pytest.raises(IndexError):
        dv.local_var(5, 0, [int(np.prod(BOX))], (2, 2, 1))


def test_precondition_raises_before_any_launch(sess):
    from nnal_amd import patch_utils
    base = np.full((6, 7, 3), 5.)
    for bad in (-1., np.nan, 2. ** 26):
        vol = base.copy()
        vol[1, 2, 1] = bad
        with pytest.raises(ValueError):
            patch_utils.DeviceVolumes(sess, [vol]).local_var(5)
    with pytest.raises(ValueError):
        patch_utils.get_vars_2d(-base[:, :, 0], 3)
    with pytest.raises(ValueError):
        patch_utils.DeviceVolumes(sess, [base]).local_var(66)
    # the C entry point refuses the window on its own (ALQ_EINVAL = -1), before any launch
    dv = patch_utils.DeviceVolumes(sess, [base])
    out = sess.empty((6, 7, 3), sess.torch.float64)
    pd, rd = (C.c_int64 * 3)(6, 7, 3), (C.c_int32 * 3)(0, 0, 0)
    for d in (0, 66):
        assert sess.lib.alq_local_var2d(sess.ctx, C.c_void_p(dv.tensors[0].data_ptr()), 1, pd, rd, d, None, 0, C.c_void_p(out.data_ptr())) == -1


def test_get_vars_2d_HV_inds_and_partition_equal_the_reference(sess, gold):
    from nnal_amd import PW_NNAL, patch_utils
    vol = gold['vol'].astype(np.float64)
    for d in gold['gv_d']:
        for s_, z in enumerate(gold['gv_slices']):
            np.testing.assert_array_equal(patch_utils.get_vars_2d(vol[:, :, z], int(d)), gold['gv_var_%d' % d][:, :, s_])
    pool = gold['hv_pool']
    for tag in 'ab':
        pshape = tuple(int(v) for v in gold['hv_pshape_' + tag])
        rads = patch_utils.patch_radii(pshape)
        padded = np.pad(vol, [(r, r) for r in rads], 'constant')
        got = PW_NNAL.get_HV_inds(padded, pshape, 2., pool)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, gold['hv_valid_' + tag])
        got32 = PW_NNAL.get_HV_inds(padded.astype(np.float32), pshape, 2., list(pool))
        np.testing.assert_array_equal(got32, gold['hv_valid_' + tag])
    assert len(PW_NNAL.get_HV_inds(padded, pshape, 2., [])) == 0
    a, b, c = patch_utils.partition_2d_indices(vol[:, :, int(gold['part_slice'])], gold['part_mask'])
    np.testing.assert_array_equal(a, gold['part_masked'])
    np.testing.assert_array_equal(b, gold['part_hvar'])
    np.testing.assert_array_equal(c, gold['part_lvar'])


# ------------------------------------------------------------------------------------------------ alq_segment_min
def _segmin(sess, seg, inds, scores, n_labels, guard=64):
    """alq_segment_min into the middle of a larger buffer: -> (table, guard cells in front, guard cells behind)."""
    torch = sess.torch
    sess.bind_stream()
    S = seg.shape[2]
    buf = torch.full((guard + S * n_labels + guard,), -7., dtype=torch.float64, device=sess.device)
    table = buf[guard:guard + S * n_labels]
    d_lab = sess.to_device(seg.astype(np.int32), torch.int32)
    d_inds = sess.to_device(np.asarray(inds, dtype=np.int64), torch.int64)
    d_sc = sess.to_device(np.asarray(scores, dtype=np.float64), torch.float64)
    dims = (C.c_int64 * 3)(*seg.shape)
    from nnal_amd._lib import check
    check(sess.lib.alq_segment_min(sess.ctx, C.c_void_p(d_lab.data_ptr()), dims, n_labels, C.c_void_p(d_inds.data_ptr()),
                                   C.c_void_p(d_sc.data_ptr()), len(inds), C.c_void_p(table.data_ptr())))
    out = buf.cpu().numpy()
    return out[guard:-guard].reshape(S, n_labels), out[:guard], out[-guard:]


def _scores(rs, n):
    s = np.round(rs.rand(n), 2)                     # exact ties
    s[rs.rand(n) < .02] = 0.
    s[rs.rand(n) < .02] = 5e-324                    # denormals
    s[rs.rand(n) < .02] = 2.5e-310
    return s


def test_segment_min_many_labels(sess):
    from nnal_amd import regions
    rs = np.random.RandomState(905)
    shape = (17, 13, 9)
    seg = rs.randint(0, 41, size=shape)
    seg[:, :, 2][seg[:, :, 2] > 10] = 0             # labels missing from a slice
    seg[:, :, 5][seg[:, :, 5] % 3 == 1] = 7
    inds = rs.permutation(int(np.prod(shape)))[:1200]
    inds = inds[(inds % 9 != 4) & (inds % 9 != 6)]  # two slices without a scored voxel
    scores = _scores(rs, len(inds))
    want = regions.segment_min_host(seg, inds, scores, 41)
    assert np.isinf(want[[4, 6]]).all() and np.isinf(want[2, 11:]).all() and (want == 0).any() and (want == 5e-324).any()
    got, g0, g1 = _segmin(sess, seg, inds, scores, 41)
    np.testing.assert_array_equal(got, want)
    assert np.all(g0 == -7.) and np.all(g1 == -7.)
    from nnal_amd import PW_NNAL
    np.testing.assert_array_equal(PW_NNAL.superpix_scoring(seg, inds, scores), want)
    with pytest.raises(ValueError):
        PW_NNAL.superpix_scoring(seg, np.concatenate([inds, inds[:1]]), np.concatenate([scores, scores[:1]]))


def test_segment_min_few_cells_many_workgroups(sess):
    from nnal_amd import regions
    rs = np.random.RandomState(906)
    shape = (64, 64, 20)
    seg = rs.randint(0, 4, size=shape)
    inds = rs.permutation(int(np.prod(shape)))[:70001]
    scores = _scores(rs, len(inds)) + 1e-3
    scores[rs.rand(len(inds)) < 1e-3] = 0.
    want = regions.segment_min_host(seg, inds, scores, 4)
    got, g0, g1 = _segmin(sess, seg, inds, scores, 4)
    np.testing.assert_array_equal(got, want)
    assert np.all(g0 == -7.) and np.all(g1 == -7.)
    got2 = _segmin(sess, seg, inds, scores, 4)[0]
    np.testing.assert_array_equal(got2, got)


def test_segment_min_label_beyond_the_table(sess):
    from nnal_amd import regions
    rs = np.random.RandomState(907)
    shape = (17, 13, 9)
    seg = rs.randint(0, 41, size=shape)
    inds = rs.permutation(int(np.prod(shape)))[:1500]
    scores = _scores(rs, len(inds))
    got, g0, g1 = _segmin(sess, seg, inds, scores, 5)
    np.testing.assert_array_equal(got, regions.segment_min_host(seg, inds, scores, 5))
    assert np.all(g0 == -7.) and np.all(g1 == -7.)
    got, g0, g1 = _segmin(sess, seg + 1000, inds, scores, 5)          # every label >= n_labels: nothing but the fill
    assert np.all(np.isinf(got)) and np.all(got > 0) and np.all(g0 == -7.) and np.all(g1 == -7.)


# ------------------------------------------------------------------------------------------------ the queries
PSHAPE = (5, 5, 3)
RADS = (2, 2, 1)


def _textured(rs, shp):
    v = np.full(shp, 20.)
    v[:shp[0] // 2] = rs.randint(0, 50, size=(shp[0] // 2,) + shp[1:]) + rs.rand(shp[0] // 2, *shp[1:])
    v[shp[0] // 2:, :, ::2] += np.arange(shp[1])[None, :, None] * 0.25
    return v


def _subjects():
    """Two subjects of two modalities + mask; the first modality of the second one is all zero: none of its voxels has any
    local variance (a non-zero constant would have some along the borders, where the window is zero-filled)."""
    rs = np.random.RandomState(908)
    shapes = [(16, 14, 6), (9, 10, 4)]
    imgs, pools = [], []
    for s_, shp in enumerate(shapes):
        first = _textured(rs, shp) if s_ == 0 else np.zeros(shp)
        mods = [np.pad(v, [(r, r) for r in RADS], 'constant') for v in (first, rs.randn(*shp))]
        imgs.append(mods + [rs.randint(0, 2, size=shp).astype(np.float64)])
        nv = int(np.prod(shp))
        pools.append(rs.permutation(nv)[:nv // 2])
    return imgs, pools


@pytest.fixture(scope='module')
def net(sess):
    from nnal_amd import NN
    ld = netspec.net_a()
    in_shape = (5, 5, 6)
    m = NN.CNN(in_shape, ld, 'regions', None, None, sess=sess, max_batch=128)
    m.set_weights(netspec.he_init(ld, in_shape, seed=93, bias_std=0.2))
    yield m
    m.close()


def _valid(img0, pool):
    from nnal_amd import regions
    vmap = regions.local_var2d_host(img0, RADS[0], RADS)
    return np.nonzero(vmap.reshape(-1)[np.asarray(pool)] > 2.)[0]


def test_ps_random_query_multimg(sess, net):
    from nnal_amd import PW_NNAL, patch_utils
    imgs, pools = _subjects()
    valid = [_valid(imgs[i][0], pools[i]) for i in range(2)]
    sizes = [len(v) for v in valid]
    assert 20 < sizes[0] < len(pools[0]) and sizes[1] == 0
    stats = np.array([[0., 1., 0., 1.], [0., 1., 0., 1.]])
    for k, seed in ((10, 3), (10, 4), (sizes[0] + 50, 5)):
        expr = Expr({'patch_shape': PSHAPE, 'ntb': 64, 'k': k, 'B': 40}, stats)
        np.random.seed(seed)
        got = PW_NNAL.query_multimg(expr, net, sess, imgs, [list(p) for p in pools], [[], []], 'ps-random')
        np.random.seed(seed)
        rand = np.random.permutation(int(np.sum(sizes)))[:k]
        local = patch_utils.global2local_inds(rand, sizes)
        assert len(got) == 2 and len(got[1]) == 0 and len(got[0]) == min(k, sizes[0])
        for i in range(2):
            np.testing.assert_array_equal(got[i], valid[i][local[i]])
    assert sorted(got[0]) == sorted(valid[0])                     # k beyond the qualifying count: all of them


def test_ps_random_CNN_query(sess, net):
    from nnal_amd import PW_NNAL
    imgs, pools = _subjects()
    stats = [[0., 1.], [0., 1.]]
    valid = _valid(imgs[0][0], pools[0])
    for k, seed in ((7, 11), (len(valid) + 9, 12)):
        expr = Expr({'patch_shape': PSHAPE, 'ntb': 64, 'k': k, 'B': 40, 'stats': stats}, None)
        np.random.seed(seed)
        got = PW_NNAL.CNN_query(expr, net, sess, imgs[0][:2], pools[0], [], 'ps-random')
        np.random.seed(seed)
        np.testing.assert_array_equal(got, valid[np.random.permutation(len(valid))[:k]])
    expr = Expr({'patch_shape': PSHAPE, 'ntb': 64, 'k': 5, 'B': 40, 'stats': stats}, None)
    assert len(PW_NNAL.CNN_query(expr, net, sess, imgs[1][:2], pools[1], [], 'ps-random')) == 0      # the flat subject


def test_SuPix_query_entropy(sess, net):
    from nnal_amd import PW_NN, PW_NNAL, regions
    imgs, pools = _subjects()
    shp = (16, 14, 6)
    rs = np.random.RandomState(909)
    seg = np.zeros(shp, dtype=np.int64)
    for z in range(shp[2]):
        cells = (np.arange(shp[0])[:, None] // 4) * 4 + (np.arange(shp[1])[None, :] + z) // 4
        seg[:, :, z] = np.where(rs.rand(shp[0], shp[1]) < .1, 0, 1 + (cells + 3 * z) % 17)
    stats = [[0., 1.], [0., 1.]]
    pool = np.sort(pools[0])
    pool = pool[pool % shp[2] != 2]                                   # a slice without a scored voxel
    k = 11
    expr = Expr({'patch_shape': PSHAPE, 'ntb': 64, 'k': k, 'B': 40, 'stats': stats}, None)
    qSuPix, qinds = PW_NNAL.SuPix_query(expr, net, sess, imgs[0][:2], pool, seg, 'entropy')
    posts = PW_NN.batch_eval(net, sess, imgs[0][:2], pool, PSHAPE, 64, stats, 'posteriors')[0]
    table = regions.segment_min_host(seg, pool, np.abs(posts - .5))
    assert table.shape == (shp[2], int(seg.max()) + 1)
    order = np.argsort(table.ravel(), kind='stable')[:k]
    assert np.all(np.isfinite(table.ravel()[order]))
    np.testing.assert_array_equal(qSuPix, np.array(np.unravel_index(order, table.shape)))
    assert qSuPix.shape == (2, k) and not np.any(qSuPix[0] == 2)
    assert len(qinds) == k
    for i in range(k):
        z, l = int(qSuPix[0, i]), int(qSuPix[1, i])
        ii, jj = np.nonzero(seg[:, :, z] == l)
        np.testing.assert_array_equal(qinds[i], np.ravel_multi_index((ii, jj, np.full(len(ii), z)), shp))
    expr.pars['k'] = int(np.isfinite(table).sum()) + 1
    with pytest.raises(ValueError):
        PW_NNAL.SuPix_query(expr, net, sess, imgs[0][:2], pool, seg, 'entropy')
    with pytest.raises(NotImplementedError):
        PW_NNAL.SuPix_query(expr, net, sess, imgs[0][:2], pool, seg, 'random')
