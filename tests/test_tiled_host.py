"""Whole-volume inference by tiles, without a GPU: the lattice functions of the library (host arithmetic, no device call)
against nnal_amd/tiled.py, their refusals, and the statement's own properties."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import tiled_ref as ref


@pytest.fixture(scope='module')
def lib():
    import nnal_amd  # noqa: F401
    from nnal_amd import _lib
    return _lib.lib()


def test_lattice_functions_against_statement(lib):
    """alq_tile_count / alq_tile_origin / alq_tile_lattice_check for every (D, t, s) with D <= 13, t <= 6, s <= t on each axis in
    turn (the other two axes hold another lattice, so that the index arithmetic is exercised)."""
    from nnal_amd import tiled
    other = {0: ((7, 5), (3, 4), (2, 3)), 1: ((5, 9), (4, 3), (3, 1)), 2: ((4, 6), (2, 4), (1, 4))}
    for axis in range(3):
        for D in range(1, 14):
            for t in range(1, 7):
                for s in range(1, t + 1):
                    dims, tile, stride = (list(v) for v in other[axis])
                    dims.insert(axis, D), tile.insert(axis, t), stride.insert(axis, s)
                    lat = ref.lattice(dims, tile, stride)
                    assert lib.alq_tile_lattice_check(C.byref(lat)) == 0
                    counts = (C.c_int32 * 3)()
                    total = lib.alq_tile_count(C.byref(lat), counts)
                    want = tiled.tile_origins(dims, tile, stride)
                    assert tuple(counts) == tiled.tile_counts(dims, tile, stride) and total == len(want) == int(np.prod(tuple(counts)))
                    assert lib.alq_tile_count(C.byref(lat), None) == total
                    got = np.zeros((total, 3), dtype=np.int32)
                    for idx in range(total):
                        o = (C.c_int32 * 3)()
                        assert lib.alq_tile_origin(C.byref(lat), idx, o) == 0
                        got[idx] = tuple(o)
                    assert np.array_equal(got, want), (dims, tile, stride)


def test_every_voxel_is_covered_and_the_last_tile_ends_with_the_axis():
    from nnal_amd import tiled
    for D in range(1, 14):
        for t in range(1, 7):
            for s in range(1, t + 1):
                o = tiled.lattice_origins(D, t, s)
                assert o[0] == 0 and np.all(np.diff(o) >= 1) and np.all(np.diff(o) <= s)
                assert o[-1] + t == max(D, t)
                covered = np.zeros(D, dtype=bool)
                for a in o:
                    covered[a:a + t] = True
                assert covered.all(), (D, t, s)
                assert len(o) == (1 if D <= t else -(-(D - t) // s) + 1)


def test_lattice_refusals(lib):
    ok = ((9, 13, 11), (4, 6, 5), (2, 3, 2))
    assert lib.alq_tile_lattice_check(None) == -1 and b'null' in lib.alq_last_error()
    assert lib.alq_tile_count(None, None) == -1
    for field, axis, value, word in ((0, 1, 0, b'voxels'), (0, 2, -3, b'voxels'), (1, 0, 0, b'tile'), (2, 0, 0, b'stride'), (2, 1, 7, b'stride'),
                                     (2, 2, -1, b'stride')):
        args = [list(v) for v in ok]
        args[field][axis] = value
        lat = ref.lattice(*args)
        assert lib.alq_tile_lattice_check(C.byref(lat)) == -1, (field, axis, value)
        assert word in lib.alq_last_error() and b'axis %d' % axis in lib.alq_last_error()
        assert lib.alq_tile_count(C.byref(lat), None) == -1
        assert lib.alq_tile_origin(C.byref(lat), 0, (C.c_int32 * 3)()) == -1
    lat = ref.lattice(*ok)
    total = lib.alq_tile_count(C.byref(lat), None)
    assert total == 4 * 4 * 4
    o = (C.c_int32 * 3)()
    assert lib.alq_tile_origin(C.byref(lat), -1, o) == -1 and lib.alq_tile_origin(C.byref(lat), total, o) == -1
    assert b'tile 64 of 64' in lib.alq_last_error()
    assert lib.alq_tile_origin(C.byref(lat), 0, None) == -1
    assert lib.alq_tile_origin(C.byref(lat), total - 1, o) == 0 and tuple(o) == (5, 7, 6)
    assert lib.alq_tile_blend_trip_voxels() >= 256
    from nnal_amd import tiled
    for bad in ((0, 4, 2), (5, 0, 1), (5, 4, 0), (5, 4, 5)):
        with pytest.raises(ValueError):
            tiled.lattice_origins(*bad)
    with pytest.raises(ValueError):
        tiled.window('hann', 4)


def test_windows():
    from nnal_amd import tiled
    for t in (1, 2, 5, 8):
        u, tr, g = (tiled.window(name, t) for name in tiled.WINDOWS)
        assert u.dtype == tr.dtype == g.dtype == np.float32 and u.shape == tr.shape == g.shape == (t,)
        assert np.all(u == 1.) and np.array_equal(tr, np.minimum(np.arange(t) + 1, t - np.arange(t)).astype(np.float32))
        assert np.array_equal(g, g[::-1]) and np.all(g > 0) and g.max() <= 1.
        want = np.exp(-0.5 * ((np.arange(t, dtype=np.float64) - (t - 1) / 2.) / (t / 8.)) ** 2)
        assert np.array_equal(g, want.astype(np.float32))


def _random_tiles(rs, c, ntiles, tile):
    p = rs.rand(c, ntiles, *tile) + 0.01
    return (p / p.sum(axis=0, keepdims=True)).astype(np.float32)


def test_whole_tiles_without_overlap_come_back_untouched():
    """s = t on a volume of whole tiles: a voxel has one tile, its sum is w p and its weight w.  Under 'uniform' (w = 1) the
    quotient is p itself, bit for bit.  Under the other windows fl(fl(w p) / w) carries two roundings of relative size 2^-24
    each: |q - p| <= (2^-23 + 2^-47) p, asserted as 2^-22.9 p."""
    from nnal_amd import tiled
    rs = np.random.RandomState(5)
    tile, counts, c = (4, 6, 5), (2, 1, 3), 3
    dims = tuple(t * n for t, n in zip(tile, counts))
    P = _random_tiles(rs, c, int(np.prod(counts)), tile)
    org = tiled.tile_origins(dims, tile, tile)
    for name in tiled.WINDOWS:
        q, label = tiled.segment_host(P, dims, tile, tile, name, hwz=False)
        for j, (oz, oh, ow) in enumerate(org):
            got = q[:, oz:oz + 4, oh:oh + 6, ow:ow + 5]
            if name == 'uniform':
                assert got.tobytes() == P[:, j].tobytes()
            else:
                assert np.all(np.abs(got.astype(np.float64) - P[:, j]) <= 2. ** -22.9 * P[:, j])
            assert np.array_equal(label[oz:oz + 4, oh:oh + 6, ow:ow + 5], np.argmax(got, axis=0))


def test_equal_posteriors_in_every_tile_blend_to_the_same_bits():
    """Every tile holds the same dyadic value p_k per class (a few mantissa bits): under 'uniform' and 'triangle' the weights are
    small integers, so sum (w p) = p sum w without any rounding, and the quotient is p exactly - whatever the overlap."""
    from nnal_amd import tiled
    pk = np.array([0.125, 0.625, 0.25], dtype=np.float32)
    for dims, tile, stride in (((9, 13, 11), (4, 6, 5), (2, 3, 2)), ((11, 8, 9), (8, 8, 8), (4, 4, 4)), ((3, 4, 2), (4, 6, 5), (1, 1, 1))):
        ntiles = len(tiled.tile_origins(dims, tile, stride))
        P = np.broadcast_to(pk[:, None, None, None, None], (3, ntiles) + tile).copy()
        for name in ('uniform', 'triangle'):
            q, label = tiled.segment_host(P, dims, tile, stride, name, hwz=True)
            assert q.shape == (3, dims[1], dims[2], dims[0]) and label.shape == (dims[1], dims[2], dims[0])
            assert q.tobytes() == np.broadcast_to(pk[:, None, None, None], q.shape).astype(np.float32).tobytes(), (dims, name)
            assert np.all(label == 1)


@pytest.mark.parametrize('case', ['A', 'B', 'F'])
def test_blend_host_over_ranges_gives_equal_bytes(case):
    from nnal_amd import tiled
    dims, tile, stride, c, name, kind = ref.BLEND_CASES[case]
    ntiles = len(tiled.tile_origins(dims, tile, stride))
    V = int(np.prod(tile))
    post = ref.posterior_table(np.random.RandomState(17), 'random', c, ntiles, V)
    wins = [tiled.window(name, t) for t in tile]
    accs = []
    for per in (1, 3, None):
        acc = np.zeros((c + 1,) + dims, dtype=np.float32)
        for first, n in ref.cuts(ntiles, per):
            tiled.blend_host(acc, post.reshape(c, ntiles, V)[:, first:first + n].reshape(c, n * V), tile, stride, *wins, first=first, n=n)
        accs.append(acc)
    assert accs[0].tobytes() == accs[1].tobytes() == accs[2].tobytes()
    assert np.all(accs[0][c] > 0)


def test_blend_host_is_the_per_voxel_definition():
    """The statement against a literal loop, voxel by voxel, over all tiles in index order (a small case)."""
    from nnal_amd import tiled
    dims, tile, stride, c = (5, 4, 6), (3, 3, 4), (1, 2, 3), 2
    org = tiled.tile_origins(dims, tile, stride)
    V = int(np.prod(tile))
    rs = np.random.RandomState(2)
    post = ref.posterior_table(rs, 'random', c, len(org), V)
    wz, wh, ww = (tiled.window('gaussian', t) for t in tile)
    got = tiled.blend_host(np.zeros((c + 1,) + dims, dtype=np.float32), post, tile, stride, wz, wh, ww)
    want = np.zeros((c + 1,) + dims, dtype=np.float32)
    p5 = post.reshape(c, len(org), *tile)
    for z, h, w in itertools.product(*(range(d) for d in dims)):
        for idx, (oz, oh, ow) in enumerate(org):
            lz, lh, lw = z - oz, h - oh, w - ow
            if 0 <= lz < tile[0] and 0 <= lh < tile[1] and 0 <= lw < tile[2]:
                wt = np.float32(np.float32(wz[lz] * wh[lh]) * ww[lw])
                for k in range(c):
                    want[k, z, h, w] = np.float32(want[k, z, h, w] + np.float32(wt * p5[k, idx, lz, lh, lw]))
                want[c, z, h, w] = np.float32(want[c, z, h, w] + wt)
    assert got.tobytes() == want.tobytes()


def test_gather_host_and_finalize_host():
    from nnal_amd import tiled
    rs = np.random.RandomState(3)
    vol = rs.randn(3, 7, 6, 2).astype(np.float32)
    X = tiled.gather_host(vol, (4, 4, 8), (2, 2, 4), fill=-1.)
    org = tiled.tile_origins((3, 7, 6), (4, 4, 8), (2, 2, 4))
    assert X.shape == (len(org), 4, 4, 8, 2) and len(org) == 1 * 3 * 1
    for j, (oz, oh, ow) in enumerate(org):
        assert np.array_equal(X[j, :3, :, :6], vol[:, oh:oh + 4, :, :]) and np.all(X[j, 3:] == -1.) and np.all(X[j, :, :, 6:] == -1.)
    assert np.array_equal(tiled.gather_host(vol, (4, 4, 8), (2, 2, 4), first=1, n=2, fill=-1.), X[1:])
    acc = np.array([[[[1., 2., 0.]]], [[[1., 1., 0.]]], [[[2., 4., 0.]]]], dtype=np.float32)          # [c + 1 = 3, 1, 1, 3]
    q, label = tiled.finalize_host(acc)
    assert np.array_equal(q[:, 0, 0, :2], [[0.5, 0.5], [0.5, 0.25]]) and np.isnan(q[:, 0, 0, 2]).all()
    assert label.dtype == np.uint8 and label.tolist() == [[[0, 0, 0]]]          # ties and NaN: the first class
    q2, label2 = tiled.finalize_host(acc, hwz=True)
    assert q2.shape == (2, 1, 3, 1) and label2.shape == (1, 3, 1)


def test_signatures():
    import inspect
    from nnal_amd import device, eval_utils
    sig = inspect.signature(eval_utils.full_volume_segment)
    assert list(sig.parameters) == ['model', 'sess', 'img_paths_or_mats', 'data_reader', 'op', 'stride', 'window', 'fill', 'keep_on_device']
    assert sig.parameters['op'].default == 'prediction' and sig.parameters['window'].default == 'gaussian'
    assert sig.parameters['stride'].default is None and sig.parameters['keep_on_device'].default is False
    sig = inspect.signature(eval_utils.get_full_segs_tiled)
    assert list(sig.parameters) == ['model', 'sess', 'dat', 'stride', 'window', 'post_process', 'save_path', 'dat_writer']
    sig = inspect.signature(device.DeviceModel.forward_maps_device)
    assert sig.parameters['first_sample'].default == 0 and list(sig.parameters)[-1] == 'first_sample'
