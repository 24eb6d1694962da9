"""Whole-volume inference by tiles on the device (csrc/tile.hip, eval_utils.full_volume_segment; GPU box).

Kernels alone: alq_tile_gather, alq_tile_blend and alq_tile_finalize on arrays the test builds against nnal_amd/tiled.py on the
same arrays.  Every comparison is bit for bit (the statement is fp32 operation by operation and the file is compiled without
contraction), every output lies between pattern-filled guard margins, and the margins are checked.

Through the model: the statement is applied to the model's own posteriors of tiles the test cuts with torch indexing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import tiled_ref as ref  # noqa: E402

NAN = float('nan')


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


# ---------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize('case', sorted(ref.GATHER_CASES))
def test_gather_against_statement(sess, case):
    from nnal_amd import tiled
    torch = sess.torch
    dims, tile, stride, m, fill, rng = ref.GATHER_CASES[case]
    rs = np.random.RandomState(len(case))
    vol = rs.randn(*dims, m).astype(np.float32)
    lat = sess.tile_lattice(dims, tile, stride)
    ntiles = sess.tile_count(lat)
    first, n = rng or (0, ntiles)
    assert first + n <= ntiles and ('first' not in case or first > 0) and ('n = 1' not in case or n == 1)
    rowlen = tile[2] * m
    if 'vector' in case or 'misaligned' in case or 'fill' in case:
        assert rowlen % 4 == 0
    if 'scalar' in case:
        assert rowlen % 4 != 0
    if 'misaligned' in case:          # source rows that start off a 16-byte boundary, and some that start on one
        starts = {((z * dims[1] + h) * dims[2] + ow) * m % 4 for z in range(2) for h in range(2) for ow in tiled.lattice_origins(dims[2], tile[2], stride[2])}
        assert len(starts) > 1 and 0 in starts
    if 'fill' in case:
        assert any(D < t for D, t in zip(dims, tile))
    d_vol = ref.Guarded(sess, vol.shape, torch.float32, 12345., init=vol)
    X = ref.Guarded(sess, (n,) + tuple(tile) + (m,), torch.float32, NAN)
    sess.tile_gather(d_vol.t, lat, first, n, fill, out=X.t)
    want = tiled.gather_host(vol, tile, stride, first, n, fill)
    got = X.numpy()
    assert got.tobytes() == want.tobytes(), case
    assert X.margins_intact() and d_vol.margins_intact() and np.array_equal(d_vol.numpy(), vol)
    # an output that is only 4-byte aligned takes the one-float path: the same bytes
    X1 = ref.Guarded(sess, (want.size + 1,), torch.float32, NAN)
    sess.tile_gather(d_vol.t, lat, first, n, fill, out=X1.t[1:].view(want.shape))
    assert X1.numpy()[1:].tobytes() == want.tobytes() and np.isnan(X1.numpy()[0]) and X1.margins_intact()


# ---------------------------------------------------------------------------------------------------- blend and finalize
def _blend_device(sess, post, lat, dims, tile, c, wins, per):
    """acc after blending in cuts of `per` tiles: (bytes of the payload, margins intact)."""
    torch = sess.torch
    ntiles, V = sess.tile_count(lat), int(np.prod(tile))
    acc = ref.Guarded(sess, (c + 1,) + tuple(dims), torch.float32, -777.)
    acc.t.zero_()
    p3 = post.reshape(c, ntiles, V)
    for first, n in ref.cuts(ntiles, per):
        d_post = ref.Guarded(sess, (c, n * V), torch.float32, 4321., init=np.ascontiguousarray(p3[:, first:first + n]).reshape(c, n * V))
        sess.tile_blend(d_post.t, lat, first, n, wins, acc.t)
        assert d_post.margins_intact()
    return acc


def _finalize_all_forms(sess, acc, want_acc, c, dims):
    """Both layouts, with and without the posteriors, against finalize_host of the statement's accumulator."""
    from nnal_amd import tiled
    torch = sess.torch
    N = int(np.prod(dims))
    for hwz in (False, True):
        q, lab = tiled.finalize_host(want_acc, hwz)
        for want_post in (True, False):
            d_q = ref.Guarded(sess, q.shape, torch.float32, NAN) if want_post else None
            d_lab = ref.Guarded(sess, lab.shape, torch.uint8, 201)
            sess.tile_finalize(acc.t, hwz=hwz, want_post=want_post, post=d_q.t if want_post else None, label=d_lab.t)
            assert d_lab.numpy().tobytes() == lab.tobytes() and d_lab.margins_intact(), (hwz, want_post)
            if want_post:
                assert d_q.numpy().tobytes() == q.tobytes() and d_q.margins_intact(), hwz
                d_only = ref.Guarded(sess, q.shape, torch.float32, NAN)
                sess.tile_finalize(acc.t, hwz=hwz, want_label=False, post=d_only.t)
                assert d_only.numpy().tobytes() == q.tobytes() and d_only.margins_intact()
        # byte-aligned label pointer: the one-byte stores
        d_odd = ref.Guarded(sess, (N + 1,), torch.uint8, 201)
        sess.tile_finalize(acc.t, hwz=hwz, want_post=False, label=d_odd.t[1:].view(lab.shape))
        assert d_odd.numpy()[1:].tobytes() == lab.tobytes() and d_odd.numpy()[0] == 201 and d_odd.margins_intact()
    return q, lab


@pytest.mark.parametrize('case', sorted(ref.BLEND_CASES))
def test_blend_and_finalize_against_statement(sess, case):
    from nnal_amd import tiled
    torch = sess.torch
    dims, tile, stride, c, name, kind = ref.BLEND_CASES[case]
    lat = sess.tile_lattice(dims, tile, stride)
    ntiles, V = sess.tile_count(lat), int(np.prod(tile))
    assert ntiles == len(tiled.tile_origins(dims, tile, stride))
    post = ref.posterior_table(np.random.RandomState(ord(case)), kind, c, ntiles, V)
    host_wins = [tiled.window(name, t) for t in tile]
    wins = tuple(sess.to_device(w, torch.float32) for w in host_wins)
    want = tiled.blend_host(np.zeros((c + 1,) + tuple(dims), dtype=np.float32), post, tile, stride, *host_wins)
    first_acc = None
    for per in ref.RANGES:
        acc = _blend_device(sess, post, lat, dims, tile, c, wins, per)
        got = acc.numpy()
        assert got.tobytes() == want.tobytes(), (case, per)
        assert acc.margins_intact()
        first_acc = first_acc or acc
    q, lab = _finalize_all_forms(sess, first_acc, want, c, dims)
    if kind == 'ties':          # exact ties between classes do occur, and the first class wins them
        qz = np.moveaxis(q, 0, -1)
        top = qz.max(axis=-1, keepdims=True)
        assert np.any((qz == top).sum(axis=-1) > 1) and np.array_equal(lab, np.argmax(qz, axis=-1))
    if kind == 'zero plane':
        assert np.all(q[1] == 0.) and not np.any(lab == 1)
    # a call over a middle range alone touches nothing outside its tiles' bounding box, and inside it only voxels its tiles cover
    if ntiles >= 3:
        a, n = ntiles // 3, max(ntiles // 3, 1)
        part = ref.Guarded(sess, (c + 1,) + tuple(dims), torch.float32, -777.)
        part.t.zero_()
        p3 = np.ascontiguousarray(post.reshape(c, ntiles, V)[:, a:a + n]).reshape(c, n * V)
        sess.tile_blend(sess.to_device(p3, torch.float32), lat, a, n, wins, part.t)
        want_part = tiled.blend_host(np.zeros((c + 1,) + tuple(dims), dtype=np.float32), p3, tile, stride, *host_wins, first=a, n=n)
        assert part.numpy().tobytes() == want_part.tobytes() and part.margins_intact()


def test_bounding_box_beyond_one_sweep_of_the_capped_grid(sess):
    """80 x 81 x 81 voxels in one call over all 8 tiles of 48^3: the box is the volume and passes alq_tile_blend_trip_voxels()
    (asserted; 80 x 81 x 80 would not), so workgroups take a second voxel.  Z = 80 also has whole 32-plane tiles with 4-byte label
    stores and a ragged last one in the [H, W, Z] finalize."""
    from nnal_amd import tiled
    torch = sess.torch
    dims, tile, stride, c = (80, 81, 81), (48, 48, 48), (32, 33, 33), 2
    trip = int(sess.lib.alq_tile_blend_trip_voxels())
    assert 80 * 81 * 80 <= trip < int(np.prod(dims))
    lat = sess.tile_lattice(dims, tile, stride)
    ntiles, V = sess.tile_count(lat), int(np.prod(tile))
    assert ntiles == 8
    post = ref.posterior_table(np.random.RandomState(8), 'random', c, ntiles, V)
    host_wins = [tiled.window('gaussian', t) for t in tile]
    wins = tuple(sess.to_device(w, torch.float32) for w in host_wins)
    want = tiled.blend_host(np.zeros((c + 1,) + dims, dtype=np.float32), post, tile, stride, *host_wins)
    for per in (None, 3):
        acc = _blend_device(sess, post, lat, dims, tile, c, wins, per)
        assert acc.numpy().tobytes() == want.tobytes() and acc.margins_intact(), per
    _finalize_all_forms(sess, acc, want, c, dims)


def test_refusals(sess):
    """Before any launch: the outputs keep their pattern, the message names the condition."""
    torch = sess.torch
    lib = sess.lib
    dims, tile, stride = (9, 13, 11), (4, 6, 5), (2, 3, 2)
    lat = ref.lattice(dims, tile, stride)
    ntiles = lib.alq_tile_count(C.byref(lat), None)
    buf = ref.Guarded(sess, (4096,), torch.float32, 55.)
    lab = ref.Guarded(sess, (4096,), torch.uint8, 9)
    p, pl = buf.t.data_ptr(), lab.t.data_ptr()
    P = C.c_void_p
    bad_lat = ref.lattice(dims, tile, (2, 7, 2))
    huge = ref.lattice((2048, 1024, 1024), tile, stride)
    i3 = (C.c_int32 * 3)

    def gather(vol=p, m=1, la=lat, first=0, n=1, X=p):
        return lib.alq_tile_gather(sess.ctx, P(vol) if vol else None, m, C.byref(la) if la else None, first, n, 0., P(X) if X else None)

    def blend(post=p, c=2, la=lat, first=0, n=1, wz=p, wh=p, ww=p, acc=p):
        return lib.alq_tile_blend(sess.ctx, *[P(v) if v else None for v in (post,)], c, C.byref(la) if la else None, first, n,
                                  *[P(v) if v else None for v in (wz, wh, ww, acc)])

    def finalize(acc=p, c=2, d=(2, 3, 4), hwz=0, post=p, label=pl):
        return lib.alq_tile_finalize(sess.ctx, P(acc) if acc else None, c, i3(*d) if d else None, hwz, P(post) if post else None,
                                     P(label) if label else None)

    checks = [
        (lambda: gather(vol=None), -1, b'null'), (lambda: gather(X=None), -1, b'null'), (lambda: gather(la=None), -1, b'null'),
        (lambda: gather(la=bad_lat), -1, b'stride'), (lambda: gather(first=-1), -1, b'tiles'), (lambda: gather(n=0), -1, b'tiles'),
        (lambda: gather(first=ntiles - 1, n=2), -1, b'tiles'), (lambda: gather(m=0), -1, b'modalities'),
        (lambda: gather(vol=p + 2), -1, b'aligned'), (lambda: gather(X=p + 1), -1, b'aligned'),
        (lambda: gather(m=9), -4, b'modalities'), (lambda: gather(la=huge), -4, b'2^31'),
        (lambda: blend(post=None), -1, b'null'), (lambda: blend(ww=None), -1, b'null'), (lambda: blend(acc=None), -1, b'null'),
        (lambda: blend(la=bad_lat), -1, b'stride'), (lambda: blend(first=-2), -1, b'tiles'), (lambda: blend(first=ntiles, n=1), -1, b'tiles'),
        (lambda: blend(acc=p + 2), -1, b'aligned'), (lambda: blend(wh=p + 3), -1, b'aligned'),
        (lambda: blend(c=1), -4, b'classes'), (lambda: blend(c=9), -4, b'classes'), (lambda: blend(la=huge), -4, b'2^31'),
        (lambda: finalize(acc=None), -1, b'null'), (lambda: finalize(d=None), -1, b'null'), (lambda: finalize(d=(2, 0, 4)), -1, b'volume'),
        (lambda: finalize(hwz=2), -1, b'hwz'), (lambda: finalize(post=p + 2), -1, b'aligned'),
        (lambda: finalize(c=1), -4, b'classes'), (lambda: finalize(c=9), -4, b'classes'),
        (lambda: finalize(d=(2048, 1024, 1024)), -4, b'2^31'),
    ]
    for i, (call, code, word) in enumerate(checks):
        assert call() == code, i
        assert word in lib.alq_last_error(), (i, lib.alq_last_error())
    sess.synchronize()
    assert np.all(buf.numpy() == 55.) and np.all(lab.numpy() == 9) and buf.margins_intact() and lab.margins_intact()
    with pytest.raises(ValueError, match='stride'):
        sess.tile_lattice(dims, tile, (2, 7, 2))


# ---------------------------------------------------------------------------------------------------- through the model
def _model(sess, fn, c, in_shape, max_batch, seed=23, **kw):
    from nnal_amd import device, netspec
    ld, sk = getattr(netspec, fn)(c)
    m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch, **kw)
    m.set_weights(netspec.he_init(ld, in_shape, seed=seed, skips=sk, bias_std=0.05))
    return m


def _statement(sess, model, imgs, tile, stride, window, fill=0.):
    """tiled.segment_host on the model's posteriors of the tiles cut with torch indexing out of the (h, w, z) arrays `imgs`:
    (q float32 [c, h, w, z], label uint8 [h, w, z], tile posteriors [c, n tiles, tz, th, tw])."""
    from nnal_amd import tiled
    torch = sess.torch
    vol = torch.as_tensor(np.stack([np.asarray(v, dtype=np.float32) for v in imgs], axis=-1)).to(sess.device).permute(2, 0, 1, 3)      # [Z, H, W, m]
    dims = tuple(int(v) for v in vol.shape[:3])
    org = tiled.tile_origins(dims, tile, stride)
    X = torch.full((len(org),) + tuple(tile) + (len(imgs),), float(fill), dtype=torch.float32, device=sess.device)
    for j, (oz, oh, ow) in enumerate(org):
        src = vol[oz:oz + tile[0], oh:oh + tile[1], ow:ow + tile[2]]
        X[j, :src.shape[0], :src.shape[1], :src.shape[2]] = src
    c = model.nclass
    maps = model.forward_maps_device(X.contiguous(), len(org))[0]          # [n, *spatial, c]
    P = maps.movedim(-1, 0).reshape((c, len(org)) + tuple(tile)).cpu().numpy()
    q, label = tiled.segment_host(P, dims, tile, stride, window, hwz=True)
    return q, label, P


def test_net_c_dense_whole_volume(sess):
    """net_c_dense(2) with 8^3 tiles on (h, w, z) = (12, 20, 11): 2 x 2 x 4 = 16 tiles at the default stride; max_batch = 5 (four
    passes, the last one of a single tile) and 16 (one pass) equal the statement and each other."""
    from nnal_amd import eval_utils, tiled
    from nnal_amd.datasets.utils import ResidentSubject
    rs = np.random.RandomState(41)
    vol = rs.randn(12, 20, 11).astype(np.float32)
    assert tiled.tile_counts((11, 12, 20), (8, 8, 8), (4, 4, 4)) == (2, 2, 4)
    outs = {}
    for mb in (5, 16):
        m = _model(sess, 'net_c_dense', 2, (8, 8, 8, 1), mb)
        assert m.max_batch == mb
        if mb == 16:
            q, label, _ = _statement(sess, m, [vol], (8, 8, 8), (4, 4, 4), 'gaussian')
        post = eval_utils.full_volume_segment(m, sess, vol, op='posterior')
        pred = eval_utils.full_volume_segment(m, sess, [vol], None, 'prediction')
        dev = eval_utils.full_volume_segment(m, sess, ResidentSubject.pack(sess, [vol]), op='prediction', keep_on_device=True)
        assert post.dtype == pred.dtype == np.float64 and post.shape == (2, 12, 20, 11) and pred.shape == (12, 20, 11)
        assert dev.dtype == sess.torch.uint8 and tuple(dev.shape) == (12, 20, 11) and np.array_equal(dev.cpu().numpy(), pred)
        outs[mb] = (post, pred)
        m.close()
    for mb in (5, 16):
        assert outs[mb][0].astype(np.float32).tobytes() == q.tobytes(), mb
        assert np.array_equal(outs[mb][1], label), mb
    assert 0 < outs[5][1].sum() < outs[5][1].size
    assert np.all(np.abs(outs[5][0].sum(axis=0) - 1.) < 1e-5)


def test_whole_tiles_equal_the_forward_outputs(sess):
    """s = t on (h, w, z) = (16, 8, 8): two tiles side by side; under the uniform window (w = 1) the volume's posteriors are the two
    tiles' forward outputs, bit for bit; under the default window they equal the statement."""
    from nnal_amd import eval_utils
    rs = np.random.RandomState(43)
    vol = rs.randn(16, 8, 8).astype(np.float32)
    m = _model(sess, 'net_c_dense', 2, (8, 8, 8, 1), 4)
    q, label, P = _statement(sess, m, [vol], (8, 8, 8), (8, 8, 8), 'uniform')
    assert P.shape == (2, 2, 8, 8, 8)
    got = eval_utils.full_volume_segment(m, sess, vol, op='posterior', stride=8, window='uniform').astype(np.float32)
    for j in range(2):          # P [c, tile, z, h, w] -> (c, h, w, z)
        assert got[:, 8 * j:8 * j + 8].tobytes() == np.ascontiguousarray(P[:, j].transpose(0, 2, 3, 1)).tobytes()
    qg, lg, _ = _statement(sess, m, [vol], (8, 8, 8), (8, 8, 8), 'gaussian')
    assert eval_utils.full_volume_segment(m, sess, vol, op='posterior', stride=(8, 8, 8)).astype(np.float32).tobytes() == qg.tobytes()
    m.close()


def test_net_c_2d_dense_whole_volume_and_slices(sess):
    """net_c_2d_dense at 16 x 16 (two channels) on (20, 24, 3) with stride 8: tiles (1, 16, 16), 2 x 2 per slice; and on a volume
    whose slices are the model's input, 'prediction' under the uniform window is full_slice_segment's array."""
    from nnal_amd import NN_extended, eval_utils, netspec, tiled
    rs = np.random.RandomState(47)
    imgs = [rs.randn(20, 24, 3).astype(np.float32) for _ in range(2)]
    ld, sk = netspec.net_c_2d_dense(3)
    m = NN_extended.CNN((16, 16, 2), ld, 'tiled2d', list(sk), sess=sess, max_batch=5)
    m.set_weights(netspec.he_init(ld, (16, 16, 2), seed=29, skips=sk, bias_std=0.05))
    assert tiled.tile_counts((3, 20, 24), (1, 16, 16), (1, 8, 8)) == (3, 2, 2)
    q, label, _ = _statement(sess, m, imgs, (1, 16, 16), (1, 8, 8), 'gaussian')
    post = eval_utils.full_volume_segment(m, sess, imgs, None, 'posterior', stride=8)
    pred = eval_utils.full_volume_segment(m, sess, imgs, None, 'prediction', stride=8)
    assert post.shape == (3, 20, 24, 3) and post.astype(np.float32).tobytes() == q.tobytes()
    assert pred.shape == (20, 24, 3) and np.array_equal(pred, label)
    whole = [rs.randn(16, 16, 6).astype(np.float32) for _ in range(2)]
    np.random.seed(3)
    want = eval_utils.full_slice_segment(m, sess, whole, None, 'prediction')
    got = eval_utils.full_volume_segment(m, sess, whole, None, 'prediction', window='uniform')
    assert got.shape == want.shape == (16, 16, 6) and got.dtype == want.dtype and np.array_equal(got, want)
    assert len(np.unique(got)) > 1
    m.close()


def test_get_full_segs_tiled_post_process(sess):
    """One model for subjects of two sizes; post_process=True equals post_processing's functions on the plain result."""
    from nnal_amd import eval_utils, post_processing as pp
    rs = np.random.RandomState(53)
    vols = [rs.randn(20, 24, 4).astype(np.float32), rs.randn(16, 19, 3).astype(np.float32)]
    m = _model(sess, 'net_c_2d_dense', 2, (16, 16, 1), 8, seed=19)

    class Dat(object):
        mods = ['T1']
        img_addrs = {'T1': vols}
        reader = None
    plain = eval_utils.get_full_segs_tiled(m, sess, Dat())
    assert [s.shape for s in plain] == [(20, 24, 4), (16, 19, 3)] and all(s.dtype == np.float64 for s in plain)
    for s, v in zip(plain, vols):
        assert np.array_equal(s, eval_utils.full_volume_segment(m, sess, v))
    done = eval_utils.get_full_segs_tiled(m, sess, Dat(), post_process=True)
    for s, d in zip(plain, done):
        assert 0 < s.sum() < s.size
        want = pp.fill_holes(pp.connected_component_analysis_3d(s, sess=sess), sess=sess)
        assert d.dtype == want.dtype and np.array_equal(d, want)
    m.close()


def test_mc_posterior_does_not_depend_on_the_batch(sess):
    """'MC-posterior': the dropout masks are keyed by (pass seed, tile index), the seeds are drawn once per call - max_batch = 3 and
    8 give the same bytes under one np.random seed, and another seed gives other ones."""
    from nnal_amd import NN_extended, eval_utils, netspec
    rs = np.random.RandomState(59)
    vol = rs.randn(20, 24, 2).astype(np.float32)
    ld, sk = netspec.net_c_2d_dense(2)
    outs = []
    for mb, seed in ((3, 7), (8, 7), (8, 8)):
        m = NN_extended.CNN((16, 16, 1), ld, 'tiledmc%d' % mb, list(sk), dropout=[[0], 0.5], sess=sess, max_batch=mb)
        m.set_weights(netspec.he_init(ld, (16, 16, 1), seed=31, skips=sk, bias_std=0.05))
        np.random.seed(seed)
        outs.append(eval_utils.full_volume_segment(m, sess, vol, op='MC-posterior'))
        m.close()
    assert outs[0].shape == (2, 20, 24, 2) and outs[0].tobytes() == outs[1].tobytes() and outs[0].tobytes() != outs[2].tobytes()
    assert np.all(np.abs(outs[0].sum(axis=0) - 1.) < 1e-5)


def test_fc_head_model_is_refused(sess):
    from nnal_amd import eval_utils
    m = _model(sess, 'net_c_2d', 2, (16, 16, 1), 2)
    with pytest.raises(NotImplementedError):
        eval_utils.full_volume_segment(m, sess, np.zeros((16, 16, 2), np.float32))
    m.close()
    d = _model(sess, 'net_c_2d_dense', 2, (16, 16, 1), 2)
    with pytest.raises(ValueError):
        eval_utils.full_volume_segment(d, sess, np.zeros((16, 16, 2), np.float32), op='loss')
    with pytest.raises(ValueError):
        eval_utils.full_volume_segment(d, sess, np.zeros((16, 16, 2), np.float32), stride=(8, 8, 8))
    with pytest.raises(ValueError, match='stride'):
        eval_utils.full_volume_segment(d, sess, np.zeros((16, 16, 2), np.float32), stride=17)
    d.close()
