"""Post-processing on the device (csrc/ccl.hip; GPU box): alq_cc_label, alq_cc_keep_largest and alq_fill_holes against the
scipy.ndimage restatements of nnal_amd.regions and against expected arrays written down from how the volumes were built
(tests/postproc_cases.py), the wrappers of nnal_amd.post_processing against a literal restatement of the reference, and
full_model_eval(post_process=True).  Integers throughout: every comparison is an equality."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from tests import postproc_cases as pc  # noqa: E402
from tests.test_committee_host import Expr  # noqa: E402


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _dev(sess, seg):
    return sess.to_device(np.asarray(seg, dtype=np.uint8), sess.torch.uint8)


def _label(sess, seg, conn, select_zero=False):
    got = sess.cc_label(_dev(sess, seg), seg.shape, conn, select_zero)
    assert got.dtype == sess.torch.int32 and tuple(got.shape) == tuple(seg.shape if seg.ndim == 3 else seg.shape + (1,))
    return got.cpu().numpy().reshape(seg.shape)


# ------------------------------------------------------------------------------------------------ canonical labels
@pytest.mark.parametrize('select_zero', [False, True])
@pytest.mark.parametrize('conn', pc.CONNS)
@pytest.mark.parametrize('shape', [pc.BOX, pc.SMALL, pc.FLAT])
def test_labels_random_volumes(sess, shape, conn, select_zero):
    for d in pc.DENSITIES:
        seg = pc.random_volume(shape, d)
        np.testing.assert_array_equal(_label(sess, seg, conn, select_zero), pc.host_labels(shape, d, conn, select_zero),
                                      err_msg='density %g' % d)


def test_labels_2d_shape(sess):
    """A [H, W] shape is the volume [H, W, 1]."""
    from nnal_amd import regions
    img = np.array(pc.random_volume(pc.FLAT, 0.35))[:, :, 0]
    for conn in pc.CONNS:
        got = sess.cc_label(_dev(sess, img), img.shape, conn).cpu().numpy()
        np.testing.assert_array_equal(got.reshape(img.shape), regions.cc_label_host(img, conn))


@pytest.fixture(scope='module')
def big():
    from nnal_amd import regions
    seg = pc.random_volume(pc.BIG, 0.35)
    lab = regions.cc_label_host(seg, 26)
    sizes = np.unique(lab[lab >= 0], return_counts=True)[1]
    assert sizes.max() == 366864                                  # the giant of the issue
    return seg, lab


def test_labels_big_volume_and_determinism(sess, big):
    """128 x 128 x 64: far more workgroups than one XCD holds and one giant component that every one of them hooks into;
    every call twice, bit-equal."""
    from nnal_amd import regions
    seg, lab = big
    torch = sess.torch
    d_seg = _dev(sess, seg)
    a = sess.cc_label(d_seg, seg.shape, 26)
    b = sess.cc_label(d_seg, seg.shape, 26)
    assert torch.equal(a, b)
    np.testing.assert_array_equal(a.cpu().numpy(), lab)
    k1, i1 = sess.cc_keep_largest(d_seg, seg.shape, 26, True)
    k2, i2 = sess.cc_keep_largest(d_seg, seg.shape, 26, True)
    assert torch.equal(k1, k2) and i1.tolist() == i2.tolist()
    want, winfo = regions.keep_largest_host(seg, 26, True, with_info=True)
    np.testing.assert_array_equal(k1.cpu().numpy(), want)
    assert i1.tolist() == winfo.tolist() and i1[2] == 366864
    f1, j1 = sess.fill_holes(d_seg, seg.shape)
    f2, j2 = sess.fill_holes(d_seg, seg.shape)
    assert torch.equal(f1, f2) and j1.tolist() == j2.tolist()
    want, winfo = regions.fill_holes_host(seg, with_info=True)
    np.testing.assert_array_equal(f1.cpu().numpy(), want)
    assert j1.tolist() == winfo.tolist()
    z1 = sess.cc_label(d_seg, seg.shape, 6, True)
    z2 = sess.cc_label(d_seg, seg.shape, 6, True)
    assert torch.equal(z1, z2)
    np.testing.assert_array_equal(z1.cpu().numpy(), regions.cc_label_host(seg, 6, True))


def test_labels_built_shapes(sess):
    for name, seg, expected in pc.built_label_cases():
        for conn in pc.CONNS:
            np.testing.assert_array_equal(_label(sess, seg, conn), expected[conn], err_msg='%s, connectivity %d' % (name, conn))


def test_labels_built_shapes_other_polarity(sess):
    """The same built volumes inverted and labelled with select_zero: the same labels."""
    for name, seg, expected in pc.built_label_cases():
        for conn in pc.CONNS:
            np.testing.assert_array_equal(_label(sess, 1 - seg, conn, True), expected[conn], err_msg='%s, connectivity %d' % (name, conn))


def test_labels_nonbinary_values_are_foreground(sess):
    from nnal_amd import regions
    seg = np.array(pc.random_volume(pc.SMALL, 0.2)) * np.random.RandomState(5).randint(1, 256, size=pc.SMALL).astype(np.uint8)
    assert seg.max() > 1
    np.testing.assert_array_equal(_label(sess, seg, 26), regions.cc_label_host(seg, 26))


# ------------------------------------------------------------------------------------------------ keep largest
@pytest.mark.parametrize('shape', [pc.BOX, pc.SMALL, pc.FLAT])
def test_keep_largest_random_volumes(sess, shape):
    from nnal_amd import regions
    for d in pc.DENSITIES:
        seg = pc.random_volume(shape, d)
        for conn in pc.CONNS:
            want, winfo = regions.keep_largest_host(seg, conn, True, with_info=True)
            got, info = sess.cc_keep_largest(_dev(sess, seg), shape, conn, True)
            assert got.dtype == sess.torch.uint8 and info.dtype == np.int64
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg='density %g, connectivity %d' % (d, conn))
            assert info.tolist() == winfo.tolist(), (d, conn)


def test_keep_largest_tie_goes_to_the_first_in_c_order(sess):
    seg = pc.random_volume(pc.SMALL, 0.05)
    lab = pc.host_labels(pc.SMALL, 0.05, 26, False)
    roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
    tied = roots[sizes == sizes.max()]
    assert sizes.max() == 8 and len(tied) == 2
    got, info = sess.cc_keep_largest(_dev(sess, seg), pc.SMALL, 26, True)
    assert info.tolist() == [len(roots), int(tied.min()), 8, int(seg.sum())]
    np.testing.assert_array_equal(got.cpu().numpy(), lab == tied.min())


def _origin_in_giant():
    seg = np.array(pc.random_volume(pc.BOX, 0.35))
    seg[0, 0, :] = 1
    seg[0, :, 0] = 1
    return seg


def test_keep_largest_skip_origin(sess):
    from nnal_amd import regions
    seg = _origin_in_giant()
    lab = regions.cc_label_host(seg, 26)
    roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
    assert roots[np.argmax(sizes)] == 0 and sizes.max() > 9000 and len(roots) > 1        # voxel 0 lies in the giant
    got, info = sess.cc_keep_largest(_dev(sess, seg), pc.BOX, 26, False)
    assert info.tolist() == [len(roots), 0, int(sizes.max()), int(seg.sum())]
    np.testing.assert_array_equal(got.cpu().numpy(), lab == 0)
    got, info = sess.cc_keep_largest(_dev(sess, seg), pc.BOX, 26, True)
    want, winfo = regions.keep_largest_host(seg, 26, True, with_info=True)
    assert winfo[0] == len(roots) - 1 and 0 < winfo[2] < 100 and winfo[1] > 0
    assert info.tolist() == winfo.tolist()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # nothing but the origin's component: no candidate, an all-zero mask
    only = (lab == 0).astype(np.uint8)
    got, info = sess.cc_keep_largest(_dev(sess, only), pc.BOX, 26, True)
    assert info.tolist() == [0, -1, 0, int(only.sum())] and not got.any()
    got, info = sess.cc_keep_largest(_dev(sess, np.zeros(pc.SMALL, dtype=np.uint8)), pc.SMALL, 26, False)
    assert info.tolist() == [0, -1, 0, 0] and not got.any()
    ones = np.ones(pc.SMALL, dtype=np.uint8)
    got, info = sess.cc_keep_largest(_dev(sess, ones), pc.SMALL, 6, False)
    assert info.tolist() == [1, 0, ones.size, ones.size] and got.all()


def test_keep_largest_in_place(sess):
    for shape, d in ((pc.BOX, 0.12), (pc.SMALL, 0.05), (pc.FLAT, 0.35)):
        seg = pc.random_volume(shape, d)
        want, winfo = sess.cc_keep_largest(_dev(sess, seg), shape, 26, True)
        buf = _dev(sess, seg)
        got, info = sess.cc_keep_largest(buf, shape, 26, True, out=buf)
        assert got.data_ptr() == buf.data_ptr() and sess.torch.equal(got.reshape(-1), want.reshape(-1))
        assert info.tolist() == winfo.tolist()


def _guarded(sess, seg, call, guard=64):
    """`call(dims, out pointer, info pointer, work pointer)` with the output in the middle of a larger buffer:
    -> (output, guard bytes in front, guard bytes behind, info)."""
    torch = sess.torch
    sess.bind_stream()
    n = int(seg.size)
    buf = torch.full((guard + n + guard,), 7, dtype=torch.uint8, device=sess.device)
    dims = (C.c_int64 * 3)(*seg.shape)
    work = sess.empty((int(sess.lib.alq_cc_work_bytes(dims)),), torch.uint8)
    info = torch.full((6,), -5, dtype=torch.int64, device=sess.device)
    from nnal_amd._lib import check
    check(call(dims, C.c_void_p(buf.data_ptr() + guard), C.c_void_p(info.data_ptr()), C.c_void_p(work.data_ptr())))
    out = buf.cpu().numpy()
    info = info.cpu().numpy()
    assert info[4] == -5 and info[5] == -5
    return out[guard:-guard].reshape(seg.shape), out[:guard], out[-guard:], info[:4]


def test_outputs_stay_inside_the_callers_buffers(sess):
    from nnal_amd import regions
    for shape, d in ((pc.BOX, 0.2), (pc.SMALL, 0.12), (pc.FLAT, 0.35)):
        seg = pc.random_volume(shape, d)
        d_seg = _dev(sess, seg)
        got, g0, g1, info = _guarded(sess, seg, lambda dims, o, i, w: sess.lib.alq_cc_keep_largest(
            sess.ctx, C.c_void_p(d_seg.data_ptr()), dims, 26, 1, o, i, w))
        want, winfo = regions.keep_largest_host(seg, 26, True, with_info=True)
        np.testing.assert_array_equal(got, want)
        assert info.tolist() == winfo.tolist() and np.all(g0 == 7) and np.all(g1 == 7)
        fseg = pc.fill_volume(shape, 0.75)
        d_fseg = _dev(sess, fseg)
        got, g0, g1, info = _guarded(sess, fseg, lambda dims, o, i, w: sess.lib.alq_fill_holes(
            sess.ctx, C.c_void_p(d_fseg.data_ptr()), dims, o, i, w))
        want, winfo = regions.fill_holes_host(fseg, with_info=True)
        np.testing.assert_array_equal(got, want)
        assert info.tolist() == winfo.tolist() and np.all(g0 == 7) and np.all(g1 == 7)
    # the label volume as well: int32 guard cells around it
    torch = sess.torch
    seg = pc.random_volume(pc.BOX, 0.2)
    d_seg = _dev(sess, seg)
    buf = torch.full((16 + seg.size + 16,), -9, dtype=torch.int32, device=sess.device)
    from nnal_amd._lib import check
    check(sess.lib.alq_cc_label(sess.ctx, C.c_void_p(d_seg.data_ptr()), (C.c_int64 * 3)(*seg.shape), 26, 0, C.c_void_p(buf.data_ptr() + 64)))
    out = buf.cpu().numpy()
    np.testing.assert_array_equal(out[16:-16].reshape(seg.shape), pc.host_labels(pc.BOX, 0.2, 26, False))
    assert np.all(out[:16] == -9) and np.all(out[-16:] == -9)


# ------------------------------------------------------------------------------------------------ fill holes
@pytest.mark.parametrize('shape', [pc.BOX, pc.SMALL])
def test_fill_holes_random_volumes(sess, shape):
    from nnal_amd import regions
    for d in pc.FILL_DENSITIES:
        seg = pc.fill_volume(shape, d)
        want, winfo = regions.fill_holes_host(seg, with_info=True)
        assert winfo[1] > 0                                        # (793, 3913, 2072 voxels on the large box)
        got, info = sess.fill_holes(_dev(sess, seg), shape)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg='density %g' % d)
        assert info.tolist() == winfo.tolist(), d
        buf = _dev(sess, seg)                                      # in place
        got2, info2 = sess.fill_holes(buf, shape, out=buf)
        assert got2.data_ptr() == buf.data_ptr() and sess.torch.equal(got2.reshape(-1), got.reshape(-1))
        assert info2.tolist() == winfo.tolist()


def test_fill_holes_built_shapes(sess):
    for name, seg, want, winfo in pc.built_fill_cases():
        got, info = sess.fill_holes(_dev(sess, seg), seg.shape)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=name)
        assert info.tolist() == winfo, name


def test_fill_holes_one_slice_fills_nothing(sess):
    """S = 1: every voxel lies on a face of the volume, as scipy sees the [H, W, 1] array."""
    from nnal_amd import regions
    seg = np.zeros((9, 9, 1), dtype=np.uint8)
    seg[2:7, 2:7, 0] = 1
    seg[3:6, 3:6, 0] = 0
    got, info = sess.fill_holes(_dev(sess, seg), seg.shape)
    np.testing.assert_array_equal(got.cpu().numpy(), seg)
    np.testing.assert_array_equal(regions.fill_holes_host(seg), seg)
    assert info.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ wrappers, C entry points
def test_wrappers_against_the_reference_restatement(sess):
    from nnal_amd import post_processing as pp, regions
    branches = set()
    for name, seg in pc.wrapper_cases():
        want = pc.reference_cca(seg)
        got = pp.connected_component_analysis_3d(seg, sess)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, want, err_msg=name)
        branches.add((bool(seg[0, 0, 0]), bool(np.array_equal(got, seg == 0))))
        if not seg[0, 0, 0]:
            np.testing.assert_array_equal(got, regions.keep_largest_host(seg))
        t = pp.connected_component_analysis_3d(_dev(sess, seg), sess, seg.shape)
        assert t.dtype == sess.torch.uint8 and t.device == sess.device
        np.testing.assert_array_equal(t.cpu().numpy().reshape(seg.shape), want)
    assert branches == {(False, False), (True, True), (True, False)}
    for d in pc.FILL_DENSITIES:
        seg = pc.fill_volume(pc.SMALL, d)
        got = pp.fill_holes(seg, sess)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, regions.fill_holes_host(seg))
        t = pp.fill_holes(_dev(sess, seg), sess, seg.shape)
        np.testing.assert_array_equal(t.cpu().numpy(), regions.fill_holes_host(seg))
    ones = np.ones(pc.SMALL, dtype=np.uint8)
    with pytest.raises(IndexError):
        pp.connected_component_analysis_3d(ones, sess)              # nothing but the origin's component
    with pytest.raises(IndexError):
        pp.connected_component_analysis_3d(np.zeros(pc.SMALL, dtype=np.uint8), sess)
    two = ones.copy()
    two[3, 3, 3] = 2
    with pytest.raises(ValueError):
        pp.connected_component_analysis_3d(two, sess)
    with pytest.raises(ValueError):
        pp.connected_component_analysis_3d(_dev(sess, two), sess, two.shape)


def test_c_entry_points_refuse_bad_arguments_before_any_launch(sess):
    torch = sess.torch
    sess.bind_stream()
    seg = pc.random_volume(pc.SMALL, 0.2)
    d_seg = _dev(sess, seg)
    dims = (C.c_int64 * 3)(*seg.shape)
    out = torch.full((seg.size,), 7, dtype=torch.uint8, device=sess.device)
    lab = torch.full((seg.size,), -9, dtype=torch.int32, device=sess.device)
    info = torch.full((4,), -5, dtype=torch.int64, device=sess.device)
    work = sess.empty((int(sess.lib.alq_cc_work_bytes(dims)),), torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    L = sess.lib
    for conn in (5, 0, 27):
        assert L.alq_cc_label(sess.ctx, p(d_seg), dims, conn, 0, p(lab)) == -1
        assert L.alq_cc_keep_largest(sess.ctx, p(d_seg), dims, conn, 1, p(out), p(info), p(work)) == -1
    assert L.alq_cc_label(sess.ctx, None, dims, 26, 0, p(lab)) == -1
    assert L.alq_cc_label(sess.ctx, p(d_seg), dims, 26, 0, None) == -1
    assert L.alq_cc_label(sess.ctx, p(d_seg), None, 26, 0, p(lab)) == -1
    for args in ((None, dims, 26, 1, p(out), p(info), p(work)), (p(d_seg), dims, 26, 1, None, p(info), p(work)),
                 (p(d_seg), dims, 26, 1, p(out), None, p(work)), (p(d_seg), dims, 26, 1, p(out), p(info), None)):
        assert L.alq_cc_keep_largest(sess.ctx, *args) == -1
    for args in ((None, dims, p(out), p(info), p(work)), (p(d_seg), dims, None, p(info), p(work)),
                 (p(d_seg), dims, p(out), None, p(work)), (p(d_seg), dims, p(out), p(info), None)):
        assert L.alq_fill_holes(sess.ctx, *args) == -1
    huge = (C.c_int64 * 3)(2048, 2048, 512)      # 2^31 voxels
    assert L.alq_cc_label(sess.ctx, p(d_seg), huge, 26, 0, p(lab)) == -1
    assert L.alq_fill_holes(sess.ctx, p(d_seg), huge, p(out), p(info), p(work)) == -1
    assert L.alq_cc_work_bytes(huge) == 0 and L.alq_cc_work_bytes(dims) == 64 + 8 * seg.size
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((lab == -9).all()) and bool((info == -5).all())      # nothing was launched


# ------------------------------------------------------------------------------------------------ full_model_eval
PSHAPE = (5, 5, 3)
RADS = (2, 2, 1)


@pytest.fixture(scope='module')
def net(sess):
    from nnal_amd import NN
    ld = netspec.net_a()
    in_shape = (5, 5, 6)
    m = NN.CNN(in_shape, ld, 'postproc', None, None, sess=sess, max_batch=128)
    m.set_weights(netspec.he_init(ld, in_shape, seed=93, bias_std=0.2))
    yield m
    m.close()


def _subject():
    """A (16, 14, 6) subject for the `net` fixture, which predicts 1 on an all-zero patch and 0 as soon as a patch holds a
    large value (checked on the CPU oracle: margin 0.014 in the posterior).  One modality is zero but for spikes of 40: at
    (0, 0, 0), so that voxel 0 is background; at (5, 7, 2), which carves a 5 x 5 x 3 cavity of 75 voxels into the foreground,
    closed by slices 0 and 4; on the whole plane i = 12, a wall of background that cuts the plane i = 15 (70 voxels in the
    evaluated slices) off the main body."""
    shp = (16, 14, 6)
    a = np.zeros(shp)
    a[0, 0, 0] = a[5, 7, 2] = 40.
    a[12, :, :] = 40.
    mods = [np.pad(v, [(r, r) for r in RADS], 'constant') for v in (a, np.zeros(shp))]
    mask = np.random.RandomState(1301).randint(0, 2, size=shp).astype(np.float64)
    return mods, mask


def test_full_model_eval_post_process(sess, net, tmp_path):
    from nnal_amd import PW_analyze_results as R, nrrd_io, regions
    mods, mask = _subject()
    expr = Expr({'patch_shape': PSHAPE, 'ntb': 64, 'stats': [[0., 1.], [0., 1.]]}, None)
    slices = [0, 1, 2, 3, 4]
    raw_dir, pp_dir = str(tmp_path / 'raw'), str(tmp_path / 'pp')
    raw, F1_raw = R.full_model_eval(expr, net, sess, mods, mask, slices, save_dir=raw_dir)
    assert sorted(os.listdir(raw_dir)) == ['F1_socre.txt', 'segs.nrrd']             # today's behaviour, untouched
    assert F1_raw == R.F1_scores(raw[:, :, slices], mask[:, :, slices]) and not raw[:, :, 5].any()
    got, F1 = R.full_model_eval(expr, net, sess, mods, mask, slices, save_dir=pp_dir, post_process=True)
    kept, kinfo = regions.keep_largest_host(raw.astype(np.uint8), with_info=True)
    want, finfo = regions.fill_holes_host(kept, with_info=True)
    print('raw positives %d, largest of %d components: %d voxels, %d filled, F1 %r -> %r' % (raw.sum(), kinfo[0], kinfo[2], finfo[1],
                                                                                        F1_raw, F1))
    # both steps changed the volume: the cut-off plane went, the cavity was filled
    assert kinfo[0] == 2 and raw[15].sum() == 70 and not want[15].any() and finfo.tolist() == [1, 75, 0, 0]
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    assert F1 == R.F1_scores(want[:, :, slices].astype(np.float64), mask[:, :, slices]) and F1 != F1_raw
    assert sorted(os.listdir(pp_dir)) == ['F1_socre.txt', 'F1_socre_raw.txt', 'segs.nrrd', 'segs_raw.nrrd']
    segs = nrrd_io.read(os.path.join(pp_dir, 'segs.nrrd'))[0]
    assert segs.dtype == np.uint8
    np.testing.assert_array_equal(segs, want)
    np.testing.assert_array_equal(nrrd_io.read(os.path.join(pp_dir, 'segs_raw.nrrd'))[0], raw.astype(np.uint8))
    assert float(np.loadtxt(os.path.join(pp_dir, 'F1_socre.txt'))) == F1
    assert float(np.loadtxt(os.path.join(pp_dir, 'F1_socre_raw.txt'))) == F1_raw
    again, F1_again = R.full_model_eval(expr, net, sess, mods, mask, slices)
    np.testing.assert_array_equal(again, raw)
    assert F1_again == F1_raw
