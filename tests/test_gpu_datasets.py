"""csrc/volbatch.hip and nnal_amd.datasets on the GPU box.

  * alq_vol_pack / alq_mask_pack: bit-equal to `np.stack([v.transpose(2, 0, 1) for v in vols], -1).astype(np.float32)` for every
    source type, m = 1, 2, 3 (64-row tiles) and 5 (32-row tiles), shapes on either side of the tile edges (64 or 32 rows of
    H W, 32 planes of Z), with and without the four-outputs-a-lane path (H W m % 4, an output one element off alignment).
  * alq_slice_batch: X, labels and counts bit-equal to the NumPy statement (slices of the packed arrays) on the subjects of
    tests/golden/datasets.npz and on synthetic ones; every bad descriptor returns ALQ_EINVAL and writes nothing.
  * The device generators of D3 reproduce the batches the reference's own D3 produced (the golden file) draw for draw;
    `regular`'s reproduce the package's NumPy path (pinned against the reference by tests/test_datasets_host.py).
  * A train step fed (device X, DeviceLabels) against the same step fed (host float32 X, host one-hot): same label vector, same
    count, same scale; loss and weights within the bars of tests/test_gpu_losses.py / test_gpu_mteach.py (2e-5 / 5e-4) - both
    paths run the same kernels on the same numbers, and the test prints whether the bits agree.
Every output of a kernel call lies inside a pattern-filled buffer whose margins must keep their bits."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import datasets_cases as cases  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -4
GUARD = 64
SRC = {np.float32: 0, np.float64: 1, np.int16: 2, np.uint8: 3}
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


@pytest.fixture(scope='module')
def g():
    return cases.golden()


class _Framed(object):
    """n elements, `off` elements past an aligned address, in the middle of a pattern-filled device tensor."""

    def __init__(self, sess, n, dtype, off=0):
        torch = self.torch = sess.torch
        self.fill = {torch.float32: float('nan'), torch.int32: -77, torch.int64: -7, torch.uint8: 0xA5}[dtype]
        self.buf = torch.full((n + 2 * GUARD + off,), self.fill, dtype=dtype, device=sess.device)
        self.lo, self.n, self.dtype = GUARD + off, n, dtype
        self.view = self.buf[self.lo:self.lo + n]
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.lo * self.buf.element_size())

    def _is_fill(self, t):
        torch = self.torch
        if self.dtype == torch.float32:          # by bits: another NaN is a write too
            pat = torch.full((1,), self.fill, dtype=torch.float32, device=t.device).view(torch.int32)
            return bool((t.view(torch.int32) == pat).all())
        return bool((t == self.fill).all())

    def margins_intact(self):
        return self._is_fill(self.buf[:self.lo]) and self._is_fill(self.buf[self.lo + self.n:])

    def untouched(self):
        return self._is_fill(self.buf)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(_bits(got), _bits(want)):
        bad = np.argwhere(_bits(got) != _bits(want))
        raise AssertionError('%s: %d of %d elements differ; first at %s: device %s, statement %s' % (
            name, len(bad), got.size, [tuple(i) for i in bad[:6]], [got[tuple(i)] for i in bad[:6]], [want[tuple(i)] for i in bad[:6]]))


# ------------------------------------------------------------------------------------------ pack
def _pack_statement(vols):
    return np.stack([v.transpose(2, 0, 1) for v in vols], -1).astype(np.float32)


def _vol_pack(sess, vols, off=0):
    torch = sess.torch
    H, W, Z = vols[0].shape
    m = len(vols)
    src = [torch.as_tensor(np.ascontiguousarray(v)).to(sess.device) for v in vols]
    out = _Framed(sess, Z * H * W * m, torch.float32, off)
    sess.bind_stream()
    rc = sess.lib.alq_vol_pack(sess.ctx, (C.c_void_p * m)(*[t.data_ptr() for t in src]), m, SRC[vols[0].dtype.type], (C.c_int32 * 3)(H, W, Z), out.ptr)
    assert rc == 0, sess.lib.alq_last_error()
    assert out.margins_intact(), 'alq_vol_pack: a store outside [Z, H, W, m] for %r m=%d' % ((H, W, Z), m)
    return out.view.reshape(Z, H, W, m).cpu().numpy()


def _mask_pack(sess, mask, off=0):
    torch = sess.torch
    H, W, Z = mask.shape
    src = torch.as_tensor(np.ascontiguousarray(mask)).to(sess.device)
    out = _Framed(sess, Z * H * W, torch.uint8, off)
    sess.bind_stream()
    rc = sess.lib.alq_mask_pack(sess.ctx, C.c_void_p(src.data_ptr()), (C.c_int32 * 3)(H, W, Z), out.ptr)
    assert rc == 0, sess.lib.alq_last_error()
    assert out.margins_intact(), 'alq_mask_pack: a store outside [Z, H, W] for %r' % ((H, W, Z),)
    return out.view.reshape(Z, H, W).cpu().numpy()


def _values(rs, shape, dt):
    if dt is np.uint8:
        return rs.randint(0, 256, size=shape).astype(dt)
    if dt is np.int16:
        return rs.randint(-32768, 32768, size=shape).astype(dt)
    if dt is np.float32:
        return (rs.randn(*shape) * 100).astype(dt)
    # doubles between floats: ties (to the even and to the odd neighbour), just above and just below a tie, large and tiny
    base = rs.randint(1, 2 ** 23, size=shape).astype(np.float64) + 2. ** 23          # 24-bit integers: ulp(float) = 1 ... after / 2: 0.5
    frac = rs.choice(np.array([0., 0.5, 0.5 + 2. ** -20, 0.5 - 2. ** -20, 0.25, 0.75]), size=shape)
    scale = rs.choice(np.array([1., 2. ** -30, 2. ** 40, -1.]), size=shape)
    return (base + frac) * scale


# H W on either side of the 64- and 32-row tiles, Z on either side of the 32-plane tile
PACK_SHAPES = [(5, 7, 3), (4, 4, 1), (3, 5, 65), (1, 129, 2), (5, 13, 3), (8, 8, 33), (3, 11, 32), (16, 4, 6), (12, 10, 7)]


@pytest.mark.parametrize('dt', [np.float32, np.float64, np.int16, np.uint8])
@pytest.mark.parametrize('m', [1, 2, 3, 5])
def test_vol_pack_equals_the_numpy_statement(sess, m, dt):
    rs = np.random.RandomState(100 * m + SRC[dt])
    for shape in PACK_SHAPES:
        vols = [_values(rs, shape, dt) for _ in range(m)]
        want = _pack_statement(vols)
        _same('vol_pack %r m=%d' % (shape, m), _vol_pack(sess, vols), want)
        if (shape[0] * shape[1] * m) % 4 == 0:          # the same through the one-output-a-lane path
            _same('vol_pack %r m=%d, output off alignment' % (shape, m), _vol_pack(sess, vols, off=1), want)


def test_vol_pack_rounds_doubles_to_nearest_even(sess):
    one = np.float64(1.)
    e = 2. ** -24          # half an ulp of floats in [1, 2)
    vals = np.array([one + e, one + 3 * e, one + e + 2. ** -40, one + e - 2. ** -40, one + 3 * e + 2. ** -40, one + 3 * e - 2. ** -40,
                     -(one + e), -(one + 3 * e), 1e-46, 2. ** -149 * 1.5, 16777217., 16777219.])
    want = vals.astype(np.float32)
    assert want[0] == 1. and want[1] == np.float32(1. + 4 * e) and want[2] == np.float32(1. + 2 * e) and want[3] == 1.      # tie down, tie up, up, down
    vol = np.zeros((2, 3, 2))
    vol.reshape(-1)[:] = vals
    _same('rounding', _vol_pack(sess, [vol]), _pack_statement([vol]))


def test_mask_pack_equals_the_numpy_statement(sess):
    rs = np.random.RandomState(7)
    for shape in PACK_SHAPES:
        mask = rs.randint(0, 256, size=shape).astype(np.uint8)
        for off in (0, 1, 3):
            _same('mask_pack %r off %d' % (shape, off), _mask_pack(sess, mask, off), np.ascontiguousarray(mask.transpose(2, 0, 1)))


def test_pack_refusals(sess):
    torch = sess.torch
    src = torch.zeros((24,), dtype=torch.float32, device=sess.device)
    out = _Framed(sess, 24 * 9, torch.float32)
    dims = (C.c_int32 * 3)(2, 3, 4)
    ptrs = lambda m: (C.c_void_p * m)(*[src.data_ptr()] * m)
    sess.bind_stream()
    assert sess.lib.alq_vol_pack(sess.ctx, ptrs(9), 9, 0, dims, out.ptr) == EUNSUPPORTED
    assert sess.lib.alq_vol_pack(sess.ctx, ptrs(1), 0, 0, dims, out.ptr) == EINVAL
    assert sess.lib.alq_vol_pack(sess.ctx, ptrs(1), 1, 4, dims, out.ptr) == EINVAL
    assert sess.lib.alq_vol_pack(sess.ctx, ptrs(1), 1, 0, (C.c_int32 * 3)(2, 0, 4), out.ptr) == EINVAL
    assert sess.lib.alq_vol_pack(sess.ctx, ptrs(1), 1, 0, dims, None) == EINVAL
    assert sess.lib.alq_vol_pack(sess.ctx, (C.c_void_p * 2)(src.data_ptr(), None), 2, 0, dims, out.ptr) == EINVAL
    assert sess.lib.alq_mask_pack(sess.ctx, None, dims, out.ptr) == EINVAL
    sess.synchronize()
    assert out.untouched()


# ------------------------------------------------------------------------------------------ batches
class _Subject(object):
    """A packed subject on the device with the host arrays the statement slices."""

    def __init__(self, sess, vols, ids):
        from nnal_amd.datasets import utils
        self.res = utils.ResidentSubject.pack(sess, vols, ids)
        self.vol = _pack_statement(vols)
        self.ids = None if ids is None else np.ascontiguousarray(ids.transpose(2, 0, 1))
        _same('ResidentSubject.vol', self.res.vol.cpu().numpy(), self.vol)
        if ids is not None:
            _same('ResidentSubject.mask', self.res.mask.cpu().numpy(), self.ids)


@pytest.fixture(scope='module')
def golden_subjects(sess):
    from nnal_amd.datasets import utils
    table, img_addrs, _ = cases.subjects()
    subs = []
    for s in range(4):
        vols = [table[img_addrs[mod][s]] for mod in cases.MODS]
        subs.append(_Subject(sess, vols, utils.mask_class_ids(table['/synthetic/sub%d_mask' % s], np.arange(3))))
    return subs


def _statement(subs, desc, crop, nC):
    z, h, w = crop
    X = np.stack([subs[v].vol[zc - z // 2:zc - z // 2 + z, h0:h0 + h, w0:w0 + w] for v, zc, h0, w0, _ in desc])
    lab = np.stack([subs[v].ids[zc - z // 2:zc - z // 2 + z, h0:h0 + h, w0:w0 + w].astype(np.int32) if L else np.full((z, h, w), -1, np.int32)
                    for v, zc, h0, w0, L in desc])
    lab[lab >= nC] = -1
    return X, lab, cases.counts_of(lab, nC)


def _slice_call(sess, subs, desc, crop, nC, x_off=0, lab_off=0, m=None):
    """alq_slice_batch into framed outputs: (rc, X frame, labels frame, counts frame)."""
    torch = sess.torch
    z, h, w = crop
    b, m = len(desc), subs[0].res.m if m is None else m
    n = b * max(z, 1) * max(h, 1) * max(w, 1)
    X, lab, cnt = _Framed(sess, n * m, torch.float32, x_off), _Framed(sess, n, torch.int32, lab_off), _Framed(sess, max(nC, 0) + 1, torch.int64)
    dims = np.ascontiguousarray([s.res.shape for s in subs], dtype=np.int32)
    d = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 5)
    c = np.ascontiguousarray(crop, dtype=np.int32)
    vols = (C.c_void_p * len(subs))(*[s.res.vol.data_ptr() for s in subs])
    masks = (C.c_void_p * len(subs))(*[s.res.mask.data_ptr() if s.res.mask is not None else None for s in subs])
    sess.bind_stream()
    rc = sess.lib.alq_slice_batch(sess.ctx, vols, masks, dims.ctypes.data_as(I32P), len(subs), m, d.ctypes.data_as(I32P), b, c.ctypes.data_as(I32P),
                                  nC, X.ptr, lab.ptr, cnt.ptr)
    sess.synchronize()
    return rc, X, lab, cnt


def _check_batch(sess, subs, desc, crop, nC, x_off=0, lab_off=0):
    z, h, w = crop
    rc, X, lab, cnt = _slice_call(sess, subs, desc, crop, nC, x_off, lab_off)
    assert rc == 0, sess.lib.alq_last_error()
    tag = 'crop %r, %d samples, C=%d, offsets %d / %d' % (crop, len(desc), nC, x_off, lab_off)
    assert X.margins_intact() and lab.margins_intact() and cnt.margins_intact(), 'a store outside an output: ' + tag
    wX, wlab, wcnt = _statement(subs, desc, crop, nC)
    _same('X, ' + tag, X.view.reshape(wX.shape).cpu().numpy(), wX)
    _same('labels, ' + tag, lab.view.reshape(wlab.shape).cpu().numpy(), wlab)
    _same('counts, ' + tag, cnt.view.cpu().numpy(), wcnt)
    return wlab


def test_slice_batch_on_the_golden_subjects(sess, golden_subjects):
    """Shapes 12x10x6, 9x11x8, 12x10x7, 10x10x6, m = 2, masks in {0, 1, 2, 255}."""
    S = golden_subjects
    # w m = 14 (not a multiple of 4), odd w0 m impossible with m = 2: the odd head comes from the output offsets below
    desc = [(0, 1, 0, 0, 1), (1, 7, 1, 3, 0), (2, 6, 4, 2, 1), (3, 3, 2, 2, 1), (0, 5, 3, 1, 0), (0, 5, 3, 1, 1)]
    for x_off, lab_off in ((0, 0), (1, 0), (2, 1), (3, 3)):
        _check_batch(sess, S, desc, (2, 8, 7), 3, x_off, lab_off)
    # the last valid h0, w0 and both ends of the z window; the same subject twice; subjects of different shapes
    ends = [(0, 1, 4, 2, 1), (0, 5, 4, 2, 1), (1, 1, 1, 3, 1), (1, 7, 1, 3, 1), (2, 6, 4, 2, 1), (3, 5, 2, 2, 1), (3, 1, 0, 0, 0)]
    _check_batch(sess, S, ends, (2, 8, 8), 3)
    # crop == the full slice (subjects 0 and 2), a labelled and an unlabelled sample side by side, odd depth
    lab = _check_batch(sess, [S[0], S[2]], [(0, 3, 0, 0, 1), (1, 5, 0, 0, 0), (1, 1, 0, 0, 1)], (3, 12, 10), 3)
    assert (lab[0] >= 0).any() and (lab[0] < 0).any() and (lab[1] == -1).all()          # out-of-class voxels among the labelled
    # b = 1; z = 1 at the first and the last plane; one class only: the bytes 1 and 2 are no class
    _check_batch(sess, S, [(1, 0, 0, 0, 1)], (1, 9, 11), 3)
    _check_batch(sess, S, [(1, 7, 1, 2, 1)], (1, 5, 3), 1)
    lab = _check_batch(sess, S, [(2, 2, 0, 1, 1), (0, 2, 1, 0, 1)], (2, 3, 9), 2)
    assert (lab == -1).any() and (lab == 1).any()


@pytest.mark.parametrize('m', [1, 3])
def test_slice_batch_unaligned_rows_many_classes_and_the_grid_cap(sess, m):
    """m = 1, 3: w0 m odd and w m no multiple of 4; 12 classes (the LDS counters; up to 8 the waves count by ballots); more rows
    than one sweep of the capped grid and more samples than one launch carries."""
    rs = np.random.RandomState(40 + m)
    subs = []
    for shape in ((20, 9, 9), (18, 7, 11)):
        ids = rs.randint(0, 14, size=shape).astype(np.uint8)
        ids[rs.rand(*shape) < 0.1] = 255
        subs.append(_Subject(sess, [rs.randint(-99, 99, size=shape).astype(np.int16) for _ in range(m)], ids))
    for crop in ((2, 5, 3), (3, 17, 5), (1, 4, 1), (4, 3, 6)):
        z, h, w = crop
        desc = []
        for v, s in enumerate(subs):          # the first and the last window along every axis, and offset 1 (w0 m odd)
            H, W, Z = s.res.shape
            desc += [(v, z // 2, H - h, W - w, 1), (v, Z - z + z // 2, min(1, H - h), min(1, W - w), v), (v, z // 2 + 1, 0, 1, 1)]
        for nC in (12, 8, 9, 254):
            _check_batch(sess, subs, desc, crop, nC, x_off=m % 2)
    trip, per = int(sess.lib.alq_slice_batch_trip_rows()), int(sess.lib.alq_slice_batch_launch_samples())
    b, crop = per + 1, (8, 17, 3)
    assert per * crop[0] * crop[1] > trip                          # the first launch grid-strides; the second takes the last sample
    many = [(i % 2, 4 + i % 2, i % 2, i % 4, int(i % 5 != 0)) for i in range(b)]
    _check_batch(sess, subs, many, crop, 12)
    _check_batch(sess, subs, many, crop, 3)


def test_slice_batch_bad_descriptors_write_nothing(sess, golden_subjects):
    S = golden_subjects
    ok = [(0, 1, 4, 2, 1), (1, 7, 1, 3, 0)]
    crop = (2, 8, 8)
    bad = [(4, 1, 0, 0, 1), (-1, 1, 0, 0, 1), (0, 0, 0, 0, 1), (0, 6, 0, 0, 1), (0, -3, 0, 0, 1), (0, 1, 5, 0, 1), (0, 1, 0, 3, 1),
           (0, 1, -1, 0, 1), (1, 1, 0, -1, 1), (0, 1, 0, 0, 2), (0, 2 ** 31 - 1, 0, 0, 1), (0, 1, 2 ** 31 - 8, 0, 1)]
    for d in bad:
        for desc in ([d] + ok, ok + [d]):
            rc, X, lab, cnt = _slice_call(sess, S, desc, crop, 3)
            assert rc == EINVAL, (d, rc)
            assert X.untouched() and lab.untouched() and cnt.untouched(), d
    for nC in (0, 255, -1):
        rc, X, lab, cnt = _slice_call(sess, S, ok, crop, nC)
        assert rc == EINVAL and X.untouched() and lab.untouched() and cnt.untouched()
    for c in ((0, 8, 8), (2, 0, 8), (2, 8, -1), (2, 13, 8), (2, 8, 12)):
        rc, X, lab, cnt = _slice_call(sess, S, ok, c, 3)
        assert rc == EINVAL and X.untouched() and lab.untouched() and cnt.untouched(), c
    rc, X, lab, cnt = _slice_call(sess, S, ok, crop, 3, m=0)
    assert rc == EINVAL and X.untouched()
    # a labelled sample of a subject without a packed mask
    bare = _Subject(sess, [np.zeros((8, 8, 4), np.float32)], None)
    rc, X, lab, cnt = _slice_call(sess, [bare], [(0, 1, 0, 0, 1)], (2, 8, 8), 3)
    assert rc == EINVAL and X.untouched() and lab.untouched() and cnt.untouched()
    rc, X, lab, cnt = _slice_call(sess, [bare], [(0, 1, 0, 0, 0)], (2, 8, 8), 3)
    assert rc == 0 and (lab.view == -1).all() and cnt.view.cpu().numpy().tolist() == [0, 0, 0, 128]
    from nnal_amd.datasets import utils
    with pytest.raises(ValueError):
        utils.slice_batch(sess, [s.res for s in S], [(0, 6, 0, 0, 1)], crop, 3)


# ------------------------------------------------------------------------------------------ generators
def test_device_d3_generator_gives_the_reference_batches(sess, g):
    from nnal_amd.datasets import DeviceLabels, data_holders
    d3 = cases.holder(data_holders.D3, cases.d3_luv(), sess=sess)
    np.random.seed(int(g['d3_seed']))
    d3.create_train_valid_gens(4, [8, 8, 2], n_labeled_train=2)
    assert d3.train_n_slices == list(g['d3_train_n_slices'])
    for k in range(int(g['d3_batches'])):
        X, Y = d3.train_gen_fn()
        wantX, wantY = g['d3_X_%d' % k], g['d3_Y_%d' % k]
        assert isinstance(Y, DeviceLabels) and X.is_cuda and X.dtype == sess.torch.float32 and Y.labels.dtype == sess.torch.int32
        _same('X of batch %d' % k, X.cpu().numpy(), wantX.astype(np.float32))
        _same('labels of batch %d' % k, Y.labels.cpu().numpy(), cases.labels_of(wantY))
        _same('counts of batch %d' % k, Y.counts, cases.counts_of(cases.labels_of(wantY), 3))
        _same('one-hot of batch %d' % k, np.asarray(Y), wantY)
    assert np.random.rand() == float(g['d3_after'])


@pytest.mark.parametrize('class_labels', [None, [0, 2, 1]])
def test_device_regular_generators_equal_the_numpy_path(sess, class_labels):
    """2-D batches [b, h, w, m] (the slice itself), training with and without a fixed labelled share,
    validation 'random' (uniform slice draws) and 'full'; identity and mapped class labels."""
    from nnal_amd.datasets import data_holders
    luv = [np.array([0, 1]), np.array([2]), np.array([1, 0])]
    host = cases.holder(data_holders.regular, luv, class_labels=class_labels)
    dev = cases.holder(data_holders.regular, luv, class_labels=class_labels, sess=sess)
    for mode, nl in (('random', None), ('full', 2)):
        outs = []
        for dat in (host, dev):
            np.random.seed(17)
            dat.create_train_valid_gens(4, [8, 8], valid_mode=mode, n_labeled_train=nl)
            outs.append([dat.train_gen_fn() for _ in range(3)] + [dat.valid_gen_fn() for _ in range(3)] + [np.random.rand()])
        assert outs[0][-1] == outs[1][-1]
        for k, ((Xh, Yh), (Xd, Yd)) in enumerate(zip(outs[0][:-1], outs[1][:-1])):
            _same('X %s %d' % (mode, k), Xd.cpu().numpy(), Xh.astype(np.float32))
            _same('Y %s %d' % (mode, k), np.asarray(Yd), Yh)
            assert Yd.counts.tolist() == cases.counts_of(cases.labels_of(Yh), 3).tolist()


# ------------------------------------------------------------------------------------------ train steps
def _model(sess, tag, c, **hy):
    from nnal_amd import NN_extended, netspec
    ld, sk = netspec.net_c_2d_dense(c)
    pars = netspec.he_init(ld, (8, 8, 2), seed=91, skips=sk, bias_std=0.05)
    m = NN_extended.CNN((8, 8, 2), ld, tag, list(sk), sess=sess, max_batch=8, **hy)
    m.set_weights(pars)
    m.get_optimizer()
    return m


def _spy_scales(monkeypatch, lib, log):
    for name in ('alq_param_grads_loss', 'alq_param_grads_loss_mt'):
        fn = getattr(lib, name)

        def wrapped(*args, _fn=fn, _name=name):
            log.append((_name, args[5]))
            return _fn(*args)
        monkeypatch.setattr(lib, name, wrapped)


STEP_CASES = {
    'sgd_c3': (3, dict(learning_rate=0.05), 2e-5),
    'sgd_c2_class_weights': (2, dict(learning_rate=0.05, bin_class_weights=[0., 1.7]), 2e-5),
    'adam_c3': (3, dict(learning_rate=0.01, optimizer_name='Adam'), 5e-4),
    'mean_teacher_c3': (3, dict(learning_rate=0.05, MT_SSL=True, output_perturbation_measure='L2', max_cons_coeff=5., rampup_length=2,
                                Gaussian_noise_std=0.1, MT_ema_decay_schedule=lambda t: 0.9), 2e-5),
}


@pytest.mark.parametrize('case', sorted(STEP_CASES))
def test_step_fed_from_the_device_equals_the_step_fed_from_the_host(sess, case, monkeypatch):
    from nnal_amd.datasets import data_holders
    c, hy, bar = STEP_CASES[case]
    dat = cases.holder(data_holders.regular, [np.array([0, 1]), np.array([2, 3]), np.array([], dtype=int)], sess=sess, class_labels=np.arange(c))
    np.random.seed(23)
    dat.create_train_valid_gens(6, [8, 8], n_labeled_train=3)
    md, mh = _model(sess, case + '_dev', c, **hy), _model(sess, case + '_host', c, **hy)
    log = []
    _spy_scales(monkeypatch, md.lib, log)
    equal_bits = True
    for step in range(2):
        Xd, Yd = dat.train_gen_fn()
        Xh, Yh = Xd.cpu().numpy(), np.asarray(Yd)
        assert Xh.dtype == np.float32 and Yh.shape == (6, 8, 8, c)
        lab_h = cases.labels_of(Yh)
        _same('label vector', Yd.labels.cpu().numpy(), lab_h)
        w = (lab_h >= 0).astype(np.float64)
        if 'bin_class_weights' in hy:
            w = w * np.asarray(hy['bin_class_weights'], np.float32)[np.where(lab_h == 1, 1, 0)]
        assert md._count_from_class_counts(Yd.counts, md._obj['class_w']) == int(np.count_nonzero(w)) > 0
        losses = []
        for m, X, Y in ((md, Xd, Yd), (mh, Xh, Yh)):
            np.random.seed(300 + step)          # the draws of a mean-teacher step (noise seed)
            n0 = len(log)
            losses.append(sess.run(m.train_step, feed_dict={m.x: X, m.y_: Y, m.keep_prob: 1.}))
            if hy.get('MT_SSL'):
                sess.run(m.ema_apply)
            assert len(log) == n0 + 1
        assert log[-2] == log[-1], 'the scale of the labelled term differs: %r' % (log[-2:],)
        assert abs(losses[0] - losses[1]) <= 2e-5 * max(1., abs(losses[1])), losses
        equal_bits = equal_bits and losses[0] == losses[1]
    pairs = [(md, mh)] + ([(md.teacher, mh.teacher)] if hy.get('MT_SSL') else [])
    for a, b_ in pairs:
        pa, pb = a.flat_params(), b_.flat_params()
        assert np.abs(pa - pb).max() <= bar * max(1., np.abs(pb).max())
        equal_bits = equal_bits and np.array_equal(_bits(pa), _bits(pb))
    print('%s: losses and weights of the two feeds agree bit for bit: %s' % (case, equal_bits))
    # the loss alone, and a shape that does not fit
    Xd, Yd = dat.train_gen_fn()

    def loss_of(feed):
        np.random.seed(77)          # (a mean-teacher loss draws the seed of its noise)
        feed = dict(feed)
        feed[md.keep_prob] = 1.
        return sess.run(md.loss, feed_dict=feed)
    l_dev = loss_of({md.x: Xd, md.y_: Yd})
    l_host = loss_of({md.x: Xd.cpu().numpy(), md.y_: np.asarray(Yd)})
    assert abs(l_dev - l_host) <= 2e-5 * max(1., abs(l_host))
    # per-voxel weights keep the host logic (the labels come back once)
    vw = (0.25 + np.random.RandomState(3).rand(6, 8, 8)).astype(np.float32)
    vw[0, :2] = 0
    l_dev = loss_of({md.x: Xd, md.y_: Yd, md.input_vox_weights: vw})
    l_host = loss_of({md.x: Xd.cpu().numpy(), md.y_: np.asarray(Yd), md.input_vox_weights: vw})
    assert abs(l_dev - l_host) <= 2e-5 * max(1., abs(l_host))
    with pytest.raises(ValueError):
        sess.run(md.train_step, feed_dict={md.x: Xd[:5], md.y_: Yd, md.keep_prob: 1.})
    for m in (md, mh):
        if hy.get('MT_SSL'):
            m.teacher.close()
        m.close()


def test_fc_head_models_do_not_take_device_labels(sess):
    from nnal_amd import NN_extended, netspec
    from nnal_amd.datasets import DeviceLabels
    ld, sk = netspec.net_c_2d(2)
    m = NN_extended.CNN((8, 8, 2), ld, 'fc_head', list(sk), sess=sess, max_batch=8, learning_rate=0.01)
    m.set_weights(netspec.he_init(ld, (8, 8, 2), seed=3, skips=sk, bias_std=0.05))
    m.get_optimizer()
    x = sess.torch.zeros((4, 8, 8, 2), dtype=sess.torch.float32, device=sess.device)
    dl = DeviceLabels(sess.torch.zeros((4,), dtype=sess.torch.int32, device=sess.device), 2, [4, 0, 0])
    with pytest.raises(TypeError):
        sess.run(m.train_step, feed_dict={m.x: x, m.y_: dl, m.keep_prob: 1.})
    m.close()


def test_train_loop_on_device_generators_uploads_no_batch(sess, tmp_path, monkeypatch):
    """model.train for four steps on the device generators of `regular` with a metric generator: the files of the loop test of
    tests/test_gpu_mteach.py, and no array of the size of x, of the labels or of the one-hot goes through sess.to_device."""
    from nnal_amd.datasets import DeviceLabels, data_holders
    dat = cases.holder(data_holders.regular, [np.array([0]), np.array([2]), np.array([1])], sess=sess)
    np.random.seed(29)
    b = 4
    dat.create_train_valid_gens(b, [8, 8], valid_mode='random', n_labeled_train=2)
    m = _model(sess, 'loop_ds', 3, MT_SSL=True, output_perturbation_measure='L2', Gaussian_noise_std=0.05, learning_rate=0.01)
    X, Y = dat.valid_gen_fn()
    assert isinstance(Y, DeviceLabels) and X.shape == (1, 8, 8, 2)          # one validation subject: batches of one slice
    uploads = []
    to_device = sess.to_device

    def counting(arr, dtype):
        uploads.append(int(np.size(arr)))
        return to_device(arr, dtype)
    monkeypatch.setattr(sess, 'to_device', counting)
    m.train(sess, 4, dat.train_gen_fn, [[['av_loss', 'F1'], dat.valid_gen_fn, 2, 'F1']], eval_step=2, save_path=str(tmp_path))
    monkeypatch.undo()
    batch_sizes = {n * 64 * k for n in (1, b) for k in (1, 2, 3)}          # labels, x, one-hot of a validation or a training batch
    assert not batch_sizes & set(uploads), (sorted(batch_sizes), uploads)
    assert m.global_step == 4
    files = set(os.listdir(str(tmp_path)))
    ext = '.h5' if 'model_pars.h5' in files else '.npz'
    assert {'av_loss_0.txt', 'F1_0.txt', 'model_pars' + ext, 'teacher_pars' + ext} <= files
    assert len(m.valid_metrics_0['av_loss']) == 2 and len(m.valid_metrics_0['F1']) == 2
    assert len(np.loadtxt(str(tmp_path / 'F1_0.txt'))) == 2
    assert not np.array_equal(m.teacher.flat_params(), m.flat_params())
    m.teacher.close()
    m.close()
