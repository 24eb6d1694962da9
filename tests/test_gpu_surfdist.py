"""The surface-distance calls of csrc/edt.hip on the device against their NumPy statements (nnal_amd.surfdist): alq_surface_mask
and alq_edt_sq to equality at tile edges and at the longest axis, the masked reductions on synthetic values (exact, except the
sum of square roots, which has a written bound), surface_distances / eval_full_segs_surface_distances end to end, refusals.
Every output is followed by a guard tile that must come back untouched, and every call is made twice: same bits."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GUARD = 64
SPACINGS = [(1., 1., 1.), (1., 1., 3.), (0.7, 0.9, 2.2), (1e-3, 1e3, 1.)]


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _geometry(dims):
    from nnal_amd import _lib
    out = (C.c_int32 * 4)()
    rc = _lib.lib().alq_edt_geometry((C.c_int64 * 3)(*dims), out)
    return rc, list(out)


def _max_axis():
    from nnal_amd import _lib
    return int(_lib.lib().alq_edt_max_axis())


def _tz():
    rc, g = _geometry((3, 2, 64))
    assert rc == 0
    return g[1]


def _shapes():
    T, M = _tz(), _max_axis()
    return [(1, 1, 1), (1, 1, T - 1), (1, 1, T), (1, 1, T + 1), (3, 2, T - 1), (3, 2, T), (3, 2, T + 1), (3, 1, T + 1), (5, 1, 7),
            (1, 20, 33), (13, 9, 17), (40, 37, 21), (9, 14, 1), (37, 1, 1), (300, 9, 1), (M, 2, 3), (2, M, 3), (2, 3, M)]


class Guarded(object):
    """A device buffer of n elements followed by a guard tile (NaN for float64, 0xFF for uint8) that must stay as it is."""

    def __init__(self, sess, n, dtype):
        torch = sess.torch
        self.fill = float('nan') if dtype == torch.float64 else 0xFF
        self.buf = torch.full((n + GUARD,), self.fill, dtype=dtype, device=sess.device)
        self.n = n
        self.out = self.buf[:n]

    def check(self):
        g = self.buf[self.n:].cpu().numpy()
        assert np.all(np.isnan(g)) if self.fill != 0xFF else np.all(g == 0xFF), 'guard tile overwritten'
        return self.out.cpu().numpy()


def _feature_sets(shape, seed):
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    none, full = np.zeros(shape, np.uint8), np.ones(shape, np.uint8)
    corner = none.copy()
    corner.flat[n - 1] = 1
    ties = none.copy()          # two voxels at the ends of the longest axis: its middle outputs are equidistant from both
    ax = int(np.argmax(shape))
    lo, hi = [0, 0, 0], [0, 0, 0]
    hi[ax] = shape[ax] - 1
    ties[tuple(lo)] = 1
    ties[tuple(hi)] = 1
    return [('none', none), ('all', full), ('corner', corner), ('ties', ties), ('2%', (rng.rand(*shape) < 0.02).astype(np.uint8) * 7),
            ('50%', (rng.rand(*shape) < 0.5).astype(np.uint8))]


def _edt_twice(sess, feat, spacing):
    torch = sess.torch
    d_feat = sess.to_device(feat, torch.uint8)
    res = []
    for _ in range(2):
        g = Guarded(sess, feat.size, torch.float64)
        sess.edt_sq(d_feat, feat.shape, spacing, out=g.out)
        res.append(g.check().reshape(feat.shape))
    np.testing.assert_array_equal(res[0], res[1])
    return res[0]


@pytest.mark.parametrize('shape', _shapes(), ids=lambda s: 'x'.join(str(v) for v in s))
def test_edt_sq_equals_the_statement(sess, shape):
    from nnal_amd import surfdist
    T, M = _tz(), _max_axis()
    rc, geo = _geometry(shape)
    assert rc == 0 and min(geo) >= 0
    H, W, S = shape
    # every case is in the regime it claims
    assert geo[1] <= T and geo[0] >= 1
    if max(H, W) == M:
        assert geo[1] * M * 8 <= 64 * 1024 and 1 <= geo[1] < T      # the longest strided line: a narrower tile, within the LDS asked for
    if S == M:
        assert geo[0] * M * 8 <= 64 * 1024 and geo[2] == H * W // geo[0]
    if shape == (40, 37, 21):
        assert geo[2] > 1 and geo[3] == H                   # several line tiles in the z pass; the w pass has one tile per h
    if shape[:2] == (3, 2):
        assert geo[1] == T and geo[3] == (3 * (2 if S > T else 1))      # S = T + 1: a second, one-column tile per h
    for si, spacing in enumerate(SPACINGS):
        for name, feat in _feature_sets(shape, 100 + si):
            got = _edt_twice(sess, feat, spacing)
            want = surfdist.edt_sq_host(feat, spacing)
            np.testing.assert_array_equal(got, want, err_msg='%s %r' % (name, spacing))
            if name == 'none':
                assert np.all(np.isposinf(got))
            if name == 'all':
                assert not got.any()


@pytest.mark.parametrize('shape', _shapes(), ids=lambda s: 'x'.join(str(v) for v in s))
def test_surface_mask_equals_the_statement(sess, shape):
    from nnal_amd import surfdist
    torch = sess.torch
    rng = np.random.RandomState(sum(shape))
    seg = rng.randint(0, 4, size=shape).astype(np.uint8)
    single = np.zeros(shape, np.uint8)
    single.flat[int(np.prod(shape)) // 2] = 3
    for name, vol, label in (('0..3, any', seg, -1), ('0..3, == 2', seg, 2), ('full', np.ones(shape, np.uint8), -1), ('single', single, -1),
                             ('single, == 3', single, 3), ('single, == 1', single, 1)):
        d_vol = sess.to_device(vol, torch.uint8)
        res = []
        for _ in range(2):
            g = Guarded(sess, vol.size, torch.uint8)
            sess.surface_mask(d_vol, shape, label, out=g.out)
            res.append(g.check().reshape(shape))
        np.testing.assert_array_equal(res[0], res[1])
        np.testing.assert_array_equal(res[0], surfdist.surface_host(vol, label).astype(np.uint8), err_msg=name)
    if shape == (1, 1, 1):
        assert not res[0].any()


# ---- the masked reductions on synthetic values ------------------------------------------------------------------------------
def _masked_sizes():
    from nnal_amd import _lib
    out = (C.c_int32 * 2)()
    assert _lib.lib().alq_masked_geometry(1 << 30, out) == 0
    per_wg, max_wg = int(out[0]), int(out[1])
    first_twice = per_wg * max_wg + 1          # the first n at which a grid-stride loop iterates twice
    assert _lib.lib().alq_masked_geometry(first_twice, out) == 0 and int(out[1]) == max_wg
    assert _lib.lib().alq_masked_geometry(first_twice - 1, out) == 0 and int(out[1]) * per_wg == first_twice - 1
    return [1, per_wg - 1, per_wg, per_wg + 1, first_twice]


def _values(n, seed, with_inf):
    rng = np.random.RandomState(seed)
    pool = np.array([0., 5e-324, 1e300, 0.25, 0.25, 2., 2., 2., 1e-10] + ([np.inf] if with_inf else []))
    v = np.where(rng.rand(n) < 0.5, pool[rng.randint(0, len(pool), size=n)], rng.rand(n) * 50.)
    return v.astype(np.float64)


def _mask(n, kind, seed):
    rng = np.random.RandomState(seed)
    if kind == 'empty':
        return np.zeros(n, np.uint8)
    if kind == 'full':
        return np.full(n, 3, np.uint8)
    return (rng.rand(n) < (0.03 if kind == 'sparse' else 0.9)).astype(np.uint8)


def _raw_stats(sess, d2, mask):
    torch = sess.torch
    n, work = sess._masked_args(d2, mask)
    g = Guarded(sess, 4, torch.float64)
    rc = sess.lib.alq_masked_dist_stats(sess.ctx, C.c_void_p(d2.data_ptr()), C.c_void_p(mask.data_ptr()), n, C.c_void_p(g.out.data_ptr()),
                                        C.c_void_p(work.data_ptr()))
    assert rc == 0, sess.lib.alq_last_error()
    return g.check()


def _raw_select(sess, d2, mask, ranks):
    torch = sess.torch
    n, work = sess._masked_args(d2, mask)
    g = Guarded(sess, len(ranks), torch.float64)
    rc = sess.lib.alq_masked_select(sess.ctx, C.c_void_p(d2.data_ptr()), C.c_void_p(mask.data_ptr()), n, (C.c_int64 * len(ranks))(*ranks),
                                    len(ranks), C.c_void_p(g.out.data_ptr()), C.c_void_p(work.data_ptr()))
    assert rc == 0, sess.lib.alq_last_error()
    return g.check()


@pytest.mark.parametrize('n', _masked_sizes())
def test_masked_stats_and_select(sess, n):
    from nnal_amd import surfdist
    torch = sess.torch
    for ki, kind in enumerate(('empty', 'full', 'sparse', 'dense')):
        for with_inf in (False, True):
            v, m = _values(n, 10 * ki + with_inf, with_inf), _mask(n, kind, ki)
            d_v, d_m = sess.to_device(v, torch.float64), sess.to_device(m, torch.uint8)
            want = surfdist.dist_stats_host(v, m)
            got = _raw_stats(sess, d_v, d_m)
            np.testing.assert_array_equal(got, _raw_stats(sess, d_v, d_m))
            np.testing.assert_array_equal(got, sess.masked_dist_stats(d_v, d_m))
            np.testing.assert_array_equal(got[[0, 2, 3]], want[[0, 2, 3]])          # count, max, min: exact
            count = int(want[0])
            if np.isinf(want[1]):
                assert got[1] == np.inf                                              # a masked +inf: exactly inf
            else:
                # 1 ulp per device square root + the summation-order bound
                bound = (n + 2) * EPS * want[1]
                err = abs(got[1] - want[1])
                print('n=%d %s: sum err / bound = %.3f' % (n, kind, err / bound if bound else 0.))
                assert err <= bound
            if count == 0:
                assert got[1] == 0. and got[2] == -np.inf and got[3] == np.inf
            eight = sorted(set(int(r) for r in np.linspace(0, max(count - 1, 0), 7))) + [count, count + 3]
            eight = (eight + [0] * 8)[:8]
            for ranks in ([0], [max(count - 1, 0)], [max(count - 1, 0) // 2, count // 2], eight, [count], [count + (1 << 40)]):
                sel = _raw_select(sess, d_v, d_m, ranks)
                ref = surfdist.select_host(v, m, ranks)
                np.testing.assert_array_equal(sel, ref)                              # NaN positions compare equal here
                np.testing.assert_array_equal(sel, _raw_select(sess, d_v, d_m, ranks))
                np.testing.assert_array_equal(sel, sess.masked_select(d_v, d_m, ranks))
                assert all(np.isnan(s) == (r >= count) for s, r in zip(sel, ranks))


def test_select_inside_runs_of_duplicates(sess):
    """Runs of equal values that span the asked ranks, and values that differ in the lowest digit only."""
    from nnal_amd import surfdist
    torch = sess.torch
    base = np.float64(3.)
    v = np.concatenate([np.full(400, 1.), np.full(300, base), np.nextafter(base, np.inf) * np.ones(5), np.full(295, 9.), [np.inf] * 24])
    np.random.RandomState(0).shuffle(v)
    m = np.ones(v.size, np.uint8)
    d_v, d_m = sess.to_device(v, torch.float64), sess.to_device(m, torch.uint8)
    ranks = [399, 400, 699, 700, 704, 705, 999, 1023]
    sel = _raw_select(sess, d_v, d_m, ranks)
    np.testing.assert_array_equal(sel, surfdist.select_host(v, m, ranks))
    np.testing.assert_array_equal(sel, [1., 3., 3., np.nextafter(base, np.inf), np.nextafter(base, np.inf), 9., 9., np.inf])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _box(shape, lo, size):
    a = np.zeros(shape, dtype=np.uint8)
    a[tuple(slice(l, l + size) for l in lo)] = 1
    return a


def _blobs(shape, seed, p=0.01, grow=2):
    return ndimage.binary_dilation(np.random.RandomState(seed).rand(*shape) < p, iterations=grow).astype(np.uint8)


def _same_metrics(dev, host):
    assert set(dev) == set(host)
    n = host['n_seg'] + host['n_mask']
    for k in ('HD', 'n_seg', 'n_mask', 'max_seg_to_mask', 'max_mask_to_seg', 'percentile_seg_to_mask', 'percentile_mask_to_seg'):
        assert dev[k] == host[k], (k, dev[k], host[k])          # exact maxima, counts and selected order statistics
    assert abs(dev['HD95'] - host['HD95']) <= 8 * EPS * host['HD95'] or dev['HD95'] == host['HD95']
    for k in ('ASSD', 'MHD', 'mean_seg_to_mask', 'mean_mask_to_seg'):
        if np.isinf(host[k]):
            assert dev[k] == host[k], k
        else:
            bound = (n + 2) * EPS * host[k]
            print('%s: err / bound = %.3f' % (k, abs(dev[k] - host[k]) / bound if bound else 0.))
            assert abs(dev[k] - host[k]) <= bound, k


def test_surface_distances_end_to_end(sess):
    from nnal_amd import surfdist
    torch = sess.torch
    a, b, e = _box((12, 10, 9), (2, 3, 2), 4), _box((12, 10, 9), (5, 3, 2), 4), np.zeros((12, 10, 9), np.uint8)
    res = surfdist.surface_distances(a, b, (2., 1., 1.), sess=sess)
    assert res['HD'] == 6.0
    _same_metrics(res, surfdist.surface_distances(a, b, (2., 1., 1.)))
    res = surfdist.surface_distances(a, a, sess=sess)
    assert all(res[k] == 0. for k in ('HD', 'HD95', 'ASSD', 'MHD'))
    for x, y in ((a, e), (e, a)):
        res = surfdist.surface_distances(x, y, sess=sess)
        assert all(res[k] == np.inf for k in ('HD', 'HD95', 'ASSD', 'MHD'))
    res = surfdist.surface_distances(e, e, sess=sess)
    assert all(res[k] == 0. for k in ('HD', 'HD95', 'ASSD', 'MHD'))
    _same_metrics(surfdist.surface_distances(a[:, :, 3], b[:, :, 3], (2., 1.), sess=sess), surfdist.surface_distances(a[:, :, 3], b[:, :, 3], (2., 1.)))
    seg, mask = _blobs((40, 37, 21), 1), _blobs((40, 37, 21), 2)
    for q in (95., 50.):
        host = surfdist.surface_distances(seg, mask, (0.5, 0.5, 3.), percentile=q)
        dev = surfdist.surface_distances(seg, mask, (0.5, 0.5, 3.), percentile=q, sess=sess)
        _same_metrics(dev, host)
        assert 0 < host['ASSD'] <= host['MHD'] <= host['HD']
    # device tensors are read in place and give the same result as arrays
    d_seg, d_mask = sess.to_device(seg, torch.uint8), sess.to_device(mask, torch.uint8)
    assert surfdist.surface_distances(d_seg, d_mask, (0.5, 0.5, 3.), sess=sess) == surfdist.surface_distances(seg, mask, (0.5, 0.5, 3.), sess=sess)
    flat = surfdist.surface_distances(d_seg.reshape(-1), d_mask.reshape(-1), (0.5, 0.5, 3.), sess=sess, shape=seg.shape)
    assert flat == surfdist.surface_distances(seg, mask, (0.5, 0.5, 3.), sess=sess)
    np.testing.assert_array_equal(d_seg.cpu().numpy(), seg)


def test_eval_full_segs_surface_distances_with_a_session(sess):
    from nnal_amd import eval_utils
    rng = np.random.RandomState(4)
    segs, masks = [], []
    for i in range(2):
        m = _blobs((24, 20, 11), 30 + i, p=0.02) * rng.randint(1, 3, size=(24, 20, 11)).astype(np.uint8)
        s = m.copy()
        s[rng.rand(*s.shape) < 0.03] = 2
        segs.append(s)
        masks.append(m)
    host = eval_utils.eval_full_segs_surface_distances(segs, masks, spacings=(0.5, 0.5, 3.), labels=[1, 2])
    dev = eval_utils.eval_full_segs_surface_distances(segs, masks, spacings=(0.5, 0.5, 3.), labels=[1, 2], sess=sess)
    assert host['HD'].shape == (2, 2)
    for i in range(2):
        for j in range(2):
            _same_metrics({k: v[i, j] for k, v in dev.items()}, {k: v[i, j] for k, v in host.items()})
    host = eval_utils.eval_full_segs_surface_distances(segs, masks)
    dev = eval_utils.eval_full_segs_surface_distances(segs, masks, sess=sess)
    for i in range(2):
        _same_metrics({k: v[i] for k, v in dev.items()}, {k: v[i] for k, v in host.items()})


def test_refusals_before_any_launch(sess):
    lib = sess.lib
    t = sess.torch.zeros((64,), dtype=sess.torch.float64, device=sess.device)
    p, q = C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr() + 256)
    sess.bind_stream()
    M = int(lib.alq_edt_max_axis())
    assert M >= 512
    one = (C.c_double * 3)(1., 1., 1.)
    out4 = (C.c_int32 * 4)()

    def dims(*v):
        return (C.c_int64 * 3)(*v)
    for bad in ((0, 3, 3), (3, 0, 3), (3, 3, 0), (M + 1, 2, 2), (2, M + 1, 2), (2, 2, M + 1), (1 << 11, 1 << 10, 1 << 10)):
        assert lib.alq_edt_sq(sess.ctx, p, dims(*bad), one, q, p) in (-4, -1), bad
        assert lib.alq_edt_work_bytes(dims(*bad)) == 0
        assert lib.alq_edt_geometry(dims(*bad), out4) == -4 and list(out4) == [-1] * 4
        if max(bad) != M + 1:          # (the surface mask has no axis limit: such a call would run)
            assert lib.alq_surface_mask(sess.ctx, p, dims(*bad), -1, q) in (-4, -1), bad
    assert lib.alq_edt_work_bytes(dims(2, 2, M)) > 0
    for s in (0., -1., float('inf'), float('nan')):
        for k in range(3):
            sp = [1., 1., 1.]
            sp[k] = s
            assert lib.alq_edt_sq(sess.ctx, p, dims(2, 2, 2), (C.c_double * 3)(*sp), q, p) == -1
            assert b'spacing2' in lib.alq_last_error()
    assert lib.alq_edt_sq(sess.ctx, None, dims(2, 2, 2), one, q, p) == -1
    assert lib.alq_edt_sq(sess.ctx, p, dims(2, 2, 2), one, None, p) == -1
    assert lib.alq_edt_sq(sess.ctx, p, dims(2, 2, 2), one, q, None) == -1
    assert lib.alq_edt_sq(None, p, dims(2, 2, 2), one, q, p) == -1
    assert lib.alq_surface_mask(sess.ctx, p, dims(2, 2, 2), -1, p) == -1 and b'd_seg' in lib.alq_last_error()
    assert lib.alq_surface_mask(sess.ctx, None, dims(2, 2, 2), -1, q) == -1
    assert lib.alq_surface_mask(sess.ctx, p, dims(2, 2, 2), -1, None) == -1
    assert lib.alq_surface_mask(sess.ctx, p, dims(2, 2, 2), 256, q) == -1
    ranks = (C.c_int64 * 9)(*range(9))
    assert lib.alq_masked_select(sess.ctx, p, q, 8, ranks, 9, p, q) == -1 and b'R = 9' in lib.alq_last_error()
    assert lib.alq_masked_select(sess.ctx, p, q, 8, ranks, 0, p, q) == -1
    assert lib.alq_masked_select(sess.ctx, p, q, 8, (C.c_int64 * 2)(1, -1), 2, p, q) == -1 and b'negative' in lib.alq_last_error()
    assert lib.alq_masked_select(sess.ctx, p, q, 1 << 31, ranks, 2, p, q) == -4
    assert lib.alq_masked_select(sess.ctx, None, q, 8, ranks, 2, p, q) == -1
    assert lib.alq_masked_select(sess.ctx, p, q, 8, None, 2, p, q) == -1
    assert lib.alq_masked_select(sess.ctx, p, q, 8, ranks, 2, p, None) == -1
    assert lib.alq_masked_dist_stats(sess.ctx, p, q, 1 << 31, p, q) == -4
    assert lib.alq_masked_dist_stats(sess.ctx, p, q, -1, p, q) == -4
    assert lib.alq_masked_dist_stats(sess.ctx, p, None, 8, p, q) == -1
    assert lib.alq_masked_dist_stats(sess.ctx, p, q, 8, None, q) == -1
    assert lib.alq_masked_work_bytes(1 << 31) == 0 and lib.alq_masked_work_bytes(-1) == 0 and lib.alq_masked_work_bytes(5) > 0
    sess.torch.cuda.synchronize()
    assert not t.cpu().numpy().any()          # nothing was launched on the dummy buffer
