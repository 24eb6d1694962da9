"""Slice queries on the device (csrc/sliceq.hip, nnal_amd/slice_query.py; GPU box).

Kernels alone: alq_unc_accumulate and alq_slice_scores on arrays the test builds, against slice_query.slice_scores_host on the
same arrays.  Counts are equal as integers; sums obey, per slice,
    |device - host| <= (m + 8) 2^-52 abs_sums,        m = n c (entropy, MC-entropy), n (c T + c) (BALD), n (mean) for n ROI voxels
- the a-priori bound of an m-term fp64 sum in any order plus a few ulp per term for log, the product and / T on either side
(tests/slice_query_ref.py: bound; HIP documents 1 ulp for the double log, so the per-term constant is not widened).  An fp32
evaluation of any term misses it by seven orders of magnitude.

Through the model: netspec.net_c_2d_dense at (16, 16, 2) with a dropout layer, and an AU_4U model with the c + 1 head, on 9
slices; the restatement is fed the maps the device passes themselves produced (slice_query.device_slice_sums(tap=...)).
The query runs on the subjects of tests/datasets_cases.py, whose slices are 12 x 10: NET-C's two pooling levels do not divide
that, so the query test uses a two-layer dense model (3x3 conv with dropout, 1x1 head) of that input shape."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import datasets_cases as cases  # noqa: E402
from tests import slice_query_ref as ref  # noqa: E402

VS = [1, 63, 65, 16 * 16, 37 * 41]
NS = [1, 3, 7]
CS = [2, 3, 8]
TS = [1, 2, 10]
ROIS = ['none', 'random', 'empty slice', 'single voxel']


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _check(sess, kind, P=None, roi=None, au=None, tag=''):
    """One device evaluation against the restatement; returns the device sums."""
    from nnal_amd import slice_query
    want, wcnt, mag = slice_query.slice_scores_host(P, kind, roi=roi, au=au)
    got, gcnt, guards = ref.device_scores(sess, kind, P=P, roi=roi, au=au)
    c, T = (2, 1) if kind == 'AU' else (P.shape[-3], P.shape[0] if P.ndim == 4 else 1)
    lim = ref.bound(ref.terms(kind, wcnt, c, T), mag)
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(lim, 1e-300)))
    print('%s %s: max |dev - host| / bound = %.3f' % (tag, kind, worst))
    assert gcnt.dtype == np.int64 and np.array_equal(gcnt, wcnt), (tag, kind)
    assert not np.isnan(got).any() and np.all(err <= lim), (tag, kind, got, want, lim)
    assert np.all(got[wcnt == 0] == 0.)
    for g in guards:
        assert g.margins_intact(), (tag, kind)
        assert g.t.dtype != sess.torch.float64 or not bool(sess.torch.isnan(g.t).any())          # `first` assigned: no NaN of the fill left
    return got


@pytest.mark.parametrize('V', VS)
def test_kernels_against_restatement(sess, V):
    """Every n_slices x c at this V, every kind on each; T and the ROI rotate so that each kind meets every T and every ROI."""
    rs = np.random.RandomState(1000 + V)
    geo_seen = set()
    for i, (n, c) in enumerate((n, c) for n in NS for c in CS):
        T = TS[(i // 3 + i % 3) % 3]
        P = ref.mixed_posteriors(rs, T, c, n, V)
        rois = ref.roi_cases(rs, n, V)
        g = ref.geometry(sess.lib, c, n, V)
        assert g['threads'] == 256 and g['sweep'] == 4 * g['threads'] and g['partials'] == (V + g['sweep'] - 2) // g['sweep'] + 1
        geo_seen.add((n * V > g['sweep'], g['sweep'] % V != 0 and n > 1))
        for j, kind in enumerate(ref.KINDS):
            roi = rois[ROIS[(i + j) % 4]]
            tag = 'V=%d n=%d c=%d T=%d roi=%s' % (V, n, c, T, ROIS[(i + j) % 4])
            if kind == 'AU':
                _check(sess, kind, au=(rs.randn(n, V) * 3).astype(np.float32), roi=roi, tag=tag)
            else:
                _check(sess, kind, P=P[:1] if kind == 'entropy' else P, roi=roi, tag=tag)
    if V == 37 * 41:
        assert (True, True) in geo_seen          # more than one sweep, and slice boundaries inside sweeps


def test_just_past_one_sweep_of_the_capped_grid(sess):
    """R = cap * sweep + 4 rows: every workgroup takes one sweep and the first a second one (asserted from the geometry); the
    16-byte path (R % 4 == 0)."""
    c, n = 2, 2
    g = ref.geometry(sess.lib, c, 1, 1)
    V = (g['cap'] * g['sweep'] + 4) // n
    g = ref.geometry(sess.lib, c, n, V)
    R = n * V
    sweeps = -(-R // g['sweep'])
    assert R % 4 == 0 and sweeps == g['cap'] + 1 and g['partials'] == -(-(V - 1) // g['sweep']) + 1
    rs = np.random.RandomState(7)
    P = ref.softmax_posteriors(rs, 2, c, n, V, 3.)
    roi = (rs.rand(n, V) < 0.3).astype(np.uint8)
    _check(sess, 'entropy', P=P[:1], roi=None, tag='capped grid')
    _check(sess, 'BALD', P=P, roi=roi, tag='capped grid')


@pytest.mark.parametrize('V,n', [(700, 3), (1022, 5)])
def test_a_workgroup_spans_two_slices(sess, V, n):
    """V below the rows of a sweep and no divisor of it: sweeps hold the end of one slice and the start of the next (asserted
    from the geometry); V = 1022 takes the guarded path (R % 4 != 0), V = 700 the 16-byte one."""
    c = 3
    g = ref.geometry(sess.lib, c, n, V)
    assert V < g['sweep'] < n * V and g['sweep'] % V != 0 and g['partials'] == 2
    assert any((k * g['sweep']) // V != (min((k + 1) * g['sweep'], n * V) - 1) // V for k in range(-(-n * V // g['sweep'])))
    rs = np.random.RandomState(V)
    P = ref.mixed_posteriors(rs, 2, c, n, V)
    rois = ref.roi_cases(rs, n, V)
    for j, kind in enumerate(ref.KINDS):
        if kind == 'AU':
            _check(sess, kind, au=(rs.randn(n, V) * 3).astype(np.float32), roi=rois[ROIS[j]], tag='span')
        else:
            _check(sess, kind, P=P[:1] if kind == 'entropy' else P, roi=rois[ROIS[j]], tag='span')


def test_exact_values_and_equal_bits(sess):
    """One-hot posteriors sum to exactly 0.0; BALD of one pass is exactly 0.0 (both kernels evaluate h through one device
    function); the same call twice gives the same bits."""
    rs = np.random.RandomState(3)
    for V, n, c in ((65, 3, 3), (256, 7, 8)):
        hot = ref.one_hot(rs, 1, c, n, V)
        for kind, P in (('entropy', hot), ('MC-entropy', np.repeat(hot, 3, axis=0)), ('BALD', np.repeat(hot, 3, axis=0))):
            got, cnt, _ = ref.device_scores(sess, kind, P=P)
            assert np.all(got == 0.) and np.all(cnt == V), (kind, got)
        P = ref.mixed_posteriors(rs, 1, c, n, V)
        got, _, _ = ref.device_scores(sess, 'BALD', P=P)
        assert np.all(got == 0.), got
        P = ref.mixed_posteriors(rs, 10, c, n, V)
        roi = ref.roi_cases(rs, n, V)['random']
        for kind in ('entropy', 'MC-entropy', 'BALD'):
            a = ref.device_scores(sess, kind, P=P[:1] if kind == 'entropy' else P, roi=roi)
            b = ref.device_scores(sess, kind, P=P[:1] if kind == 'entropy' else P, roi=roi)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), kind


def test_unaligned_buffers_take_the_guarded_path(sess):
    """R % 4 == 0, but every buffer starts one element past a 16-byte boundary."""
    from nnal_amd import slice_query
    torch = sess.torch
    c, n, V, T = 3, 3, 256, 2
    R = n * V
    rs = np.random.RandomState(11)
    P = ref.mixed_posteriors(rs, T, c, n, V)
    roi = ref.roi_cases(rs, n, V)['random']

    def off(arr, dtype):
        t = sess.empty((arr.size + 1,), dtype)
        t[1:] = sess.to_device(np.ascontiguousarray(arr).reshape(-1), dtype)
        assert t[1:].data_ptr() % 16 != 0
        return t[1:]
    sum_p = sess.empty((c * R + 1,), torch.float64)[1:]
    sum_h = sess.empty((R + 1,), torch.float64)[1:]
    for k in range(T):
        sess.unc_accumulate(off(P[k], torch.float32).view(c, R), sum_p.view(c, R), sum_h, first=k == 0)
    d_roi = off(roi, torch.uint8)
    want, wcnt, mag = slice_query.slice_scores_host(P, 'BALD', roi=roi)
    got, gcnt = sess.slice_scores(slice_query.KINDS['BALD'], n, V, c, T=T, sum_p=sum_p.view(c, R), sum_h=sum_h, roi=d_roi)
    assert np.array_equal(gcnt.cpu().numpy(), wcnt)
    assert np.all(np.abs(got.cpu().numpy() - want) <= ref.bound(ref.terms('BALD', wcnt, c, T), mag))
    want, wcnt, mag = slice_query.slice_scores_host(P[:1], 'entropy', roi=roi)
    got, gcnt = sess.slice_scores(slice_query.KINDS['entropy'], n, V, c, f32=off(P[0], torch.float32), roi=d_roi)
    assert np.array_equal(gcnt.cpu().numpy(), wcnt)
    assert np.all(np.abs(got.cpu().numpy() - want) <= ref.bound(ref.terms('entropy', wcnt, c, 1), mag))


def test_refusals_leave_the_outputs_alone(sess):
    torch = sess.torch
    lib, ctx = sess.lib, sess.ctx
    c, n, V = 3, 2, 8
    R = n * V
    post = sess.torch.full((c * R,), 0.25, dtype=torch.float32, device=sess.device)
    sum_p = torch.full((c * R,), 5., dtype=torch.float64, device=sess.device)
    sum_h = torch.full((R,), 6., dtype=torch.float64, device=sess.device)
    scores = torch.full((n,), 7., dtype=torch.float64, device=sess.device)
    counts = torch.full((n,), 8, dtype=torch.int64, device=sess.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    big = 1 << 31
    acc = [((None, p(post), c, R, 1, p(sum_p), p(sum_h)), -1), ((ctx, None, c, R, 1, p(sum_p), p(sum_h)), -1),
           ((ctx, p(post), c, R, 1, None, p(sum_h)), -1), ((ctx, p(post), c, 0, 1, p(sum_p), p(sum_h)), -1),
           ((ctx, p(post), 1, R, 1, p(sum_p), p(sum_h)), -4), ((ctx, p(post), 9, R, 1, p(sum_p), p(sum_h)), -4),
           ((ctx, p(post), c, big, 1, p(sum_p), p(sum_h)), -4)]
    for args, rc in acc:
        assert lib.alq_unc_accumulate(*args) == rc, args
    E, M, B, A = 0, 1, 2, 3
    sc = [((None, E, 1, c, n, V, None, None, p(post), None, p(scores), p(counts)), -1),
          ((ctx, E, 1, c, n, V, None, None, None, None, p(scores), p(counts)), -1),            # entropy without posteriors
          ((ctx, E, 1, c, n, V, None, None, p(post), None, None, p(counts)), -1),
          ((ctx, E, 1, c, n, V, None, None, p(post), None, p(scores), None), -1),
          ((ctx, M, 2, c, n, V, None, None, p(post), None, p(scores), p(counts)), -1),        # MC-entropy without sum_p
          ((ctx, B, 2, c, n, V, p(sum_p), None, None, None, p(scores), p(counts)), -1),       # BALD without sum_h
          ((ctx, A, 1, c, n, V, p(sum_p), p(sum_h), None, None, p(scores), p(counts)), -1),   # mean without its map
          ((ctx, 4, 1, c, n, V, p(sum_p), p(sum_h), p(post), None, p(scores), p(counts)), -1),
          ((ctx, -1, 1, c, n, V, p(sum_p), p(sum_h), p(post), None, p(scores), p(counts)), -1),
          ((ctx, B, 0, c, n, V, p(sum_p), p(sum_h), None, None, p(scores), p(counts)), -1),
          ((ctx, E, 1, c, 0, V, None, None, p(post), None, p(scores), p(counts)), -1),
          ((ctx, E, 1, c, n, 0, None, None, p(post), None, p(scores), p(counts)), -1),
          ((ctx, E, 1, 1, n, V, None, None, p(post), None, p(scores), p(counts)), -4),
          ((ctx, E, 1, 9, n, V, None, None, p(post), None, p(scores), p(counts)), -4),
          ((ctx, E, 1, c, 1 << 16, 1 << 15, None, None, p(post), None, p(scores), p(counts)), -4),
          ((ctx, E, 1, c, 1, big, None, None, p(post), None, p(scores), p(counts)), -4)]
    for args, rc in sc:
        assert lib.alq_slice_scores(*args) == rc, args
        assert b'alq_slice_scores' in lib.alq_last_error()
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    assert lib.alq_slice_scores_geometry(c, n, V, None) == -1 and lib.alq_slice_scores_geometry(c, 0, V, out) == -1
    assert lib.alq_slice_scores_geometry(9, n, V, out) == -4 and lib.alq_slice_scores_geometry(c, 1 << 16, 1 << 15, out) == -4
    assert list(out) == [-1] * 4
    sess.synchronize()
    assert bool((sum_p == 5.).all()) and bool((sum_h == 6.).all()) and bool((scores == 7.).all()) and bool((counts == 8).all())
    # and the last permitted size is not refused by the arithmetic: the geometry of 2^31 - 1 rows
    assert lib.alq_slice_scores_geometry(c, 1, big - 1, out) == 0 and out[3] == (big - 1 + 1022) // 1024 + 1


# ---------------------------------------------------------------------------------------------------- through the model
C_MODEL, Z = 3, 9


def _models(sess):
    from nnal_amd import NN_extended, netspec
    out = {}
    for tag, heads, kw in (('mc', C_MODEL, {}), ('au', C_MODEL + 1, dict(AU_4U=True))):
        ld, sk = netspec.net_c_2d_dense(heads)
        m = NN_extended.CNN((16, 16, 2), ld, 'sq_' + tag, list(sk), dropout=[[0], 0.5], sess=sess, max_batch=6, **kw)
        m.set_weights(netspec.he_init(ld, (16, 16, 2), seed=31, skips=sk, bias_std=0.05))
        out[tag] = m
    return out


@pytest.fixture(scope='module')
def models(sess):
    ms = _models(sess)
    yield ms
    for m in ms.values():
        m.close()


def _volume():
    rs = np.random.RandomState(77)
    imgs = [rs.randn(16, 16, Z).astype(np.float32) for _ in range(2)]
    for v in imgs:
        v[:5, :, :] = 0          # a background the 'nonzero' ROI leaves out
        v[:, :, 4] = 0           # a slice without any ROI voxel
    return imgs


@pytest.mark.parametrize('method', ['entropy', 'MC-entropy', 'BALD', 'AU'])
def test_model_scores_against_restatement_and_batching(sess, models, method):
    """slice_scores against the restatement of the maps the device passes produced (same seeds, copied back once); batch = 1, 4
    and max_batch give equal bits."""
    from nnal_amd import slice_query
    m = models['au' if method == 'AU' else 'mc']
    imgs = _volume()
    T, seed, c, V = 4, 5, C_MODEL, 256
    vol = slice_query._device_slices(sess, imgs)
    roi = slice_query._device_roi(sess, 'nonzero', vol)
    roi_host = roi.cpu().numpy().reshape(Z, V)
    assert np.array_equal(roi_host.reshape(Z, 16, 16), np.moveaxis((imgs[0] != 0) | (imgs[1] != 0), -1, 0))
    maps = np.zeros((T if method in slice_query.MC_METHODS else 1, 1 if method == 'AU' else c, Z, V), dtype=np.float32)

    def tap(a, b, k, x):
        maps[k, :, a:b] = x.cpu().numpy().reshape(maps.shape[1], b - a, V)
    sums, counts = slice_query.device_slice_sums(m, sess, vol, method, roi, T=T, seed=seed, tap=tap)
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    if method == 'AU':
        want, wcnt, mag = slice_query.slice_scores_host(None, 'AU', roi=roi_host, au=maps[0, 0])
        assert (maps > 0).any()
    else:
        want, wcnt, mag = slice_query.slice_scores_host(maps, method, roi=roi_host)
        assert np.all(np.abs(maps.sum(axis=1) - 1) < 1e-5)
    assert np.array_equal(counts, wcnt) and counts[4] == 0 and counts[0] == 11 * 16
    lim = ref.bound(ref.terms(method, wcnt, c, T), mag)
    print('%s: max |dev - host| / bound = %.3f' % (method, np.max(np.abs(sums - want) / np.maximum(lim, 1e-300))))
    assert np.all(np.abs(sums - want) <= lim), (sums, want, lim)
    if method == 'BALD':
        assert sums.max() > 0          # the passes differ: dropout is on
    res = [slice_query.slice_scores(m, sess, imgs, method, roi='nonzero', T=T, seed=seed, batch=b) for b in (1, 4, None)]
    want_mean, _ = slice_query.mean_scores(sums, counts)
    for s, n in res:
        assert s.dtype == np.float64 and n.dtype == np.int64 and s.shape == n.shape == (Z,)
        assert s.tobytes() == want_mean.tobytes() and np.array_equal(n, counts)
    assert res[0][0][4] == -np.inf
    # a ROI given as an (h, w, z) array, and none at all
    s_arr, n_arr = slice_query.slice_scores(m, sess, imgs, method, roi=(imgs[0] != 0) | (imgs[1] != 0), T=T, seed=seed)
    assert s_arr.tobytes() == want_mean.tobytes() and np.array_equal(n_arr, counts)
    s_all, n_all = slice_query.slice_scores(m, sess, imgs[0:2], method, roi=None, T=T, seed=seed)
    assert np.all(n_all == V) and np.all(np.isfinite(s_all))


def test_model_refusals(sess, models):
    from nnal_amd import NN_extended, netspec, slice_query
    imgs = _volume()
    with pytest.raises(NotImplementedError):
        slice_query.slice_scores(models['mc'], sess, imgs, 'AU')
    ld, sk = netspec.net_c_2d_dense(2)
    plain = NN_extended.CNN((16, 16, 2), ld, 'sq_plain', list(sk), sess=sess, max_batch=4)
    plain.set_weights(netspec.he_init(ld, (16, 16, 2), seed=3, skips=sk))
    for method in slice_query.MC_METHODS:
        with pytest.raises(ValueError):
            slice_query.slice_scores(plain, sess, imgs, method)
    with pytest.raises(ValueError):
        slice_query.slice_scores(plain, sess, [imgs[0]], 'entropy')          # one channel for a two-channel model
    plain.close()
    ldf, skf = netspec.net_c_2d(2)
    fc = NN_extended.CNN((16, 16, 2), ldf, 'sq_fc', list(skf), sess=sess, max_batch=4)
    with pytest.raises(NotImplementedError):
        slice_query.slice_scores(fc, sess, imgs, 'entropy')
    fc.close()


def test_query_feeds_get_dat_for_FT(sess):
    """query_slices on resident subjects (read in place: no upload of a volume) ranks as a stable host argsort of the device's own
    scores, and its lists go through get_dat_for_FT unchanged: the new labelled subjects hold exactly those slices."""
    from nnal_amd import NN_extended, slice_query
    from nnal_amd.datasets import data_holders
    from nnal_amd.datasets.utils import mask_class_ids
    luv = [np.array([1]), np.array([0, 2]), np.array([], dtype=int)]          # unlabelled: the two 12 x 10 subjects (6 and 7 slices)
    dat = cases.holder(data_holders.regular, luv, sess=sess)
    ld = OrderedDict([('c1', ['conv', [8, [3, 3]], 'MA']), ('last', ['conv', [3, [1, 1]], 'M'])])
    from nnal_amd import netspec
    m = NN_extended.CNN((12, 10, 2), ld, 'sq_query', [], dropout=[[0], 0.5], sess=sess, max_batch=4)
    m.set_weights(netspec.he_init(ld, (12, 10, 2), seed=5, skips=[], bias_std=0.05))
    pool = dat.tr_imgs[1:]
    assert [im.shape for im in pool] == [(12, 10, 6), (12, 10, 7)]
    uploads = []
    real = sess.to_device
    sess.to_device = lambda arr, dtype: (uploads.append(np.asarray(arr).size), real(arr, dtype))[1]
    try:
        for method, k in (('BALD', 5), ('entropy', 13), ('MC-entropy', 0)):
            got = slice_query.query_slices(m, sess, dat, method, k, T=3, seed=2)
            scores = [slice_query.slice_scores(m, sess, im, method, roi='nonzero', T=3, seed=2) for im in pool]
            flat = np.concatenate([s for s, _ in scores])
            assert np.all(np.concatenate([n for _, n in scores]) > 0)
            order = np.sort(np.argsort(-flat, kind='stable')[:k])
            want = [order[order < 6], order[order >= 6] - 6]
            assert len(got) == 2 and all(np.array_equal(g, w) and g.dtype.kind == 'i' for g, w in zip(got, want)), (method, got, want)
    finally:
        sess.to_device = real
    assert max(uploads, default=0) < 12 * 10          # nothing of the size of a slice went up
    with pytest.raises(ValueError):
        slice_query.query_slices(m, sess, dat, 'BALD', 14)
    got = slice_query.query_slices(m, sess, dat, 'BALD', 5, T=3, seed=2)
    new = data_holders.get_dat_for_FT(dat, got)
    host = cases.holder(data_holders.regular, luv)          # the same subjects as NumPy arrays
    chosen = [(i, q) for i, q in enumerate(got) if len(q)]
    assert len(new.tr_imgs) == 1 + len(chosen) and np.all(new.L_indic == 1)
    for j, (i, q) in enumerate(chosen):
        sub = new.tr_masks[1 + j].subject
        assert sub.shape == (12, 10, len(q))
        want_mask = mask_class_ids(np.asarray(host.tr_masks[1 + i])[:, :, q], np.arange(3))          # (255: a voxel of no class)
        assert np.array_equal(np.moveaxis(np.asarray(sub.mask.cpu()), 0, -1), want_mask)
        for jm in range(2):
            want_img = np.asarray(host.tr_imgs[1 + i][jm])[:, :, q].astype(np.float32)
            assert np.array_equal(np.moveaxis(sub.vol[..., jm].cpu().numpy(), 0, -1), want_img)
    m.close()
