"""alq_slic (csrc/slic.hip) against its NumPy statement nnal_amd/slic.py: labels and n_per_slice byte for byte, in both output
layouts, at the smallest shapes that take each path (the launch regime asserted from alq_slic_geometry where a case claims one);
guarded buffers, the refusals, and SuPix_query fed labels that never left the device (GPU box)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402
from tests import slic_cases  # noqa: E402
from tests.test_committee_host import Expr  # noqa: E402

CASES = slic_cases.cases()
_HOST = {}


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _host(name):
    from nnal_amd import slic
    if name not in _HOST:
        c = CASES[name]
        _HOST[name] = slic.slic_host(c['vol'], c['gh'], c['gw'], c['w'], c['T'], c['min_size'], c['mask'])
    return _HOST[name]


def _packed(sess, c):
    """(packed volume, packed mask bytes or None, lo, scale) of a case."""
    from nnal_amd import slic
    from nnal_amd.datasets.utils import ResidentSubject
    torch = sess.torch
    mods = slic.as_modalities(c['vol'])
    vol = ResidentSubject.pack(sess, mods).vol
    mask = None
    if c['mask'] is not None:
        mask = torch.as_tensor(np.ascontiguousarray(np.where(c['mask'], 0, 255).astype(np.uint8).transpose(2, 0, 1))).to(sess.device)
    lo, scale = slic.quant_range(mods, c['mask'])
    return vol, mask, lo, scale


def _device(sess, c, hwz=True):
    from nnal_amd import regions
    vol, mask, lo, scale = _packed(sess, c)
    labels, counts = regions.slic_device(sess, vol, c['gh'], c['gw'], c['w'], c['T'], c['min_size'], mask, lo, scale, hwz=hwz)
    return labels.cpu().numpy(), counts.cpu().numpy()


def _geometry(sess, c):
    mods = c['vol']
    H, W, S = mods[0].shape
    out = (C.c_int64 * 8)()
    assert sess.lib.alq_slic_geometry(sess.ctx, (C.c_int64 * 3)(H, W, S), len(mods), c['gh'], c['gw'], out) == 0
    return dict(tiles=out[0], assign_groups=out[1], clusters_per_group=out[2], update_groups=out[3], slice_groups=out[4], cap=out[5],
                pixel_groups=out[6], tile=out[7])


# ------------------------------------------------------------------------------------------------------------ byte equality
@pytest.mark.parametrize('name', sorted(CASES))
def test_bytes_equal_statement_both_layouts(sess, name):
    want_l, want_n = _host(name)
    got_l, got_n = _device(sess, CASES[name], hwz=True)
    assert got_l.dtype == np.int32 and got_n.dtype == np.int32 and got_l.shape == want_l.shape
    assert got_n.tobytes() == want_n.tobytes()
    assert got_l.tobytes() == want_l.tobytes()
    zhw_l, zhw_n = _device(sess, CASES[name], hwz=False)
    assert zhw_n.tobytes() == want_n.tobytes()
    assert zhw_l.tobytes() == np.ascontiguousarray(want_l.transpose(2, 0, 1)).tobytes()


def test_cases_take_the_paths_they_name(sess):
    """Host-side facts the case names promise, and the launch regimes from the exported geometry."""
    assert slic_cases.slice_stats(CASES['rounds'])[2]['rounds'] >= 2
    assert slic_cases.slice_stats(CASES['checkerboard'])[2]['orphans'] > 0
    assert slic_cases.slice_stats(CASES['pocket'])[2]['unadopted'] == 1
    lab, inn, _ = slic_cases.slice_stats(CASES['empty_cluster'])
    assert 0 not in lab[inn]
    g = _geometry(sess, CASES['odd'])
    assert g['tile'] == 16 and g['tiles'] == 3 * 2 * 2                 # 20 x 28: 2 x 2 tiles per slice, none of them whole
    assert 3 * 4 > g['clusters_per_group']                             # more clusters per slice than one update workgroup takes
    assert g['cap'] >= 8 and g['assign_groups'] == g['tiles']          # uncapped here: the capped regime is the test below
    assert _geometry(sess, CASES['pixel_cells'])['tiles'] == 2         # one tile per slice


def test_capped_grids_stride(sess, monkeypatch):
    """Two workgroups for everything: three slices are one more than the per-slice launches cover in a sweep, 12 tiles, 36 clusters
    and 1680 pixels need several sweeps each.  Same bytes."""
    monkeypatch.setenv('ALQ_SLIC_MAX_GROUPS', '2')
    for name in ('odd', 'mask_nan', 'rounds'):
        c = CASES[name]
        g = _geometry(sess, c)
        S = c['vol'][0].shape[2]
        assert g['cap'] == 2 and g['slice_groups'] == 2 and g['assign_groups'] == 2 and g['update_groups'] == 2 and g['pixel_groups'] == 2
        assert g['tiles'] > 2 and S * c['gh'] * c['gw'] > 2 * g['clusters_per_group'] and np.prod(c['vol'][0].shape) > 2 * 256
        if name != 'rounds':
            assert S == g['slice_groups'] + 1
        got_l, got_n = _device(sess, c)
        assert got_l.tobytes() == _host(name)[0].tobytes() and got_n.tobytes() == _host(name)[1].tobytes()
    monkeypatch.setenv('ALQ_SLIC_MAX_GROUPS', '1')
    assert _geometry(sess, CASES['odd'])['slice_groups'] == 1
    got_l, got_n = _device(sess, CASES['odd'])
    assert got_l.tobytes() == _host('odd')[0].tobytes() and got_n.tobytes() == _host('odd')[1].tobytes()


def test_same_bytes_twice(sess):
    a = _device(sess, CASES['rounds'])
    b = _device(sess, CASES['rounds'])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_oversegment_on_the_device_equals_the_host_route(sess):
    """regions.oversegment with a session (the wrapper's own quantisation range, taken on the device) against the call without one,
    host arrays and a resident subject, with a mask."""
    from nnal_amd import regions
    from nnal_amd.datasets.utils import ResidentSubject
    c = CASES['mask_nan']
    kw = dict(n_segments=12, compactness=0.02, T=3, min_size=3, mask=c['mask'], with_counts=True)
    want = regions.oversegment(c['vol'], **kw)
    got = regions.oversegment(c['vol'], sess=sess, **kw)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    from nnal_amd import slic
    subj = ResidentSubject.pack(sess, slic.as_modalities(c['vol']))
    dev = regions.oversegment(subj, keep_on_device=True, **kw)
    assert dev[0].is_cuda and dev[0].dtype == sess.torch.int32
    assert dev[0].cpu().numpy().tobytes() == want[0].tobytes() and dev[1].cpu().numpy().tobytes() == want[1].tobytes()


# --------------------------------------------------------------------------------------------------------- guards and refusals
def test_guarded_buffers(sess):
    """Output and work buffers inside guard margins: the call writes its own bytes and no other."""
    torch = sess.torch
    c = CASES['mask_nan']
    vol, mask, lo, scale = _packed(sess, c)
    Z, H, W, m = (int(v) for v in vol.shape)
    dims = (C.c_int64 * 3)(H, W, Z)
    nbytes = int(sess.lib.alq_slic_work_bytes(dims, m, c['gh'], c['gw']))
    assert nbytes > 0 and nbytes % 8 == 0
    G = 64
    work = torch.full((G + nbytes + G,), 0x5a, dtype=torch.uint8, device=sess.device)
    lab = torch.full((16 + H * W * Z + 16,), -77, dtype=torch.int32, device=sess.device)
    cnt = torch.full((16 + Z + 16,), -77, dtype=torch.int32, device=sess.device)
    assert work.data_ptr() % 8 == 0
    sess.bind_stream()
    for hwz in (1, 0):
        rc = sess.lib.alq_slic(sess.ctx, C.c_void_p(vol.data_ptr()), C.c_void_p(mask.data_ptr()), dims, m, (C.c_double * m)(*lo),
                               (C.c_double * m)(*scale), c['gh'], c['gw'], c['w'], c['T'], c['min_size'], hwz, C.c_void_p(lab.data_ptr() + 64),
                               C.c_void_p(cnt.data_ptr() + 64), C.c_void_p(work.data_ptr() + G))
        assert rc == 0, sess.lib.alq_last_error()
        lab_h, cnt_h, work_h = lab.cpu().numpy(), cnt.cpu().numpy(), work.cpu().numpy()
        assert np.all(lab_h[:16] == -77) and np.all(lab_h[-16:] == -77) and np.all(cnt_h[:16] == -77) and np.all(cnt_h[-16:] == -77)
        assert np.all(work_h[:G] == 0x5a) and np.all(work_h[-G:] == 0x5a)
        want = _host('mask_nan')
        assert cnt_h[16:-16].tobytes() == want[1].tobytes()
        assert lab_h[16:-16].tobytes() == (want[0] if hwz else np.ascontiguousarray(want[0].transpose(2, 0, 1))).tobytes()


def test_refusals(sess):
    from nnal_amd._lib import ALQ_EINVAL
    ALQ_EUNSUPPORTED = -4
    torch = sess.torch
    H, W, Z, m = 6, 7, 2, 1
    vol = torch.zeros((Z, H, W, m), dtype=torch.float32, device=sess.device)
    lab = torch.full((H * W * Z,), -77, dtype=torch.int32, device=sess.device)
    cnt = torch.full((Z,), -77, dtype=torch.int32, device=sess.device)
    work = torch.zeros((4096,), dtype=torch.int64, device=sess.device)
    one = (C.c_double * 8)(*([1.0] * 8))
    good = dict(vol=vol.data_ptr(), mask=None, dims=(H, W, Z), m=m, lo=one, scale=one, gh=2, gw=2, w=1.0, T=1, min_size=0, hwz=1,
                lab=lab.data_ptr(), cnt=cnt.data_ptr(), work=work.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return sess.lib.alq_slic(sess.ctx, C.c_void_p(a['vol']) if a['vol'] else None, a['mask'], (C.c_int64 * 3)(*a['dims']), a['m'], a['lo'],
                                 a['scale'], a['gh'], a['gw'], a['w'], a['T'], a['min_size'], a['hwz'], C.c_void_p(a['lab']) if a['lab'] else None,
                                 C.c_void_p(a['cnt']) if a['cnt'] else None, C.c_void_p(a['work']) if a['work'] else None)

    sess.bind_stream()
    bad = [dict(vol=0), dict(lab=0), dict(cnt=0), dict(work=0), dict(lo=None), dict(scale=None), dict(dims=(0, W, Z)), dict(dims=(H, W, 0)),
           dict(m=0), dict(gh=0), dict(gw=0), dict(gh=H + 1), dict(gw=W + 1), dict(w=-1.0), dict(w=float('nan')), dict(w=float('inf')),
           dict(T=-1), dict(min_size=-1), dict(hwz=2), dict(work=work.data_ptr() + 4), dict(lab=lab.data_ptr() + 2),
           dict(lo=(C.c_double * 8)(float('nan'))), dict(scale=(C.c_double * 8)(float('inf')))]
    for kw in bad:
        assert call(**kw) == ALQ_EINVAL, kw
    for kw in (dict(m=9), dict(dims=(1 << 16, 1 << 15, 1), gh=1, gw=1), dict(dims=(1 << 10, 1 << 10, 1 << 11), gh=1, gw=1)):
        assert call(**kw) == ALQ_EUNSUPPORTED, kw
    sess.synchronize()
    assert np.all(lab.cpu().numpy() == -77) and np.all(cnt.cpu().numpy() == -77)          # refused before any launch
    assert sess.lib.alq_slic_work_bytes((C.c_int64 * 3)(H, W, Z), 9, 2, 2) == 0
    assert sess.lib.alq_slic_work_bytes((C.c_int64 * 3)(H, W, Z), 1, H + 1, 2) == 0
    assert sess.lib.alq_slic_geometry(sess.ctx, (C.c_int64 * 3)(H, W, Z), 1, 2, 2, None) == ALQ_EINVAL
    assert call() == 0                                                                      # and the good call is good
    sess.synchronize()
    assert np.all(cnt.cpu().numpy() == 4)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_SuPix_query_from_the_volume(sess):
    """SuPix_query(overseg_img=None): labels made on the device and never copied back before the table is built - the same query
    as the one fed slic_host's labels as a host array, and as the one fed the device tensor."""
    from nnal_amd import NN, PW_NNAL, regions
    from tests.test_gpu_regions import PSHAPE, RADS, _subjects
    imgs, pools = _subjects()
    ld = netspec.net_a()
    net = NN.CNN((5, 5, 6), ld, 'slic_supix', None, None, sess=sess, max_batch=128)
    try:
        net.set_weights(netspec.he_init(ld, (5, 5, 6), seed=93, bias_std=0.2))
        pool = np.sort(pools[0])
        expr = Expr({'patch_shape': PSHAPE, 'ntb': 64, 'k': 9, 'B': 40, 'stats': [[0., 1.], [0., 1.]]}, None)
        kw = dict(n_segments=12, compactness=0.05, T=4, min_size=3)
        box = [v[RADS[0]:v.shape[0] - RADS[0], RADS[1]:v.shape[1] - RADS[1], RADS[2]:v.shape[2] - RADS[2]] for v in imgs[0][:2]]
        seg = regions.oversegment(box, **kw)
        assert seg.shape == (16, 14, 6) and seg.max() >= 6
        want = PW_NNAL.SuPix_query(expr, net, sess, imgs[0][:2], pool, seg, 'entropy')
        got = PW_NNAL.SuPix_query(expr, net, sess, imgs[0][:2], pool, None, 'entropy', **kw)
        dseg = regions.oversegment(box, sess=sess, keep_on_device=True, **kw)
        dev = PW_NNAL.SuPix_query(expr, net, sess, imgs[0][:2], pool, dseg, 'entropy')
        for res in (got, dev):
            np.testing.assert_array_equal(res[0], want[0])
            assert len(res[1]) == len(want[1])
            for a, b in zip(res[1], want[1]):
                np.testing.assert_array_equal(a, b)
        table = PW_NNAL.superpix_scoring(dseg, pool[:50], np.linspace(0., 1., 50))
        np.testing.assert_array_equal(table, PW_NNAL.superpix_scoring(seg, pool[:50], np.linspace(0., 1., 50)))
    finally:
        net.close()
