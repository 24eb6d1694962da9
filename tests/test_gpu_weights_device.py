"""Weights packed on the device (alq_model_set_weights_device, csrc/wpack.hip) against the host packers (GPU box).

Model H takes its weights through alq_model_set_weights (a DeviceModel created under ALQ_HOST_REPACK=1), model D through
alq_model_set_weights_device from an uploaded copy (DeviceModel.set_weights_device, never a host call before it).  The
contract is bit identity: every comparison below is torch.equal / array_equal on the raw bits."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import netspec  # noqa: E402

WIDE = 256          # fcgemm_build_plan: K and N multiples of the tile and >= 256 (net_b_small's default 64 stays below)


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _env_model(sess, env, *args, **kwargs):
    from nnal_amd import device
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return device.DeviceModel(sess, *args, **kwargs)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _host_model(sess, *args, **kwargs):
    m = _env_model(sess, {'ALQ_HOST_REPACK': '1'}, *args, **kwargs)
    assert m._host_repack
    return m


def _upload(sess, pars):
    torch = sess.torch
    return OrderedDict((n, (sess.to_device(np.ascontiguousarray(W, dtype=np.float32), torch.float32),
                            sess.to_device(np.ascontiguousarray(b, dtype=np.float32), torch.float32)))
                       for n, (W, b) in pars.items())


def _host_elems(m):
    v = m.lib.alq_model_engine_info(m._m, 14)
    assert v >= 0, v
    return v


def _w_elems(m, which):
    return sum(int(np.prod(m.param_shapes[t][1])) for t in range(m.L) if which(t))


def _adversarial(pars, names, seed, zero_layer=None):
    """The corners of the two splits in the wide fc layers `names`: exact zeros of either sign, values whose bf16
    rounding is a tie (low half 0x8000 over an even and over an odd high half), values that turn into fp16 subnormals
    (or vanish) under the scale one huge outlier sets, negative twins of all of them; `zero_layer`: all zeros (amax = 0)."""
    out = OrderedDict((n, [np.array(W, dtype=np.float32), np.array(b, dtype=np.float32)]) for n, (W, b) in pars.items())
    rs = np.random.RandomState(seed)
    for n in names:
        W = out[n][0]
        flat = W.reshape(-1)
        idx = rs.permutation(flat.size)
        k = flat.size // 16
        flat[idx[:k]] = 0.0
        flat[idx[k:2 * k]] = -0.0
        ties = flat[idx[2 * k:4 * k]].view(np.uint32)
        ties = (ties & np.uint32(0xffff0000)) | np.uint32(0x8000)
        flat[idx[2 * k:4 * k]] = ties.view(np.float32)
        tiny = np.array([1e-6, 3e-7, 7.5e-9, 7.4e-9, 1e-9, 1e-30, 1e-39, 1.4e-45], dtype=np.float32)
        sub = tiny[rs.randint(0, tiny.size, size=2 * k)] * rs.choice([-1., 1.], size=2 * k).astype(np.float32)
        flat[idx[4 * k:6 * k]] = sub
        flat[idx[6 * k]] = -1000.0          # the outlier: max |w| in [2^9, 2^10) -> w_exp = 4
        assert np.abs(flat).max() == 1000.0
    if zero_layer is not None:
        out[zero_layer][0][...] = 0.0
    return out


def _nets():
    ld_c, sk_c = netspec.net_c()
    # (name, layers, input shape, skips, patches, the layer whose output takes the dropout mask)
    return [('neta', netspec.net_a(), (20, 20, 1), (), 6, 2),
            ('netc8', ld_c, (8, 8, 8, 1), sk_c, 6, 8),
            ('netc32', ld_c, (32, 32, 32, 1), sk_c, 3, 8),
            ('netb25', netspec.net_b_small(width=WIDE), (25, 25, 2), (), 6, 7),       # fc1: 4704 inputs, not a multiple of 64 -> host; fc2 wide
            ('netb32', netspec.net_b_small(width=WIDE), (32, 32, 32), (), 6, 7)]      # fc1 (6144 inputs, 8 x 8 x 96 flatten) and fc2 wide


def _outputs(sess, m, x, labels):
    """Every device entry point on one batch: name -> tensor."""
    torch = sess.torch
    n = int(x.shape[0])
    t = sess.to_device(x.reshape(n, -1), torch.float32)
    out = OrderedDict()
    post, pred, feat = m.forward_device(t, n, want_pred=True, want_feat=True)
    out['post'], out['pred'], out['feat'] = post, pred, feat
    r = m.fisher_device(t, n, None, 1e-3)
    for k in ('p1', 'g0', 'g1', 'A', 'trace', 'Asum'):
        out['fisher_' + k] = r[k]
    g0, p0, _ = m.param_grads_device(t, n, 0, cls=1, keep_prob=0.5, seed=77, want_post=True)
    out['pg0'], out['pg0_post'] = g0, p0
    g1, _, l1 = m.param_grads_device(t, n, 1, labels=labels, loss_scale=1. / n, keep_prob=0.5, seed=78, per_sample=False, want_loss=True)
    out['pg1'], out['pg1_loss'] = g1, l1
    out['sqn'] = m.grad_sqnorms_device(t, n)
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    import torch
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        # bit patterns, not values: a NaN equals itself, -0 differs from +0
        ia, ib = a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)
        assert torch.equal(ia, ib), '%s: %s differs (%d of %d elements)' % (
            what, k, int((a[k] != b[k]).sum()), a[k].numel())


@pytest.mark.parametrize('name,ld,in_shape,sk,n,drop', _nets())
def test_same_bits_as_the_host_path(sess, name, ld, in_shape, sk, n, drop):
    """Forward, Fisher, parameter gradients (mode 0 and 1, with dropout) and gradient norms of model D equal model H's
    bit for bit, on the default engines and on the exact-fp32 engine (alq_debug_set(4, 1)), for He-normal weights and
    for the adversarial sets; the wide fc layers really took the device packers (engine info 14)."""
    from nnal_amd._lib import check
    he = netspec.he_init(ld, in_shape, seed=61, skips=sk, bias_std=0.05)
    names = list(he.keys())
    rs = np.random.RandomState(62)
    x = rs.randn(n, *in_shape).astype(np.float32)
    labels = rs.randint(0, 2, size=n).astype(np.int32)
    n_layers = len(ld)
    kw = dict(max_batch=8, feature_layer=n_layers - 2, dropout=([drop], 0.5))
    H = _host_model(sess, ld, in_shape, sk, **kw)
    D = _env_model(sess, {}, ld, in_shape, sk, **kw)
    wide = [t for t in range(D.L) if D._dev_pack[t]]
    if name == 'netb32':
        assert [D.var_names[t] for t in wide] == ['fc1', 'fc2']
    elif name == 'netb25':
        assert [D.var_names[t] for t in wide] == ['fc2']
    else:
        assert wide == []
    sets = [('he', he)]
    if wide:
        wn = [D.var_names[t] for t in wide]
        sets.append(('adversarial', _adversarial(he, wn, 63)))
        sets.append(('zero_layer', _adversarial(he, wn[:-1], 64, zero_layer=wn[-1])))
    assert _host_elems(D) == 0
    for sname, pars in sets:
        h0, d0 = _host_elems(H), _host_elems(D)
        H.set_weights(pars)
        D.set_weights_device(_upload(sess, pars))          # the first set of model D is a device one: first-call allocations
        assert _host_elems(H) - h0 == _w_elems(H, lambda t: True)
        assert _host_elems(D) - d0 == _w_elems(D, lambda t: t not in wide), 'a wide fc layer crossed to the host'
        # var_dict of D comes back from the device on access, with the values that went in
        for nme in names:
            for a, b in zip(D.var_dict[nme], pars[nme]):
                assert np.array_equal(np.asarray(a).view(np.uint32).ravel(), np.asarray(b, dtype=np.float32).view(np.uint32).ravel())
        _same(_outputs(sess, H, x, labels), _outputs(sess, D, x, labels), '%s %s default' % (name, sname))
        d1 = _host_elems(D)
        check(sess.lib.alq_debug_set(4, 1))
        try:
            oh, od = _outputs(sess, H, x, labels), _outputs(sess, D, x, labels)
        finally:
            check(sess.lib.alq_debug_set(4, 0))
        _same(oh, od, '%s %s exact fp32' % (name, sname))
        # the forms behind the knob were packed from the resident weights when the knob first selected them, once
        assert _host_elems(D) - d1 == _w_elems(D, lambda t: t in wide)
        _same(_outputs(sess, H, x, labels), _outputs(sess, D, x, labels), '%s %s default again' % (name, sname))
        assert _host_elems(D) - d1 == _w_elems(D, lambda t: t in wide)
    H.close()
    D.close()


def _debug_words(sess, m, layer_idx, what, words):
    torch = sess.torch
    buf = torch.zeros((max(words, 4),), dtype=torch.int32, device=sess.device)
    e = C.c_int64()
    from nnal_amd._lib import check
    check(m.lib.alq_model_debug_copy(m._m, int(layer_idx), int(what), 1, C.c_void_p(buf.data_ptr()), C.byref(e)))
    torch.cuda.synchronize()
    return buf[:e.value].cpu().numpy()


@pytest.mark.parametrize('wset', ['he', 'adversarial', 'zero_layer'])
def test_packed_bytes(sess, wset):
    """The bf16-triple and fp16-pair buffers of both Gemm orientations of the wide fc layers, the fp16 scale exponents
    and the fp64 L1 bound: byte-identical between the host packers and the device packers."""
    ld, in_shape = netspec.net_b_small(width=WIDE), (32, 32, 32)
    he = netspec.he_init(ld, in_shape, seed=65, bias_std=0.05)
    pars = {'he': he, 'adversarial': _adversarial(he, ['fc1', 'fc2'], 66),
            'zero_layer': _adversarial(he, ['fc1'], 67, zero_layer='fc2')}[wset]
    H = _host_model(sess, ld, in_shape, (), max_batch=4)
    D = _env_model(sess, {}, ld, in_shape, (), max_batch=4)
    H.set_weights(pars)
    D.set_weights_device(_upload(sess, pars))
    assert sess.lib.alq_model_engine_info(D._m, 0) == 1, 'fp16 pairs need fp16 subnormals in the matrix cores'
    lidx = {nme: i for i, nme in enumerate(ld.keys())}
    for nme, K, N in (('fc1', 6144, WIDE), ('fc2', WIDE, WIDE)):
        for what, per in ((6, 3), (7, 2), (8, 3), (9, 2)):
            words = K * N * per // 2
            h = _debug_words(sess, H, lidx[nme], what, words)
            d = _debug_words(sess, D, lidx[nme], what, words)
            assert h.size == words == d.size
            assert np.array_equal(h, d), '%s form %d: %d of %d words differ' % (nme, what, int((h != d).sum()), words)
        h, d = _debug_words(sess, H, lidx[nme], 10, 4), _debug_words(sess, D, lidx[nme], 10, 4)
        assert np.array_equal(h, d), (nme, h, d)
        W = np.asarray(pars[nme][0], dtype=np.float32)
        amax = float(np.abs(W).max())
        assert h[0] == h[1] == 14 - (int(np.frexp(np.float32(amax))[1]) if amax > 0 else 0)
        l1 = np.abs(W.astype(np.float64)).sum(0).max()          # (NumPy's pairwise sums: the value, not the bits)
        assert abs(h[2:4].view(np.float64)[0] - l1) <= 1e-12 * max(l1, 1.)
    H.close()
    D.close()


def _train_run(sess, env, ld, in_shape, sk, pars, opt, lr, train_layers, peek, tmp_path, tag):
    m = _env_model(sess, env, ld, in_shape, sk, max_batch=8)
    m.set_weights(pars)
    m.get_optimizer(lr, train_layers, opt)
    rs = np.random.RandomState(71)
    losses, grow = [], []
    for step in range(5):
        x = rs.randn(12, *in_shape).astype(np.float32)
        lab = rs.randint(0, 2, size=12)
        y = np.zeros((2, 12))
        y[lab, np.arange(12)] = 1
        before = _host_elems(m)
        losses.append(sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1.}))
        grow.append(_host_elems(m) - before)
        if peek and step == 2:
            assert m.var_dict.stale
            _ = [np.array(a) for wb in m.var_dict.values() for a in wb]
            assert not m.var_dict.stale
    xq = rs.randn(8, *in_shape).astype(np.float32)
    post = m.forward(xq)['posteriors']
    flat = m.flat_params()
    path = str(tmp_path / ('w_%s.npz' % tag))
    m.save_weights(path)
    saved = dict(np.load(path))
    wide = [t for t in range(m.L) if m._dev_pack[t]]
    sizes = [int(np.prod(m.param_shapes[t][1])) for t in range(m.L)]
    trained = [t for t in range(m.L) if (not train_layers or m.var_names[t] in train_layers)]
    m.close()
    return dict(losses=losses, grow=grow, post=post, flat=flat, saved=saved, wide=wide, sizes=sizes, trained=trained)


@pytest.mark.parametrize('opt,lr', [('SGD', 0.003), ('Adam', 0.002)])
@pytest.mark.parametrize('net', ['netb32', 'netc8'])
@pytest.mark.parametrize('subset', [False, True])
def test_training_same_bits_and_no_host_round_trip(sess, tmp_path, net, opt, lr, subset):
    """Five optimiser steps fed from the device vector against ALQ_HOST_REPACK=1 (the host round trip of every step):
    the loss of every step, the posteriors of a later query, flat_params() and the arrays of a save_weights file are
    bit-identical (the files are compared array by array: the .npz container carries time stamps); reading var_dict
    mid-way changes nothing.  Over the steps engine info 14 grows by no element of a wide fc layer on the default
    path and by every layer's full size per step under ALQ_HOST_REPACK=1."""
    if net == 'netb32':
        ld, in_shape, sk = netspec.net_b_small(width=WIDE), (32, 32, 32), ()
        tl = ['fc2', 'fc3'] if subset else []
    else:
        ld, sk = netspec.net_c()
        in_shape = (8, 8, 8, 1)
        tl = ['dec2', 'fc'] if subset else []
    pars = netspec.he_init(ld, in_shape, seed=72, skips=sk, bias_std=0.05)
    runs = {}
    for tag, env, peek in (('host', {'ALQ_HOST_REPACK': '1'}, False), ('dev', {}, False), ('dev_peek', {}, True)):
        runs[tag] = _train_run(sess, env, ld, in_shape, sk, pars, opt, lr, tl, peek, tmp_path, tag)
    h = runs['host']
    assert (len(h['wide']) == 2) == (net == 'netb32')
    for tag in ('dev', 'dev_peek'):
        d = runs[tag]
        assert [np.float64(v).tobytes() for v in d['losses']] == [np.float64(v).tobytes() for v in h['losses']], (tag, d['losses'], h['losses'])
        assert np.array_equal(d['flat'].view(np.uint32), h['flat'].view(np.uint32)), tag
        assert np.array_equal(d['post'].view(np.uint32), h['post'].view(np.uint32)), tag
        assert sorted(d['saved']) == sorted(h['saved'])
        for k in h['saved']:
            assert d['saved'][k].dtype == h['saved'][k].dtype and np.array_equal(d['saved'][k].view(np.uint32), h['saved'][k].view(np.uint32)), (tag, k)
        # the default path: only the layers without device packers (and with new values) went through the host
        want = sum(d['sizes'][t] for t in d['trained'] if t not in d['wide'])
        assert d['grow'] == [want] * 5, (tag, d['grow'], want)
        assert all(g == 0 for g in d['grow']) or any(t not in d['wide'] for t in d['trained'])
    assert h['grow'] == [sum(h['sizes'])] * 5, h['grow']          # today's path: the whole parameter vector, every step
    wide_elems = sum(h['sizes'][t] for t in h['wide'])
    assert all(hg - dg >= wide_elems for hg, dg in zip(h['grow'], runs['dev']['grow']))


def test_error_paths(sess):
    """Null pointers and a bad layer index give ALQ_EINVAL; a layer without device packers is not an error."""
    ld, in_shape = netspec.net_b_small(width=WIDE), (32, 32, 32)
    pars = netspec.he_init(ld, in_shape, seed=73)
    m = _env_model(sess, {}, ld, in_shape, (), max_batch=4)
    up = _upload(sess, pars)
    Wd, bd = up['fc2']
    lib = m.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    EINVAL = -1
    assert lib.alq_model_set_weights_device(None, 0, ptr(Wd), ptr(bd)) == EINVAL
    assert lib.alq_model_set_weights_device(m._m, m.var_names.index('fc2'), None, ptr(bd)) == EINVAL
    assert lib.alq_model_set_weights_device(m._m, m.var_names.index('fc2'), ptr(Wd), None) == EINVAL
    assert lib.alq_model_set_weights_device(m._m, -1, ptr(Wd), ptr(bd)) == EINVAL
    assert lib.alq_model_set_weights_device(m._m, m.L, ptr(Wd), ptr(bd)) == EINVAL
    assert lib.alq_model_layer_packs_on_device(m._m, m.L) == EINVAL
    assert lib.alq_model_layer_packs_on_device(m._m, m.var_names.index('fc2')) == 1
    assert lib.alq_model_layer_packs_on_device(m._m, 0) == 0
    assert lib.alq_model_engine_info(m._m, 14) == 0
    # conv1: no device packers -> its slice takes the host packers, the call succeeds
    Wc, bc = up['conv1']
    assert lib.alq_model_set_weights_device(m._m, 0, ptr(Wc), ptr(bc)) == 0
    assert lib.alq_model_engine_info(m._m, 14) == int(Wc.numel())
    with pytest.raises(ValueError):
        m.set_weights_device(sess.torch.zeros((3,), dtype=sess.torch.float32, device=sess.device))
    m.close()


def test_two_pipelines_after_a_device_update(sess):
    """fisher_device over several device passes with two scoring pipelines after a training step fed the first model
    from the device: the second pipeline's model gets the wide fc layers from the same device vector (ordered behind
    the optimiser step) and every output equals the single pipeline's bit for bit."""
    torch = sess.torch
    ld, in_shape = netspec.net_b_small(width=WIDE), (32, 32, 32)
    pars = netspec.he_init(ld, in_shape, seed=74, bias_std=0.05)
    m = _env_model(sess, {}, ld, in_shape, (), max_batch=8)
    m.set_weights(pars)
    m.get_optimizer(0.003, [], 'SGD')
    rs = np.random.RandomState(75)
    n = 32
    xq = sess.to_device(rs.randn(n, int(np.prod(in_shape))).astype(np.float32), torch.float32)
    res = {}
    for step in range(2):
        x = rs.randn(12, *in_shape).astype(np.float32)
        lab = rs.randint(0, 2, size=12)
        y = np.zeros((2, 12))
        y[lab, np.arange(12)] = 1
        before = _host_elems(m)
        sess.run(m.train_step, feed_dict={m.x: x, m.y_: y, m.keep_prob: 1.})
        assert m.var_dict.stale
        m.lanes = 2
        r2 = m.fisher_device(xq, n, None, 1e-3)
        torch.cuda.synchronize()
        assert len(m._xlanes) == 1 and m._xlanes[0]['version'] == m._weights_version
        # neither model took a wide fc layer through the host (the second model's counter is its own)
        wide = sum(int(np.prod(m.param_shapes[t][1])) for t in range(m.L) if m._dev_pack[t])
        total = sum(int(np.prod(m.param_shapes[t][1])) for t in range(m.L))
        assert _host_elems(m) - before == total - wide
        assert m.lib.alq_model_engine_info(m._xlanes[0]['m'], 14) == (step + 1) * (total - wide)
        m.lanes = 1
        r1 = m.fisher_device(xq, n, None, 1e-3)
        torch.cuda.synchronize()
        _same(r1, r2, 'step %d' % step)
        res[step] = r1
    assert not torch.equal(res[0]['p1'], res[1]['p1'])          # the update did change the model
    m.close()
