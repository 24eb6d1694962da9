"""The general-path entry points share one scratch-sizing walk, one forward prologue and one device flag (csrc/grads.hip): whatever
ran before on a model, each of them returns the bits it returns on a fresh model (GPU box).

Per case every call is recorded once on a model that runs nothing else - the reference, left unchanged - and must come out bit for
bit (a) on one model that runs all of them in list order, (b) on one that runs them in reverse order, a Fisher pass between every
two and each call first on 2 patches, then on all (the scratch buffers that are sized by n grow between the calls), (c) right after
a call that a class outside [0, nclass) made fail.  Bit equality has no tolerance: every launch here reduces in a fixed order.

Shapes: NET-C at 8^3 (conv, conv_transpose, pool, concat skips, fc head), 5 patches under max_batch 8; NET-B with narrow fc layers
at 25 x 25 x 2, the smallest input the GPU suite runs it at, 3 patches; NET-C with the 1x1 conv head at 8^3 for the two entry
points a fully-convolutional model accepts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 83
LOSS_SCALE = 0.37


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _cases():
    from nnal_amd import netspec
    ld_c, sk_c = netspec.net_c()
    ld_d, sk_d = netspec.net_c_dense()
    return {'netc': (ld_c, sk_c, (8, 8, 8, 1), 8, 5, False),
            'netb_small': (netspec.net_b_small(), (), (25, 25, 2), 4, 3, False),
            'netc_dense': (ld_d, sk_d, (8, 8, 8, 1), 8, 5, True)}


class _Case(object):
    """The inputs of one case on the device, a factory of fresh models, and the list of calls: name -> f(model, n) -> host arrays."""

    def __init__(self, sess, name):
        from nnal_amd import device, netspec
        torch = sess.torch
        ld, sk, in_shape, max_batch, n, dense = _cases()[name]
        self.sess, self.n, self.dense = sess, n, dense
        pars = netspec.he_init(ld, in_shape, seed=SEED, skips=sk, bias_std=0.05)

        def fresh():
            m = device.DeviceModel(sess, ld, in_shape, sk, max_batch=max_batch)
            m.set_weights(pars)
            return m
        self.fresh = fresh
        rs = np.random.RandomState(SEED + 1)
        x = rs.randn(n, *in_shape).astype(np.float32)
        self.t = sess.to_device(np.ascontiguousarray(x.reshape(n, -1)), torch.float32)
        m = fresh()
        self.nclass, V, P = m.nclass, m.out_voxels, m.num_params
        m.close()
        lab = rs.randint(0, self.nclass, size=n * V).astype(np.int32)
        lab[0], lab[1] = 0, 1
        self.lab = lab
        self.labd = sess.to_device(lab, torch.int32)
        self.classes = np.stack([lab[:n], (lab[:n] + 1) % self.nclass], axis=1)      # [n, J = 2]
        self.v = sess.to_device(rs.randn(P).astype(np.float32), torch.float32)
        self.V = V
        host = lambda *ts: [None if a is None else a.cpu().numpy() for a in ts]      # noqa: E731
        t, c = self.t, self

        def loss_grad(m, k):
            y = (c.lab[:k * V][None, :] == np.arange(c.nclass)[:, None]).astype(np.float32)      # [c, k V] one-hot columns
            g, loss = m._objective_pass(t[:k], k, y, 1., None, None, None)                        # alq_param_grads_loss
            return host(g) + [np.float64(loss)]
        if dense:
            self.calls = [('forward', lambda m, k: host(*m.forward_device(t[:k], k, want_pred=True)[:2])),
                          ('loss_grad', loss_grad)]
        else:
            self.calls = [
                ('param_grads_0', lambda m, k: host(*m.param_grads_device(t[:k], k, 0, cls=1, want_post=True))),
                ('param_grads_1', lambda m, k: host(*m.param_grads_device(t[:k], k, 1, labels=c.labd[:k], loss_scale=LOSS_SCALE,
                                                                          per_sample=False, want_post=True, want_loss=True))),
                ('sqnorms_class', lambda m, k: host(m.grad_sqnorms_device(t[:k], k, cls=0))),
                ('sqnorms_per_sample', lambda m, k: host(m.grad_sqnorms_device(t[:k], k, cls_per_sample=c.labd[:k]))),
                ('class_layer_sums', lambda m, k: host(m.class_layer_sums_device(t[:k], k, c.classes[:k]))),
                ('diag_fisher', lambda m, k: host(m.diagonal_fisher_device(t[:k], k, c.labd[:k]))),
                ('hess_vecp', lambda m, k: host(*m.hess_vecp_device(t[:k], k, c.labd[:k], c.v, None, loss_scale=1. / k, want_loss=True))),
                ('loss_grad', loss_grad)]
        self.ref = {}
        for nme, f in self.calls:      # each on a model that runs only that call
            m = fresh()
            self.ref[nme] = f(m, n)
            m.close()

    def same(self, nme, got, where):
        ref = self.ref[nme]
        assert len(got) == len(ref), (nme, where)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert (a is None) == (b is None), (nme, where, i)
            if a is not None:
                a, b = np.asarray(a), np.asarray(b)
                assert a.shape == b.shape and a.dtype == b.dtype, (nme, where, i)
                assert a.tobytes() == b.tobytes(), '%s %s: output %d differs from the fresh-model call in %d of %d entries' % (
                    nme, where, i, int(np.count_nonzero(a != b)), a.size)


_cache = {}


def _case(sess, name):
    if name not in _cache:
        _cache[name] = _Case(sess, name)
    return _cache[name]


NAMES = ['netc', 'netb_small', 'netc_dense']


@pytest.mark.parametrize('name', NAMES)
def test_references_are_finite_and_repeatable(sess, name):
    """What the other tests compare against: finite, non-trivial, and the same bits from a second fresh model."""
    c = _case(sess, name)
    for nme, f in c.calls:
        for a in c.ref[nme]:
            if a is not None:
                assert np.all(np.isfinite(a)) and np.any(np.asarray(a) != 0), nme
        m = c.fresh()
        c.same(nme, f(m, c.n), 'second fresh model')
        m.close()


@pytest.mark.parametrize('name', NAMES)
def test_calls_in_list_order_on_one_model(sess, name):
    c = _case(sess, name)
    m = c.fresh()
    for nme, f in c.calls:
        c.same(nme, f(m, c.n), 'in list order')
    m.close()


@pytest.mark.parametrize('name', NAMES)
def test_calls_in_reverse_order_with_fisher_passes_and_growing_n(sess, name):
    """Reverse order; each call on 2 patches first, then on all of them (wg_partial / gn_partial are sized by n and grow); between every
    two calls a Fisher pass, which leaves its own cotangents and engine state behind (an fc-head model only: a fully-convolutional
    model has no Fisher pass)."""
    c = _case(sess, name)
    m = c.fresh()
    for nme, f in reversed(c.calls):
        f(m, 2)
        c.same(nme, f(m, c.n), 'in reverse order, after n = 2')
        if not c.dense:
            m.fisher_device(c.t, c.n)
    m.close()


@pytest.mark.parametrize('name', ['netc', 'netb_small'])
def test_bad_class_is_refused_by_name_and_leaves_the_flag_clear(sess, name):
    from nnal_amd import _lib
    c = _case(sess, name)
    n, t = c.n, c.t
    m = c.fresh()
    calls = dict(c.calls)
    bad = c.lab[:n].copy()
    bad[n - 1] = c.nclass
    with pytest.raises(_lib.AlqError) as e:
        m.diagonal_fisher_device(t, n, bad)
    assert 'alq_diag_fisher' in str(e.value) and 'outside [0, %d)' % c.nclass in str(e.value), str(e.value)
    for nme in ('diag_fisher', 'class_layer_sums'):
        c.same(nme, calls[nme](m, n), 'after a refused alq_diag_fisher')
    badc = c.classes.copy()
    badc[0, 1] = c.nclass
    with pytest.raises(_lib.AlqError) as e:
        m.class_layer_sums_device(t, n, badc)
    assert 'alq_class_layer_sums' in str(e.value) and 'outside [0, %d)' % c.nclass in str(e.value), str(e.value)
    for nme in ('class_layer_sums', 'diag_fisher'):
        c.same(nme, calls[nme](m, n), 'after a refused alq_class_layer_sums')
    m.close()
