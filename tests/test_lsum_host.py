"""Multi-class Fisher query on class slots (alq_class_layer_sums), host side: the new C symbol and the slot construction of
DeviceModel.fisher_classes against NNAL.class_weights (no GPU needed)."""
import ctypes as C
import re
import subprocess

import numpy as np
import torch


def test_class_layer_sums_symbol_is_declared_and_exported():
    import os
    from nnal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'alq.h')).read()
    assert re.search(r'\bint alq_class_layer_sums\(alq_model \*m, const float \*d_x, int N, int J, const int32_t \*d_cls, '
                     r'float \*d_post, double \*d_g\);', hdr)
    assert 'alq_class_layer_sums' in _lib.exported_names()
    _lib.build()
    nm = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert re.search(r'\bT alq_class_layer_sums\b', nm)
    src = open(os.path.join(_lib._HERE, 'csrc', 'build.sh')).read()
    assert len(re.findall(r'\blsum\b', src)) == 2          # compiled and linked


# ------------------------------------------------------------------------------------------------ slot construction
class _Sess(object):
    """The session calls fisher_classes makes, on CPU tensors (TEST INFRASTRUCTURE)."""
    torch = torch
    ctx = None

    def to_device(self, arr, dtype):
        return torch.as_tensor(np.ascontiguousarray(arr)).to(dtype)

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype)

    def bind_stream(self):
        pass


def _arr(p, n):
    return np.ctypeslib.as_array((C.c_double * n).from_address(p.value))


class _Lib(object):
    """alq_fisher_classes as a sequential NumPy loop over the class axis, on the pointers the caller passes."""

    def alq_fisher_classes(self, ctx, g, w, diag, n, c, L, A):
        g_, w_, d_ = _arr(g, n * c * L).reshape(n, c, L), _arr(w, n * c).reshape(n, c), _arr(diag, n)
        A_ = _arr(A, n * L * L).reshape(n, L, L)
        for i in range(n):
            acc = np.zeros((L, L))
            for j in range(c):
                acc = acc + w_[i, j] * np.outer(g_[i, j], g_[i, j])
            A_[i] = acc + d_[i] * np.eye(L)
        self.last_c = c
        return 0


class _Model(object):
    """A stand-in that runs the real fisher_classes / class_slots of DeviceModel on a table of random gradients."""

    def __init__(self, g):
        from nnal_amd import device
        self.g = g                                   # [n, c, L]
        self.nclass = g.shape[1]
        self.sess, self.lib = _Sess(), _Lib()
        self.class_slots = device.DeviceModel.class_slots
        self._fc = device.DeviceModel.fisher_classes
        self.seen = None

    def _as_device_batch(self, x):
        return torch.as_tensor(x), len(x)

    def class_layer_sums_device(self, t, n, classes):
        self.seen = np.array(classes)
        return torch.as_tensor(np.take_along_axis(self.g, np.asarray(classes)[:, :, None], axis=1).copy())

    def shrunk_class_gradients(self, x):
        return torch.as_tensor(self.g.copy()), None

    def fisher_classes(self, x, W, diag, fused=None):
        return self._fc(self, x, W, diag, fused)


def _posteriors():
    """[c = 12, B = 5] hand-made columns: a dropped class, the ten-largest branch, unequal kept counts."""
    c = 12
    P = np.zeros((c, 5))
    P[:, 0] = np.r_[0.5, 0.3, 0.2 - 3e-7, 3e-7, np.zeros(8)]                       # class 3 under 1e-6: dropped, 3 kept
    P[:, 1] = np.arange(1, 13) / 78.                                              # 12 non-zero: the ten largest (2 .. 11)
    P[:, 2] = np.r_[np.zeros(7), 0.4, 0.6, np.zeros(3)]                            # 2 kept, class 0 not among them
    P[:, 3] = np.r_[np.full(10, 0.1 - 1e-8), 5e-8, 5e-8]                           # exactly ten left after the drop
    P[:, 4] = np.r_[1. - 11e-3, np.full(11, 1e-3)]                                 # 12 non-zero with ties among the small ones
    return P


def test_slots_equal_class_weights_per_sample():
    from nnal_amd import NNAL, device
    P = _posteriors()
    c, B = P.shape
    W = np.zeros((B, c))
    kept = []
    for i in range(B):
        W[i], k = NNAL.class_weights(P[:, i].copy())
        kept.append(k)
    assert kept == [3, 10, 2, 10, 10]
    classes, weights = device.DeviceModel.class_slots(W)
    assert classes.shape == weights.shape == (B, 10)
    for i in range(B):
        sel = np.flatnonzero(W[i])
        np.testing.assert_array_equal(classes[i, :len(sel)], sel)                  # ascending class order
        np.testing.assert_array_equal(weights[i, :len(sel)], W[i, sel])
        np.testing.assert_array_equal(classes[i, len(sel):], 0)                    # spare slots: class 0, weight 0
        np.testing.assert_array_equal(weights[i, len(sel):], 0.)
    np.testing.assert_array_equal(classes[0, :3], [0, 1, 2])
    np.testing.assert_array_equal(classes[1], np.arange(2, 12))
    np.testing.assert_array_equal(classes[2, :2], [7, 8])


def test_fi_A_matrices_on_slots_equal_the_per_class_sum_exactly():
    from nnal_amd import NNAL
    P = _posteriors()
    c, B = P.shape
    L = 4
    g = np.random.RandomState(11).randn(B, c, L) * 10. ** np.random.RandomState(12).uniform(-4, 1, size=(B, c, 1))
    x = np.zeros((B, 2, 2, 1), dtype=np.float32)
    m = _Model(g)
    A_slots = np.stack(NNAL.fi_A_matrices(m, None, x, P.copy()))
    assert m.lib.last_c == 10 and m.seen.shape == (B, 10)                          # alq_fisher_classes ran over J slots
    # the per-class sum as the reference writes it (NNAL.py:399-409), classes in ascending order
    ref = np.zeros((B, L, L))
    for i in range(B):
        w, kept = NNAL.class_weights(P[:, i].copy())
        acc = np.zeros((L, L))
        for j in range(c):
            if w[j] != 0:
                acc = acc + w[j] * np.outer(g[i, j], g[i, j])
        ref[i] = acc + kept * 1e-5 * np.eye(L)
    np.testing.assert_array_equal(A_slots, ref)
    # ... and the rows arm (all c classes, zero weights on the dropped ones) gives the same bits
    m2 = _Model(g)
    W = np.stack([NNAL.class_weights(P[:, i].copy())[0] for i in range(B)])
    diag = np.array([NNAL.class_weights(P[:, i].copy())[1] * 1e-5 for i in range(B)])
    np.testing.assert_array_equal(m2.fisher_classes(x, W, diag, fused=False), ref)
    assert m2.lib.last_c == c and m2.seen is None
    np.testing.assert_array_equal(m2.fisher_classes(x, W, diag, fused=True), ref)


def test_fused_default_follows_the_environment(monkeypatch):
    g = np.random.RandomState(3).randn(2, 3, 2)
    W = np.array([[1., 0., 2.], [0., 3., 0.]])
    x = np.zeros((2, 1), dtype=np.float32)
    m = _Model(g)
    monkeypatch.delenv('ALQ_FI_ROWS', raising=False)
    m.fisher_classes(x, W, np.zeros(2))
    assert m.seen is not None and m.lib.last_c == 2
    m = _Model(g)
    monkeypatch.setenv('ALQ_FI_ROWS', '1')
    m.fisher_classes(x, W, np.zeros(2))
    assert m.seen is None and m.lib.last_c == 3
