"""Host side of the last-layer closed forms: exported symbols, and the implicit float64 restatement (tests/llfc_ref.py) against
tests/golden/llfc.npz, the outputs of the reference's own NN.LLFC_grads / NN.LLFC_hess / PW_NNAL.stoch_approx_IF (explicit
np.kron Hessians).  The GPU tests compare the device with that restatement."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import llfc_ref

NETS = ('pool', 'fc')
SYMBOLS = ('alq_llfc_grads', 'alq_llfc_hess', 'alq_llfc_hess_max_bytes', 'alq_llfc_stoch_if', 'alq_llfc_if_path', 'alq_llfc_if_work_bytes')


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'llfc.npz'))


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_new_symbols_are_exported():
    from nnal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'alq.h')).read()
    assert re.search(r'\bint alq_llfc_stoch_if\(alq_ctx \*ctx, const float \*d_pool_feat, const float \*d_pool_post, '
                     r'const int32_t \*d_pool_labels, int n_pool,', hdr)
    _lib.build()
    nm = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for sym in SYMBOLS:
        assert sym in _lib.exported_names(), sym
        assert re.search(r'\bT %s\b' % sym, nm), sym
    src = open(os.path.join(_lib._HERE, 'csrc', 'build.sh')).read()
    assert len(re.findall(r'\bllfc\b', src)) == 2          # compiled and linked
    L = _lib.lib()
    assert L.alq_llfc_hess_max_bytes() == 256 << 20
    assert L.alq_llfc_if_work_bytes(67, 3) == 67 * 3 * 8
    # NET-B's column (2 x 4096 floats) stays in LDS, NET-C's (2 x 262144) and more than four classes stream
    assert L.alq_llfc_if_path(4096, 2) == 1 and L.alq_llfc_if_path(262144, 2) == 2 and L.alq_llfc_if_path(130, 5) == 2


def test_python_names_are_exported():
    from nnal_amd import NN, PW_NNAL, model_utils
    from nnal_amd.device import DeviceModel
    for name in ('LLFC_grads', 'LLFC_hess', 'PW_LLFC_grads'):
        assert callable(getattr(NN, name)) and getattr(model_utils, name) is getattr(NN, name)
    assert callable(PW_NNAL.stoch_approx_IF)
    for name in ('llfc_grads_device', 'llfc_stoch_if_device'):
        assert callable(getattr(DeviceModel, name))


@pytest.mark.parametrize('net', NETS)
def test_restatement_reproduces_the_reference(gold, net):
    g = {k[len(net) + 1:]: gold[k] for k in gold.files if k.startswith(net + '_')}
    Up, Pp, Ut, Pt = g['pool_feat'], g['pool_post'], g['tr_feat'], g['tr_post']
    d, c = Up.shape[0], Pp.shape[0]
    assert g['V'].shape == ((d + 1) * c, Up.shape[1]) and g['H3'].shape == ((d + 1) * c, (d + 1) * c)
    assert _rel(llfc_ref.llfc_grads(Up, Pp, g['labels']), g['G_given']) < 1e-12
    assert _rel(llfc_ref.llfc_grads(Up, Pp, g['pred']), g['G_pred']) < 1e-12
    np.testing.assert_array_equal(g['pred'], Pp.argmax(0))
    np.testing.assert_array_equal(g['weak'], g['pred'])
    assert _rel(llfc_ref.llfc_hess(Ut[:, 3], Pt[:, 3]), g['H3']) < 1e-12
    V = llfc_ref.stoch_if(Up, Pp, g['weak'], Ut, Pt, g['draws'], float(gold['scale']))
    assert _rel(V, g['V']) < 1e-12
    # the fixture contracts: |u~|^2 <= scale, and V stays below max_iter * max|G|
    assert ((Ut.astype(np.float64) ** 2).sum(0) + 1 <= float(gold['scale'])).all()
    assert np.abs(g['V']).max() < int(gold['max_iter']) * np.abs(g['G_pred']).max()
    # one explicit step of the reference's form, V <- G + V - (-H) V / scale, equals one implicit step
    G = g['G_pred']
    r = int(g['draws'][0])
    H = llfc_ref.llfc_hess(Ut[:, r], Pt[:, r])
    V1 = llfc_ref.stoch_if(Up, Pp, g['weak'], Ut, Pt, g['draws'][:1], float(gold['scale']))
    assert _rel(V1, G + G - (-H) @ G / float(gold['scale'])) < 1e-12


@pytest.mark.parametrize('net', NETS)
def test_draw_order_under_seed(gold, net):
    n_tr = gold[net + '_tr_x'].shape[0]
    np.random.seed(int(gold[net + '_seed']))
    draws = np.array([np.random.randint(n_tr) for _ in range(int(gold['max_iter']))])
    np.testing.assert_array_equal(draws, gold[net + '_draws'])
    assert len(np.unique(draws)) < len(draws)        # repeated draws are part of the fixture


def test_hessian_structure():
    rs = np.random.RandomState(5)
    u = rs.randn(6)
    p = np.exp(rs.randn(3))
    p /= p.sum()
    H = llfc_ref.llfc_hess(u, p)
    np.testing.assert_array_equal(H, H.T)
    ut = np.append(u, 1.)
    A = llfc_ref.llfc_A(p)
    assert np.abs(A.sum(1)).max() < 1e-15            # rows of A sum to p_j (sum_k p_k - 1) = 0
    full = np.kron(A, np.outer(ut, ut))              # in (class, u~) order: move every class's bias entry behind the weights
    order = [j * 7 + i for j in range(3) for i in range(6)] + [j * 7 + 6 for j in range(3)]
    np.testing.assert_allclose(H, full[np.ix_(order, order)], rtol=0, atol=1e-15)
