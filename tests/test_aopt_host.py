"""The launch decomposition of the device A-optimal design solve (tests/aopt_ref.py: four elementwise maps, each followed by a
reduction with O(m^2) output) against the shipped host solver NNAL_tools._aopt_newton.  CPU only.  This pins the decomposition
the kernels of csrc/aopt.hip are tested against (tests/test_gpu_aopt.py)."""
import numpy as np
import pytest

import nnal_amd  # noqa: F401
from nnal_amd import NNAL_tools

from tests import aopt_ref


@pytest.mark.parametrize('case', range(len(aopt_ref.CASES)))
def test_restated_loop_follows_the_host_solver(case):
    """Same number of Newton steps and max|q - q_host| <= 1e-10 (measured <= ~1e-13: the two differ in the summation order of
    the reductions and in M(q + alpha dq) formed as M(q) + alpha M(dq); the margin covers BLAS builds that sum in another
    order)."""
    n, L, load = aopt_ref.CASES[case]
    A = aopt_ref.make_case(n, L, load, seed=100 + case)
    q_host, st_host, steps_host = NNAL_tools._aopt_newton(A, 1e-7, 500)
    q, st, steps, info = aopt_ref.solve(A, 1e-7, 500)
    print('case %r: steps %d / %d, max|q - q_host| = %.3e' % (aopt_ref.CASES[case], steps, steps_host, np.abs(q - q_host).max()))
    assert st_host == 'optimal' and st == 'optimal'
    assert steps == steps_host
    assert np.abs(q - q_host).max() <= 1e-10
    assert info['maxd'] <= info['obj'] * (1 + 1e-7)


@pytest.mark.parametrize('name', ['identical', 'dominant', 'saturated'])
def test_extra_cases_are_solved_by_the_host_solver(name):
    """The three further inputs of the device tests are 'optimal' on the host; identical matrices stop at step 1."""
    A = dict(aopt_ref.extra_cases())[name]
    q_host, st_host, steps_host = NNAL_tools._aopt_newton(A, 1e-7, 500)
    q, st, steps, _ = aopt_ref.solve(A, 1e-7, 500)
    print('%s: steps %d / %d, max|q - q_host| = %.3e' % (name, steps, steps_host, np.abs(q - q_host).max()))
    assert st_host == 'optimal' and st == 'optimal'
    if name == 'identical':
        assert steps_host == 1 and steps == 1


def test_svec_is_the_basis_of_the_host_solver():
    A = aopt_ref.make_case(37, 8, 1e-3, seed=5)
    V = A.reshape(37, 64) @ NNAL_tools._svec_basis(8)
    np.testing.assert_allclose(aopt_ref.svec(A), V, rtol=4e-16, atol=0)


def test_launch_blocks_are_the_woodbury_pieces():
    """G, h_r, h_1, s_r, s_1 of launch A and dq of launch B are the U^T D^-1 U, H^-1 r and H^-1 1 of _aopt_newton."""
    from scipy.linalg import cho_factor, cho_solve
    trace = []
    A = aopt_ref.make_case(257, 7, 1e-3, seed=102)
    aopt_ref.solve(A, 1e-7, 500, trace=trace)
    s = trace[len(trace) // 2]
    V, q, R, mu, obj = s['V'], s['q'], s['R'], s['mu'], s['obj']
    n, m = V.shape
    st = aopt_ref.stats(V, q, s['kvec'], R, mu, obj)
    U = V @ R
    Dinv = q * q / mu
    r = -(V @ s['kvec']) - mu / q + (obj + n * mu)
    np.testing.assert_allclose(st['G'], U.T @ (U * Dinv[:, None]), rtol=1e-9, atol=1e-12 * np.abs(st['G']).max())
    np.testing.assert_allclose(st['h_r'], U.T @ (Dinv * r), rtol=1e-7, atol=1e-10 * np.abs(st['h_r']).max())
    np.testing.assert_allclose(st['s_1'], Dinv.sum(), rtol=1e-12)
    S = cho_factor(np.eye(m) + U.T @ (U * Dinv[:, None]))

    def Hinv(x):
        y = Dinv * x
        return y - (U * Dinv[:, None]) @ cho_solve(S, U.T @ y)
    a, b = Hinv(r), Hinv(np.ones(n))
    dq_host = -a + (a.sum() / b.sum()) * b
    dq = aopt_ref.direction(V, q, s['kvec'], R, s['c_r'], s['c_1'], s['ratio'], mu, obj)['dq']
    np.testing.assert_allclose(dq, dq_host, rtol=1e-6, atol=1e-9 * np.abs(dq_host).max())


def test_device_key_needs_a_device_session(golden_dir, tmp_path):
    """NNAL.CNN_query(..., 'fi') with SDP_solver 'DEVICE' and a session that is no DeviceSession: a TypeError that says so."""
    from nnal_amd import NNAL
    from oracle.model import OracleModel
    from tests.test_r3_goldens import _OracleImgModel, _load
    from tests.test_gpu_aopt import _imgfi_setup
    g = _load(golden_dir, 'r3_imgfi.npz')
    ld, in_shape, pars, expr, seed, k = _imgfi_setup(g, 'c3', tmp_path, {'lambda_': 0., 'SDP_solver': 'DEVICE'})
    m = _OracleImgModel(OracleModel(ld, in_shape, pars, feature_layer=len(ld) - 2))
    np.random.seed(seed)
    with pytest.raises(TypeError, match='DeviceSession'):
        NNAL.CNN_query(m, expr, g['c3_pool_inds'], 'fi', m.osess, col=True)
