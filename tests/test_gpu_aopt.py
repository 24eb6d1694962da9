"""The device A-optimal design solve of the `fi` query (csrc/aopt.hip, DeviceSession.aopt_design) on the GPU: every launch
through the C ABI against the NumPy restatement tests/aopt_ref.py, run-to-run determinism, whole solves against the host
solver's optimality conditions and the reference's own statement of the SDP, and the opt-in call sites end to end.

Bars of the launch tests.  The kernels evaluate the elementwise maps in the operation order of the restatement, so every
term of a sum is the same double on both sides and only the summation order differs: a sum of n terms is within
n 2^-52 sum|term| of the restatement's (the standard bound for any order; both sides' own rounding fits in it), the bound
formed by the test from the terms.  Max / min outputs are exact.  dq is within 4 m 2^-52 of the sum of its dot products'
|terms|.  Every device buffer of n candidates is followed by a tile of NaN: none of it may reach an output."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import aopt_ref  # noqa: E402

EPS = 2.0 ** -52
TOL = 1e-7


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _tile():
    from nnal_amd import _lib
    return int(_lib.lib().alq_aopt_tile())


def _shapes():
    from nnal_amd import _lib
    T = _tile()
    return [1, 2, 37, T - 1, T, T + 1, 3 * T + 5, T * int(_lib.lib().alq_aopt_max_workgroups()) + 5]


# n is given as an index into _shapes(): the tile is read from the library when the tests run.  The last size is the first
# at which a workgroup walks more than one tile (the grid is capped): one L is enough for that path
SHAPES = [(ni, L) for ni in range(7) for L in (1, 3, 7, 8)] + [(7, 3)]


@functools.lru_cache(maxsize=None)
def _state(ni, L):
    """A mid-solve state of the host restatement: the top of a late Newton step (q spread over many decades, mu small) and
    everything the four launches take there."""
    from scipy.linalg import cho_factor, cho_solve
    n = _shapes()[ni]
    A = aopt_ref.make_case(n, L, 1e-5, seed=1000 + 10 * ni + L)
    trace = []
    # a tight tolerance: late steps, q down to ~1e-11 (the large size: a dozen steps, enough to spread q)
    aopt_ref.solve(A, 1e-10, 500 if ni < 7 else 12, trace=trace)
    s = dict(trace[-2] if len(trace) >= 2 else trace[-1])
    V, q, kvec, R, mu, obj = s['V'], s['q'], s['kvec'], s['R'], s['mu'], s['obj']
    m = V.shape[1]
    st = aopt_ref.stats(V, q, kvec, R, mu, obj)
    S = cho_factor(np.eye(m) + st['G'])
    c_r, c_1 = cho_solve(S, st['h_r']), cho_solve(S, st['h_1'])
    ratio = (st['s_r'] - st['h_1'] @ c_r) / (st['s_1'] - st['h_1'] @ c_1)
    di = aopt_ref.direction(V, q, kvec, R, c_r, c_1, ratio, mu, obj)
    alpha0 = min(1.0, 0.99 * di['minratio']) if np.isfinite(di['minratio']) else 1.0
    s.update(A=A, n=n, L=L, m=m, c_r=c_r, c_1=c_1, ratio=ratio, dq=di['dq'], alphas=aopt_ref.alpha_ladder(alpha0), stats=st, dir=di)
    return s


def _padded(sess, arr):
    """The array on the device, followed by one tile of NaN rows; returns (view of the first n rows, whole buffer)."""
    torch = sess.torch
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    pad = np.full((_tile(),) + arr.shape[1:], np.nan)
    buf = sess.to_device(np.concatenate((arr, pad)), torch.float64)
    return buf[:arr.shape[0]], buf


def _tail_is_nan(buf, n):
    return bool(buf[n:].isnan().all().item())


def _within(dev, ref, bound, what):
    dev, ref, bound = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    err = np.abs(dev - ref)
    assert np.all(np.isfinite(dev)), what
    worst = (err / np.maximum(bound, 1e-300)).max() if err.size else 0.0
    print('%s: max err / bound = %.3f' % (what, worst))
    assert np.all(err <= bound), (what, float(err.max()), float(worst))


# ------------------------------------------------------------------------------------------------ launch by launch
@pytest.mark.parametrize('ni,L', SHAPES)
def test_svec(sess, ni, L):
    s = _state(ni, L)
    A, Abuf = _padded(sess, s['A'])
    V = sess.aopt_svec(A)
    np.testing.assert_array_equal(V.cpu().numpy(), aopt_ref.svec(s['A']))
    from nnal_amd import NNAL_tools
    np.testing.assert_allclose(V.cpu().numpy(), s['A'].reshape(s['n'], L * L) @ NNAL_tools._svec_basis(L), rtol=4e-16, atol=0)


@pytest.mark.parametrize('ni,L', SHAPES)
def test_stats(sess, ni, L):
    s = _state(ni, L)
    n, m = s['n'], s['m']
    V, _ = _padded(sess, s['V'])
    q, _ = _padded(sess, s['q'])
    work = sess.aopt_work(n, L)
    got = sess.aopt_stats(V, q, s['kvec'], s['R'], s['mu'], s['obj'], work)
    again = sess.aopt_stats(V, q, s['kvec'], s['R'], s['mu'], s['obj'], work)
    T, d = aopt_ref.stats_terms(s['V'], s['q'], s['kvec'], s['R'], s['mu'], s['obj'])
    ref = s['stats']
    bound = n * EPS * np.abs(T).sum(axis=0)
    print('n = %d, L = %d: min q = %.2e, mu = %.2e' % (n, L, s['q'].min(), s['mu']))
    assert got['maxd'] == ref['maxd'] == d.max()
    iu = np.triu_indices(m)                                  # the launch forms the upper triangle, (w u_a) u_b with a <= b
    _within(got['G'][iu], ref['G'][iu], bound[:m, :m][iu], 'G')
    np.testing.assert_array_equal(got['G'], got['G'].T)
    _within(got['h_r'], ref['h_r'], bound[:m, m], 'h_r')
    _within(got['h_1'], ref['h_1'], bound[:m, m + 1], 'h_1')
    _within(got['s_r'], ref['s_r'], bound[m, m + 1], 's_r')
    _within(got['s_1'], ref['s_1'], bound[m + 1, m + 1], 's_1')
    for key in got:
        np.testing.assert_array_equal(got[key], again[key])


@pytest.mark.parametrize('ni,L', SHAPES)
def test_direction(sess, ni, L):
    s = _state(ni, L)
    n, m = s['n'], s['m']
    torch = sess.torch
    V, _ = _padded(sess, s['V'])
    q, _ = _padded(sess, s['q'])
    dq, dqbuf = _padded(sess, np.zeros(n))
    dq2 = torch.zeros_like(dq)
    work = sess.aopt_work(n, L)
    args = (s['kvec'], s['R'], s['c_r'], s['c_1'], s['ratio'], s['mu'], s['obj'])
    got = sess.aopt_direction(V, q, *args, dq, work)
    again = sess.aopt_direction(V, q, *args, dq2, work)
    dq_ref, r, mag = aopt_ref.direction_terms(s['V'], s['q'], *args)
    dq_dev = dq.cpu().numpy()
    assert _tail_is_nan(dqbuf, n)
    _within(dq_dev, dq_ref, 4 * m * EPS * mag, 'dq')
    # the reductions, on the terms of the dq the device wrote
    _within(got['dec'], -(r * dq_dev).sum(), n * EPS * np.abs(r * dq_dev).sum(), 'dec')
    neg = dq_dev < 0
    assert got['minratio'] == (np.min(-s['q'][neg] / dq_dev[neg]) if neg.any() else np.inf)
    terms = dq_dev[:, None] * s['V']
    _within(got['vdq'], terms.sum(axis=0), n * EPS * np.abs(terms).sum(axis=0), 'vdq')
    np.testing.assert_array_equal(dq_dev, dq2.cpu().numpy())
    for key in ('dec', 'minratio', 'vdq'):
        np.testing.assert_array_equal(got[key], again[key])


@pytest.mark.parametrize('ni,L', SHAPES)
def test_linesearch(sess, ni, L):
    s = _state(ni, L)
    n = s['n']
    q, _ = _padded(sess, s['q'])
    dq, _ = _padded(sess, s['dq'])
    work = sess.aopt_work(n, L)
    alphas = s['alphas']
    assert 1 <= len(alphas) <= 64
    got = sess.aopt_linesearch(q, dq, alphas, work)
    again = sess.aopt_linesearch(q, dq, alphas, work)
    ref = aopt_ref.linesearch(s['q'], s['dq'], alphas)
    # the same terms with an 80-bit logarithm: a reference whose own rounding is far below the bar
    args = [s['q'] + a * s['dq'] for a in alphas] + [s['q']]
    logs = [np.log(x.astype(np.longdouble)) for x in args]
    exact = np.array([float(v.sum()) for v in logs])
    bound = np.array([n * EPS * float(np.abs(v).sum()) for v in logs])
    _within(got, exact, bound, 'log sums against the 80-bit evaluation')
    _within(got, ref, bound, 'log sums against the restatement')
    np.testing.assert_array_equal(got, again)


@pytest.mark.parametrize('ni,L', SHAPES)
def test_update(sess, ni, L):
    s = _state(ni, L)
    n = s['n']
    V, _ = _padded(sess, s['V'])
    work = sess.aopt_work(n, L)
    alpha = s['alphas'][min(1, len(s['alphas']) - 1)]
    outs = []
    for _ in range(2):
        q, qbuf = _padded(sess, s['q'])
        dq, _ = _padded(sess, s['dq'])
        total, vq = sess.aopt_update(q, dq, V, alpha, work)
        assert _tail_is_nan(qbuf, n)
        outs.append((total, vq, q.cpu().numpy()))
    total, vq, q_dev = outs[0]
    qn = s['q'] + alpha * s['dq']
    _within(total, qn.sum(), n * EPS * np.abs(qn).sum(), 'sum of q')
    np.testing.assert_array_equal(q_dev, qn / total)                   # the division by the device's own sum is exact
    terms = q_dev[:, None] * s['V']
    _within(vq, terms.sum(axis=0), n * EPS * np.abs(terms).sum(axis=0), 'sum q V')
    q_ref, _, vq_ref = aopt_ref.update(s['q'], s['dq'], s['V'], alpha)
    np.testing.assert_allclose(q_dev, q_ref, rtol=(n + 2) * EPS, atol=0)
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


def test_unsupported_shapes_are_refused(sess):
    from nnal_amd import _lib
    lib = sess.lib
    t = sess.torch.zeros((64,), dtype=sess.torch.float64, device=sess.device)
    p = C.c_void_p(t.data_ptr())
    h = (C.c_double * 128)()
    sess.bind_stream()
    assert lib.alq_aopt_svec(sess.ctx, p, 1, 9, p) == -4 and b'L = 9' in lib.alq_last_error()
    assert lib.alq_aopt_svec(sess.ctx, p, 0, 3, p) == -4
    assert lib.alq_aopt_stats(sess.ctx, p, p, 4, 5, h, h, 1.0, 1.0, p, p) == -4        # m = 5 is no L(L+1)/2
    assert lib.alq_aopt_stats(sess.ctx, p, p, (1 << 31) // 36, 36, h, h, 1.0, 1.0, p, p) == -4
    assert lib.alq_aopt_update(sess.ctx, p, p, p, (1 << 31) // 6, 6, 1.0, p, p) == -4
    assert lib.alq_aopt_linesearch(sess.ctx, p, p, 4, h, 65, p, p) == -4
    assert lib.alq_aopt_work_bytes(100, 9) == 0 and lib.alq_aopt_work_bytes(100, 8) > 0
    with pytest.raises(_lib.AlqError):
        sess.aopt_svec(sess.torch.zeros((2, 9, 9), dtype=sess.torch.float64, device=sess.device))


# ------------------------------------------------------------------------------------------------ whole solves
def _whole_cases():
    out = [('case%d' % i, aopt_ref.make_case(n, L, load, seed=100 + i)) for i, (n, L, load) in enumerate(aopt_ref.CASES)]
    return out + aopt_ref.extra_cases()


WHOLE = ['case0', 'case1', 'case2', 'case3', 'case4', 'identical', 'dominant', 'saturated']


@functools.lru_cache(maxsize=None)
def _host_solution(name):
    from nnal_amd import NNAL_tools
    A = dict(_whole_cases())[name]
    return A, NNAL_tools.SDP_query_distribution(A, 0., [], None, tol=TOL)


def _recomputed(A, q):
    M = np.tensordot(q, A, axes=(0, 0))
    Mi = np.linalg.inv(M)
    f = float(np.trace(Mi))
    d = np.tensordot(A, Mi @ Mi, axes=([1, 2], [0, 1]))
    return f, float(d.max() / f - 1.0)


@pytest.mark.parametrize('name', WHOLE)
def test_whole_solve(sess, name):
    A, host = _host_solution(name)
    n = A.shape[0]
    assert host['status'].startswith('optimal')
    A_dev = sess.to_device(A, sess.torch.float64)
    soln = sess.aopt_design(A_dev, tol=TOL)
    again = sess.aopt_design(A_dev, tol=TOL)
    q = np.asarray(soln['x'][:n])
    q_host = np.asarray(host['x'][:n])
    f_dev, gap_dev = _recomputed(A, q)
    f_host, _ = _recomputed(A, q_host)
    print('%s: device %d steps (%s), host %d steps, max|q_dev - q_host| = %.3e, gap %.3e, f %.10e / %.10e' %
          (name, soln['iterations'], soln['status'], host['iterations'], np.abs(q - q_host).max(), gap_dev, f_dev, f_host))
    assert soln['status'].startswith('optimal') and 'device' in soln['status'] and soln['iterations'] <= 500
    assert q.min() >= 0 and abs(q.sum() - 1) < 1e-12
    assert gap_dev <= 2 * TOL
    assert abs(f_dev - f_host) <= TOL * max(f_dev, f_host)
    if name == 'identical':
        assert soln['iterations'] == 1 and host['iterations'] == 1
    # the report: like the host solver's
    assert set(host) | {'q_device'} == set(soln)
    np.testing.assert_array_equal(soln['q_device'].cpu().numpy(), q)
    np.testing.assert_allclose(soln['x'][n:], np.diag(np.linalg.inv(np.tensordot(q, A, axes=(0, 0)))), rtol=1e-9)
    assert abs(soln['primal objective'] - f_dev) <= 1e-9 * f_dev and abs(soln['gap'] - gap_dev) <= 1e-9
    np.testing.assert_allclose(soln['y'], [f_dev], rtol=1e-9)
    # two solves: the same bits
    np.testing.assert_array_equal(again['x'], soln['x'])
    assert again['iterations'] == soln['iterations']


def test_large_L_is_solved_on_the_host_and_says_so(sess):
    rs = np.random.RandomState(9)
    g = rs.randn(20, 9) * 0.3
    A = g[:, :, None] * g[:, None, :] + 1e-3 * np.eye(9)[None]
    soln = sess.aopt_design(sess.to_device(A, sess.torch.float64))
    assert soln['status'].startswith('optimal') and 'host' in soln['status']
    assert soln['q_device'].shape == (20,)


def _vec(Z):
    return np.ravel(Z, order='F')


def test_sdp_solution_certified_against_the_reference_statement(sess, golden_dir):
    """The assertions of tests/test_host_r2.py::test_sdp_solution_certified_against_the_reference_statement, `l0` case, with
    the same bars, on the device solver's (q, t, y): primal feasible for the matrices the reference's own code assembled
    (tests/golden/r2_sdp.npz), the dual point built from it feasible with zero gap."""
    from nnal_amd import NNAL_tools
    s = np.load(os.path.join(golden_dir, 'r2_sdp.npz'))
    tag = 'l0'
    A = s['A']
    assert float(s[tag + '_lambda']) == 0
    n, L = A.shape[0], A.shape[1]
    soln = NNAL_tools.SDP_query_distribution_device(sess, sess.to_device(A, sess.torch.float64), 0., [], 3, tol=1e-10)
    assert soln['status'].startswith('optimal') and 'device' in soln['status'], soln['status']
    x = np.asarray(soln['x'])
    q, t = x[:n], x[n:]
    c, Aeq, b = s[tag + '_c'].ravel(), s[tag + '_A'], s[tag + '_b'].ravel()
    nG = int(s[tag + '_nG'])
    assert nG == L + 1 and c.shape == (n + L,)
    np.testing.assert_allclose(Aeq @ x, b, atol=1e-9)
    for k in range(nG):
        G, h = s[tag + '_G%d' % k], s[tag + '_h%d' % k]
        S = h - (G @ x).reshape(h.shape, order='F')
        np.testing.assert_allclose(S, S.T, atol=1e-12)
        assert np.linalg.eigvalsh(S).min() >= -1e-9, (k, np.linalg.eigvalsh(S).min())
    M = np.tensordot(q, A, axes=(0, 0))
    Mi = np.linalg.inv(M)
    zs = []
    for j in range(L):
        v = np.concatenate((Mi[:, j], [-1.0]))
        zs.append(np.outer(v, v))
    d = np.tensordot(A, Mi @ Mi, axes=([1, 2], [0, 1]))
    y = np.asarray(soln['y'], dtype=np.float64)
    sl = y[0] - d
    assert sl.min() >= -1e-6 * d.max()
    zs.append(np.diag(np.maximum(sl, 0.)))
    resid = c + Aeq.T.ravel() * y[0]
    for k in range(nG):
        resid = resid + s[tag + '_G%d' % k].T @ _vec(zs[k])
    assert np.abs(resid).max() <= 1e-6 * max(1., d.max()), np.abs(resid).max()
    primal = float(c @ x)
    dual = -sum(np.sum(s[tag + '_h%d' % k] * zs[k]) for k in range(nG)) - float(b @ y)
    assert abs(primal - soln['primal objective']) <= 1e-9 * max(1., abs(primal))
    assert abs(primal - dual) <= 1e-6 * max(1., abs(primal)), (primal, dual)
    assert np.all(q >= 0) and abs(q.sum() - 1) < 1e-12


# ------------------------------------------------------------------------------------------------ end to end
def _same_draws_guaranteed(q_dev, q_host, k, seed):
    """True when every uniform draw of sample_query_dstr under `seed` lies farther from its nearest boundary of cumsum(q_host)
    than the two cumulative sums differ anywhere: both then pick the same positions."""
    np.random.seed(seed)
    u = np.random.sample(k)
    ch, cd = np.cumsum(np.maximum(q_host, 0)), np.cumsum(np.maximum(q_dev, 0))
    dist = np.abs(u[:, None] - ch[None, :]).min()
    diff = np.abs(ch - cd).max()
    print('max|cumsum(q_dev) - cumsum(q_host)| = %.3e, nearest draw-to-boundary distance = %.3e' % (diff, dist))
    return bool(diff < dist)


def test_fi_queries_end_to_end_with_the_device_solver(sess, golden_dir):
    from nnal_amd import PW_NNAL, NNAL_tools
    from tests.test_gpu_parity import _load, _neta_eval
    from tests.test_oracle_golden import Expr
    g = _load(golden_dir, 'eval_neta.npz')
    model, pshape = _neta_eval(sess, g)
    vols = [g['vol0'], g['vol1']]
    stats = g['stats'].tolist()
    pool = g['pool']
    base = {'patch_shape': pshape, 'ntb': 64, 'stats': stats, 'k': 10, 'B': 48, 'lambda_': 0., 'img_paths': ['a', 'b']}
    e_host, e_dev = Expr(dict(base)), Expr(dict(base, SDP_solver='DEVICE'))
    # without the key: the parent's path - candidates, host solver, draws from the global stream
    sel_inds, sel_posts, A = PW_NNAL.fisher_candidates(e_host, model, sess, vols, pool)
    host = NNAL_tools.SDP_query_distribution(A, 0., None, 10)
    q_host = np.array(host['x'][:48])
    np.random.seed(5)
    expect = sel_inds[NNAL_tools.sample_query_dstr(q_host.copy(), 10, replacement=True)]
    np.random.seed(5)
    np.testing.assert_array_equal(PW_NNAL.CNN_query(e_host, model, sess, vols, pool, None, 'fi'), expect)
    # with it
    sel_d, _, A_dev = PW_NNAL.fisher_candidates(e_dev, model, sess, vols, pool, on_device=True)
    np.testing.assert_array_equal(sel_d, sel_inds)
    np.testing.assert_array_equal(A_dev.cpu().numpy(), np.stack(A))
    q_dev = np.array(sess.aopt_design(A_dev)['x'][:48])
    np.random.seed(5)
    got = PW_NNAL.CNN_query(e_dev, model, sess, vols, pool, None, 'fi')
    assert 1 <= len(got) <= 10 and set(got) <= set(sel_inds) and len(set(got)) == len(got)
    if _same_draws_guaranteed(q_dev, q_host, 10, 5):
        np.testing.assert_array_equal(got, expect)
    with pytest.raises(NotImplementedError):
        PW_NNAL.CNN_query(Expr(dict(base, SDP_solver='DEVICE', lambda_=0.5)), model, sess, vols, pool, None, 'fi')
    # multi-image form
    mask = g['mask']
    allimgs = [vols + [mask], [vols[1], vols[0], mask]]
    pools = [pool[:170], pool[170:]]
    mm = {'patch_shape': pshape, 'ntb': 50, 'k': 8, 'B': 40, 'lambda_': 0.}
    recorded = {}
    orig = NNAL_tools.SDP_query_distribution

    def recorder(A_, *a, **kw):
        recorded['A'] = np.stack(A_)
        recorded['soln'] = orig(A_, *a, **kw)
        return recorded['soln']
    NNAL_tools.SDP_query_distribution = recorder
    try:
        np.random.seed(6)
        Q_host = PW_NNAL.query_multimg(Expr(dict(mm), train_stats=g['mm_tstats']), model, sess, allimgs, pools, None, 'fi')
    finally:
        NNAL_tools.SDP_query_distribution = orig
    ncand = recorded['A'].shape[0]
    qh = np.array(recorded['soln']['x'][:ncand])
    np.random.seed(6)
    draws = NNAL_tools.sample_query_dstr(qh.copy(), 8, replacement=True)
    sel = [g['mm_sel_inds_%d' % j] for j in range(2)]
    flat = np.concatenate(sel)
    np.testing.assert_array_equal(np.concatenate(Q_host), flat[draws])          # the default path: the module attribute, the host
    np.random.seed(6)
    Q = PW_NNAL.query_multimg(Expr(dict(mm, SDP_solver='DEVICE'), train_stats=g['mm_tstats']), model, sess, allimgs, pools, None, 'fi')
    assert len(Q) == 2 and 1 <= len(Q[0]) + len(Q[1]) <= 8
    for j in range(2):
        assert set(Q[j]) <= set(sel[j]) and len(set(Q[j])) == len(Q[j])
    qd = np.array(sess.aopt_design(sess.to_device(recorded['A'], sess.torch.float64))['x'][:ncand])
    if _same_draws_guaranteed(qd, qh, 8, 6):
        for j in range(2):
            np.testing.assert_array_equal(Q[j], Q_host[j])
    with pytest.raises(NotImplementedError):
        PW_NNAL.query_multimg(Expr(dict(mm, SDP_solver='DEVICE', lambda_=1.0), train_stats=g['mm_tstats']), model, sess, allimgs,
                              pools, None, 'fi')
    model.close()


def test_al_loop_with_the_device_solver(sess, golden_dir):
    """al_loop.run_rounds(..., sdp='device'), two rounds on 3000 NET-A patches: the bookkeeping of sdp='host', every round solved
    to 'optimal'; round 0 (the same model, the same pool) has the same candidates and A-matrices on both paths."""
    from nnal_amd import al_loop, NNAL_tools
    from tests.test_gpu_parity import _load, _neta_eval
    g = _load(golden_dir, 'eval_neta.npz')
    model, _ = _neta_eval(sess, g)
    n, B, k = 3000, 200, 10
    x = np.random.RandomState(31).randn(n, int(model.elems_per_patch)).astype(np.float32)
    pool = sess.to_device(x, sess.torch.float32)
    host = al_loop.run_rounds(model, sess, pool, 2, B, k, seed=15)
    dev = al_loop.run_rounds(model, sess, pool, 2, B, k, seed=15, sdp='device')
    with pytest.raises(NotImplementedError):
        al_loop.run_rounds(model, sess, pool, 1, B, k, seed=15, sdp='device', lambda_=0.5)
    with pytest.raises(ValueError):
        al_loop.run_rounds(model, sess, pool, 1, B, k, seed=15, sdp='gpu')
    assert len(dev) == len(host) == 2
    np.testing.assert_array_equal(dev[0]['candidates'], host[0]['candidates'])
    np.testing.assert_array_equal(dev[0]['A'], host[0]['A'])
    left, taken = n, np.zeros(0, np.int64)
    for r, (a, h) in enumerate(zip(dev, host)):
        assert set(a) == set(h) and set(a['sdp']) == set(h['sdp']) and set(a['seconds']) == set(h['seconds'])
        assert a['sdp']['status'].startswith('optimal') and 'device' in a['sdp']['status'], a['sdp']
        assert h['sdp']['status'].startswith('optimal') and 'device' not in h['sdp']['status']
        assert a['A'].shape == h['A'].shape and a['q'].shape == h['q'].shape == (B,)
        assert 1 <= len(a['queries']) <= k and len(np.unique(a['queries'])) == len(a['queries'])
        assert np.isin(a['queries'], a['candidates']).all() and not np.isin(a['candidates'], taken).any()
        taken = np.concatenate([taken, a['queries']])
        left -= len(a['queries'])
        assert a['pool_left'] == left
        assert abs(a['q'].sum() - 1) < 1e-12 and a['q'].min() >= 0 and a['sdp']['gap'] <= 2 * TOL
        if r == 0 and _same_draws_guaranteed(a['q'], h['q'], k, 15):
            np.testing.assert_array_equal(a['queries'], h['queries'])
    model.close()


def _imgfi_setup(g, tag, tmp_path, pars_extra):
    """The image-level `fi` case of tests/golden/r3_imgfi.npz (tests/test_r3_goldens.py::_imgfi_case): image files, NET-A
    weights and the experiment's parameters."""
    from oracle import netspec
    from tests.test_oracle_golden import Expr
    c, wseed, seed, k, B = [int(v) for v in g[tag + '_meta']]
    imgs = g['imgs']
    pfile = tmp_path / 'paths.txt'
    with open(pfile, 'w') as f:
        for i in range(len(imgs)):
            np.save(tmp_path / ('img_%d.npy' % i), imgs[i])
            f.write(str(tmp_path / ('img_%d.npy' % i)) + '\n')
    hw = imgs.shape[1]
    ld = netspec.net_a(nclass=c)
    in_shape = (hw, hw, 3)
    pars = netspec.he_init(ld, in_shape, seed=wseed, bias_std=0.05)
    last = list(pars.keys())[-1]
    pars[last][0] = (pars[last][0] * float(g[tag + '_logit_scale'])).astype(np.float32)
    expr = Expr(dict({'k': k, 'B': B, 'batch_size': 8, 'target_shape': (hw, hw), 'mean': 100.}, **pars_extra))
    expr.imgs_path_file = str(pfile)
    return ld, in_shape, pars, expr, seed, k


def test_image_level_fi_query_with_the_device_solver(sess, golden_dir, tmp_path):
    """NNAL.CNN_query(..., 'fi') under SDP_solver 'DEVICE': at lambda_ = 0 the device solver gets the candidates' A-matrices
    (what the host routine gets without the key) and the positions are valid; lambda_ > 0 is refused."""
    from nnal_amd import NN, NNAL, NNAL_tools
    from tests.test_gpu_parity import _load
    g = _load(golden_dir, 'r3_imgfi.npz')
    ld, in_shape, pars, expr, seed, k = _imgfi_setup(g, 'c3', tmp_path, {'lambda_': 0., 'SDP_solver': 'DEVICE'})
    model = NN.CNN(in_shape, ld, 'imgfi', len(ld) - 2, None, sess=sess, max_batch=5)
    model.set_weights(pars)
    pool = g['c3_pool_inds']
    rec = {}
    orig_dev, orig_host = NNAL_tools.SDP_query_distribution_device, NNAL_tools.SDP_query_distribution

    def dev_recorder(s_, A_dev, *a, **kw):
        rec['A_dev'] = A_dev.cpu().numpy()
        rec['soln'] = orig_dev(s_, A_dev, *a, **kw)
        return rec['soln']

    def host_recorder(A, *a, **kw):
        rec['A_host'] = np.stack(A)
        return orig_host(A, *a, **kw)
    NNAL_tools.SDP_query_distribution_device, NNAL_tools.SDP_query_distribution = dev_recorder, host_recorder
    try:
        np.random.seed(seed)
        Q = NNAL.CNN_query(model, expr, pool, 'fi', sess, col=True)
        assert 'A_host' not in rec
        expr.pars['SDP_solver'] = 'CVXOPT'
        np.random.seed(seed)
        Q_host = NNAL.CNN_query(model, expr, pool, 'fi', sess, col=True)
    finally:
        NNAL_tools.SDP_query_distribution_device, NNAL_tools.SDP_query_distribution = orig_dev, orig_host
    assert rec['soln']['status'].startswith('optimal') and 'device' in rec['soln']['status']
    np.testing.assert_array_equal(rec['A_dev'], rec['A_host'])
    assert 1 <= len(Q) <= k and len(set(Q)) == len(Q) and set(Q) <= set(range(len(pool)))
    assert 1 <= len(Q_host) <= k
    expr.pars.update(SDP_solver='DEVICE', lambda_=0.5)
    with pytest.raises(NotImplementedError):
        NNAL.CNN_query(model, expr, pool, 'fi', sess, col=True)
    model.close()
