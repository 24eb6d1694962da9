"""NumPy fp64 restatement of the device side of the A-optimal design solve (csrc/aopt.hip) and of the loop built on it
(DeviceSession.aopt_design): a test helper, never imported by the product.

Each launch is stated as an ELEMENTWISE MAP over the candidates, written operation by operation (no fused multiply-add, dot
products taken left to right), followed by sums / a max / a min over the candidates.  The kernels evaluate the maps in the same
operation order, so every term is the same IEEE double here and there; only the order of the sums differs.  `*_terms`
return the terms [n, ...] so that a test can form the summation bound  n 2^-52 sum|term|  from them."""
import numpy as np

from nnal_amd import NNAL_tools

SQRT2 = float(np.sqrt(2.0))


def svec(A):
    """[n, L, L] -> [n, m] in the column order of NNAL_tools._svec_basis: diagonal entries as they are, off-diagonal ones
    (upper triangle) times sqrt(2)."""
    A = np.asarray(A, dtype=np.float64)
    n, L = A.shape[0], A.shape[1]
    cols = []
    for i in range(L):
        for j in range(i, L):
            cols.append(A[:, i, j] if i == j else A[:, i, j] * SQRT2)
    return np.ascontiguousarray(np.stack(cols, axis=1)) if n else np.zeros((0, L * (L + 1) // 2))


def seqdot(X, y):
    """sum_j X[:, j] y[j], left to right, product rounded before the add."""
    acc = np.zeros(X.shape[0])
    for j in range(X.shape[1]):
        acc = acc + X[:, j] * y[j]
    return acc


def u_rows(V, R):
    """u_i = R^T V_i, u_ik = sum_j V_ij R_jk left to right."""
    U = np.zeros((V.shape[0], R.shape[1]))
    for j in range(V.shape[1]):
        U = U + V[:, j:j + 1] * R[j:j + 1, :]
    return U


def elementwise(V, q, kvec, R, mu, obj):
    n = V.shape[0]
    d = seqdot(V, kvec)
    r = (-d - mu / q) + (obj + float(n) * mu)
    w = q * q / mu
    return d, r, w, u_rows(V, R)


def stats_terms(V, q, kvec, R, mu, obj):
    """terms [n, m+2, m+2] of sum_i w_i u~_i u~_i^T, u~ = (u, r, 1), each (w u~_a) u~_b; and d [n]."""
    d, r, w, U = elementwise(V, q, kvec, R, mu, obj)
    Ut = np.concatenate((U, r[:, None], np.ones((len(q), 1))), axis=1)
    WU = w[:, None] * Ut
    return WU[:, :, None] * Ut[:, None, :], d


def stats(V, q, kvec, R, mu, obj):
    T, d = stats_terms(V, q, kvec, R, mu, obj)
    m = V.shape[1]
    S = T.sum(axis=0)
    return {'G': S[:m, :m], 'h_r': S[:m, m], 'h_1': S[:m, m + 1], 's_r': S[m, m + 1], 's_1': S[m + 1, m + 1], 'maxd': d.max()}


def direction_terms(V, q, kvec, R, c_r, c_1, ratio, mu, obj):
    """dq [n] and the terms the elementwise bound of dq is formed from."""
    d, r, w, U = elementwise(V, q, kvec, R, mu, obj)
    WU = w[:, None] * U
    dr, d1 = seqdot(WU, c_r), seqdot(WU, c_1)
    a, b = w * r - dr, w - d1
    dq = -a + ratio * b
    mag = np.abs(w * r) + np.abs(WU * c_r).sum(axis=1) + abs(ratio) * (np.abs(w) + np.abs(WU * c_1).sum(axis=1))
    return dq, r, mag


def direction(V, q, kvec, R, c_r, c_1, ratio, mu, obj):
    dq, r, _ = direction_terms(V, q, kvec, R, c_r, c_1, ratio, mu, obj)
    neg = dq < 0
    return {'dq': dq, 'dec': float(-(r * dq).sum()), 'minratio': float(np.min(-q[neg] / dq[neg])) if neg.any() else np.inf,
            'vdq': (dq[:, None] * V).sum(axis=0)}


def linesearch(q, dq, alphas):
    """[J + 1]: sum log(q + alpha_j dq) for every j, then sum log q."""
    out = [np.log(q + a * dq).sum() for a in alphas]
    out.append(np.log(q).sum())
    return np.array(out)


def update(q, dq, V, alpha):
    qn = q + alpha * dq
    s = qn.sum()
    qn = qn / s
    return qn, float(s), (qn[:, None] * V).sum(axis=0)


def alpha_ladder(alpha0):
    """The steps the halving loop of _aopt_newton can test: alpha0 2^-j down to the first one below 1e-12."""
    out = [alpha0]
    while out[-1] >= 1e-12 and len(out) < 64:
        out.append(out[-1] * 0.5)
    return out


def solve(A, tol=1e-7, max_iter=500, launches=None, trace=None):
    """The loop of NNAL_tools._aopt_newton on the four launches.  `launches`: an object with svec / stats / direction /
    linesearch / update of this module's signatures (default: this module); `trace`: a list that receives the state at the
    top of every step.  Returns (q, status, steps, info)."""
    from scipy.linalg import cho_factor, cho_solve
    import sys
    la = launches or sys.modules[__name__]
    A = np.asarray(A, dtype=np.float64)
    n, L = A.shape[0], A.shape[1]
    P = NNAL_tools._svec_basis(L)
    m = P.shape[1]
    V = la.svec(A)

    def at(v):
        Mi = np.linalg.inv((P @ v).reshape(L, L))
        return Mi, float(np.trace(Mi))

    q, _, vq = la.update(np.full(n, 1.0 / n), np.zeros(n), V, 0.0)
    Mi, obj = at(vq)
    mu = obj / n
    status, steps, maxd, kvec = 'unknown', 0, np.nan, None
    while steps < max_iter:
        steps += 1
        Mi2 = Mi @ Mi
        kvec = P.T @ Mi2.reshape(-1)
        K = P.T @ (np.kron(Mi, Mi2) + np.kron(Mi2, Mi)) @ P
        K = 0.5 * (K + K.T)
        R = np.linalg.cholesky(K)
        if trace is not None:
            trace.append({'q': q.copy(), 'kvec': kvec, 'R': R, 'mu': mu, 'obj': obj, 'V': V})
        st = la.stats(V, q, kvec, R, mu, obj)
        maxd = st['maxd']
        if maxd <= obj * (1.0 + tol):
            status = 'optimal'
            break
        S = cho_factor(np.eye(m) + st['G'])
        c_r, c_1 = cho_solve(S, st['h_r']), cho_solve(S, st['h_1'])
        ratio = (st['s_r'] - st['h_1'] @ c_r) / (st['s_1'] - st['h_1'] @ c_1)
        if trace is not None:
            trace[-1].update(c_r=c_r, c_1=c_1, ratio=ratio)
        di = la.direction(V, q, kvec, R, c_r, c_1, ratio, mu, obj)
        dq, dec = di['dq'], di['dec']
        alpha0 = min(1.0, 0.99 * di['minratio']) if np.isfinite(di['minratio']) else 1.0
        alphas = alpha_ladder(alpha0)
        ls = la.linesearch(q, dq, alphas)
        phi0 = obj - mu * ls[len(alphas)]
        slack = 1e-12 * abs(phi0)
        for j, alpha in enumerate(alphas):
            Mn, on = at(vq + alpha * di['vdq'])
            if on - mu * ls[j] <= phi0 - 0.25 * alpha * dec + slack or alpha < 1e-12:
                break
        if trace is not None:
            trace[-1].update(dq=dq, alphas=alphas, alpha=alpha)
        q, _, vq = la.update(q, dq, V, alpha)
        Mi, obj = at(vq)
        if dec <= 0.05 * mu * n:
            mu = max(0.2 * mu, 0.25 * tol * obj / n)
    return q, status, steps, {'maxd': maxd, 'obj': obj, 'vq': vq, 'kvec': kvec}


# ---- the cases of the whole-solve tests ---------------------------------------------------------------------------
CASES = [(2, 3, 1e-3), (37, 3, 1e-5), (257, 7, 1e-3), (4099, 8, 1e-5), (4096, 8, 1e-3)]


def make_case(n, L, diag_load, seed):
    """Fisher-like candidates: A_i = (1 - p_i) g0 g0^T + p_i g1 g1^T + diag_load I with g1 close to a negative multiple of g0
    and a tenth of the posteriors p_i saturated at either end."""
    rs = np.random.RandomState(seed)
    g0 = rs.randn(n, L) * 0.05 * np.exp(rs.randn(L))[None, :]
    g1 = -(0.5 + rs.rand(n, 1)) * g0 + 0.01 * rs.randn(n, L) * np.abs(g0).mean()
    p = rs.rand(n)
    k = n // 10
    idx = rs.permutation(n)
    p[idx[:k]] = 0.0
    p[idx[k:2 * k]] = 1.0
    # outer products first: every A_i is symmetric bit for bit
    A = ((g0[:, :, None] * g0[:, None, :]) * (1 - p)[:, None, None] + (g1[:, :, None] * g1[:, None, :]) * p[:, None, None]
         + diag_load * np.eye(L)[None])
    return np.ascontiguousarray(A)


def extra_cases():
    """(name, A): B identical matrices (any q is optimal: one step), one candidate that dominates by 1e6, and all-saturated
    candidates (rank one + load)."""
    rs = np.random.RandomState(77)
    L = 5
    B0 = rs.randn(L, L)
    same = np.tile((B0 @ B0.T + 0.1 * np.eye(L))[None], (50, 1, 1))
    dom = make_case(200, 4, 1e-4, 78)
    dom[17] *= 1e6
    g = rs.randn(300, 6) * 0.1
    sat = g[:, :, None] * g[:, None, :] + 1e-4 * np.eye(6)[None]
    return [('identical', same), ('dominant', dom), ('saturated', np.ascontiguousarray(sat))]
