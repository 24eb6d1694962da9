"""NumPy float64 restatement of the last-layer closed forms (NN.LLFC_grads / LLFC_hess, NN.py:874-955) and of the
stochastic influence recursion (PW_NNAL.stoch_approx_IF, PW_NNAL.py:851-881) in its implicit form: dot products and a
rank-c update per column, no explicit Hessian.  Shared by tests/test_llfc_host.py, tests/test_gpu_llfc.py, the golden
generator and tools/gpu_llfc.py.

Layouts are the reference's: features U [d, n], posteriors P [c, n]; a parameter vector is [W class-major (j*d + i), b]."""
import numpy as np


def llfc_grads(U, P, labels):
    """[(d+1)c, n]: column n = ((onehot(labels[n]) - P[:, n]) (x) U[:, n],  onehot - P[:, n])."""
    U = np.asarray(U, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    d, n = U.shape
    c = P.shape[0]
    E = -P.copy()
    E[np.asarray(labels).astype(np.int64), np.arange(n)] += 1.
    G = np.empty(((d + 1) * c, n))
    G[:c * d] = (E[:, None, :] * U[None, :, :]).reshape(c * d, n)
    G[c * d:] = E
    return G


def llfc_A(p):
    """A_jk = p_j (p_k - [j == k])."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    return p[:, None] * (p[None, :] - np.eye(p.size))


def llfc_hess(u, p):
    """The explicit [(d+1)c, (d+1)c] matrix of one sample: A (x) (u~ u~^T) in the [W, b] ordering."""
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    A = llfc_A(p)
    d, c = u.size, A.shape[0]
    H = np.empty(((d + 1) * c, (d + 1) * c))
    H[:c * d, :c * d] = (A[:, None, :, None] * (u[:, None, None] * u[None, None, :])[None]).reshape(c * d, c * d)
    H[:c * d, c * d:] = (A[:, None, :] * u[None, :, None]).reshape(c * d, c)
    H[c * d:, :c * d] = H[:c * d, c * d:].T
    H[c * d:, c * d:] = A
    return H


def stoch_if(Upool, Ppool, labels, Utr, Ptr, draws, scale):
    """V_0 = G; per draw r: s_k = Vw[k] . u_r + vb[k], q_j = p_j (s_j - sum_k p_k s_k), Vw[j] += Gw[j] - (q_j / scale) u_r,
    vb[j] += gb[j] - q_j / scale.  Returns V [(d+1)c, n_pool]."""
    G = llfc_grads(Upool, Ppool, labels)
    Utr = np.asarray(Utr, dtype=np.float64)
    Ptr = np.asarray(Ptr, dtype=np.float64)
    d, n = np.asarray(Upool).shape
    c = Ptr.shape[0]
    V = G.copy()
    for r in np.asarray(draws).astype(np.int64):
        u, p = Utr[:, r], Ptr[:, r]
        Vw = V[:c * d].reshape(c, d, n)
        s = np.einsum('kin,i->kn', Vw, u) + V[c * d:]
        q = p[:, None] * (s - (p[:, None] * s).sum(0)[None, :])
        V = V + G
        V[:c * d] -= ((q / scale)[:, None, :] * u[None, :, None]).reshape(c * d, n)
        V[c * d:] -= q / scale
    return V
