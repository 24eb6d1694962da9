"""The A-optimal design of the `fi` query on the device (csrc/aopt.hip), a mixin of device.DeviceSession.  One method per launch:
host scalars / vectors of size m in, the launch's O(m^2) reduction outputs back as host values (one synchronising read-back each).
V [n, m], q, dq [n]: fp64 device tensors; work: aopt_work(n, L)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, check_tensor, ptr


class AoptOps(object):
    def aopt_tile(self):
        return int(self.lib.alq_aopt_tile())

    def aopt_work(self, n, L):
        return self.empty((int(self.lib.alq_aopt_work_bytes(int(n), int(L))),), self.torch.uint8)

    def _aopt_args(self, *tensors):
        self.bind_stream()
        for t in tensors:
            check_tensor(t, self.torch.float64, device=self.device)
        return [ptr(t) for t in tensors]

    @staticmethod
    def _h64(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, C.c_void_p(a.ctypes.data)

    def aopt_svec(self, A_dev):
        n, L = int(A_dev.shape[0]), int(A_dev.shape[1])
        V = self.empty((n, L * (L + 1) // 2), self.torch.float64)
        pA, pV = self._aopt_args(A_dev, V)
        check(self.lib.alq_aopt_svec(self._ctx, pA, n, L, pV))
        return V

    def aopt_stats(self, V, q, kvec, R, mu, obj, work):
        """alq_aopt_stats -> dict(G [m, m], h_r, h_1 [m], s_r, s_1, maxd)."""
        n, m = int(V.shape[0]), int(V.shape[1])
        ne = (m + 2) * (m + 3) // 2
        out = self.empty((ne + 1,), self.torch.float64)
        pV, pq, po = self._aopt_args(V, q, out)
        kvec, pk = self._h64(kvec)
        R, pR = self._h64(R)
        check(self.lib.alq_aopt_stats(self._ctx, pV, pq, n, m, pk, pR, float(mu), float(obj), po, ptr(work)))
        o = out.cpu().numpy()
        S = np.zeros((m + 2, m + 2))
        S[np.triu_indices(m + 2)] = o[:ne]
        G = S[:m, :m]
        return {'G': G + G.T - np.diag(np.diag(G)), 'h_r': S[:m, m].copy(), 'h_1': S[:m, m + 1].copy(), 's_r': float(S[m, m + 1]),
                's_1': float(S[m + 1, m + 1]), 'maxd': float(o[ne])}

    def aopt_direction(self, V, q, kvec, R, c_r, c_1, ratio, mu, obj, dq, work):
        """alq_aopt_direction: writes the device vector dq -> dict(dec, minratio, vdq [m])."""
        n, m = int(V.shape[0]), int(V.shape[1])
        out = self.empty((2 + m,), self.torch.float64)
        pV, pq, pd, po = self._aopt_args(V, q, dq, out)
        kvec, pk = self._h64(kvec)
        R, pR = self._h64(R)
        c_r, pcr = self._h64(c_r)
        c_1, pc1 = self._h64(c_1)
        check(self.lib.alq_aopt_direction(self._ctx, pV, pq, n, m, pk, pR, pcr, pc1, float(ratio), float(mu), float(obj), pd, po, ptr(work)))
        o = out.cpu().numpy()
        return {'dq': dq, 'dec': float(o[0]), 'minratio': float(o[1]), 'vdq': o[2:].copy()}

    def aopt_linesearch(self, q, dq, alphas, work):
        """alq_aopt_linesearch -> [J + 1]: sum log(q + alpha_j dq) for every j, then sum log q."""
        J = len(alphas)
        out = self.empty((J + 1,), self.torch.float64)
        pq, pd, po = self._aopt_args(q, dq, out)
        alphas, pa = self._h64(alphas)
        check(self.lib.alq_aopt_linesearch(self._ctx, pq, pd, int(q.numel()), pa, J, po, ptr(work)))
        return out.cpu().numpy()

    def aopt_update(self, q, dq, V, alpha, work):
        """alq_aopt_update: q <- (q + alpha dq) / sum, in place -> (sum before the division, sum_i q_i V_i [m])."""
        n, m = int(V.shape[0]), int(V.shape[1])
        out = self.empty((1 + m,), self.torch.float64)
        pq, pd, pV, po = self._aopt_args(q, dq, V, out)
        check(self.lib.alq_aopt_update(self._ctx, pq, pd, pV, n, m, float(alpha), po, ptr(work)))
        o = out.cpu().numpy()
        return float(o[0]), o[1:].copy()

    def aopt_design(self, A_dev, tol=1e-7, max_iter=500):
        """The query distribution of Fisher-information AL at lambda = 0 - min tr((sum q_i A_i)^-1) over the simplex - with the
        candidates on the device: the loop of NNAL_tools._aopt_newton, its O(n) work done by the four launches of csrc/aopt.hip
        and its L x L / m x m algebra (m = L(L+1)/2) in NumPy as there.  A_dev: fp64 device tensor [n, L, L]
        (fisher_device(..., want=('A',))).  Returns a dict like NNAL_tools.SDP_query_distribution's: 'x' = concat(q, t) on the
        host, 'q_device' the device vector, 'status', 'primal objective', 'gap', 'iterations', 'y'.  L > 8 (or a pool the
        library refuses) is solved by the host routine; 'status' says so."""
        from scipy.linalg import cho_factor, cho_solve
        from . import NNAL_tools
        torch = self.torch
        assert A_dev.dim() == 3 and A_dev.shape[1] == A_dev.shape[2] and A_dev.dtype == torch.float64 and A_dev.device == self.device
        A_dev = A_dev.contiguous()
        n, L = int(A_dev.shape[0]), int(A_dev.shape[1])
        m = L * (L + 1) // 2

        def on_host(why):
            soln = NNAL_tools.SDP_query_distribution(A_dev.cpu().numpy(), 0., [], None, tol=tol, max_iter=max_iter)
            soln['status'] += ' [solved on the host: %s]' % why
            soln['q_device'] = self.to_device(soln['x'][:n], torch.float64)
            return soln
        if L > 8 or n < 1 or n >= (1 << 31) // m:
            return on_host('n = %d, L = %d is outside the device solver' % (n, L))
        P = NNAL_tools._svec_basis(L)
        try:
            work = self.aopt_work(n, L)
            V = self.aopt_svec(A_dev)
        except _lib.AlqError as e:
            return on_host(str(e))

        def at(v):
            Mi = np.linalg.inv((P @ v).reshape(L, L))
            return Mi, float(np.trace(Mi))

        def factors(Mi):
            Mi2 = Mi @ Mi
            K = P.T @ (np.kron(Mi, Mi2) + np.kron(Mi2, Mi)) @ P
            return P.T @ Mi2.reshape(-1), np.linalg.cholesky(0.5 * (K + K.T))

        q = torch.full((n,), 1.0 / n, dtype=torch.float64, device=self.device)
        dq = torch.zeros((n,), dtype=torch.float64, device=self.device)
        _, vq = self.aopt_update(q, dq, V, 0.0, work)
        Mi, obj = at(vq)
        mu = obj / n
        status, steps, maxd = 'unknown', 0, None
        max_iter = min(int(max_iter), 500)
        while steps < max_iter:
            steps += 1
            kvec, R = factors(Mi)
            st = self.aopt_stats(V, q, kvec, R, mu, obj, work)
            maxd = st['maxd']
            if maxd <= obj * (1.0 + tol):                      # optimality condition d_i <= tr M^-1 for every i
                status = 'optimal'
                break
            S = cho_factor(np.eye(m) + st['G'])
            c_r, c_1 = cho_solve(S, st['h_r']), cho_solve(S, st['h_1'])
            ratio = (st['s_r'] - st['h_1'] @ c_r) / (st['s_1'] - st['h_1'] @ c_1)
            di = self.aopt_direction(V, q, kvec, R, c_r, c_1, ratio, mu, obj, dq, work)
            dec = di['dec']
            alphas = [min(1.0, 0.99 * di['minratio']) if np.isfinite(di['minratio']) else 1.0]
            while alphas[-1] >= 1e-12 and len(alphas) < 64:    # every step the halving loop could test, in one launch
                alphas.append(alphas[-1] * 0.5)
            ls = self.aopt_linesearch(q, dq, alphas, work)
            phi0 = obj - mu * ls[len(alphas)]
            slack = 1e-12 * abs(phi0)
            for j, alpha in enumerate(alphas):
                _, on = at(vq + alpha * di['vdq'])
                if on - mu * ls[j] <= phi0 - 0.25 * alpha * dec + slack or alpha < 1e-12:
                    break
            _, vq = self.aopt_update(q, dq, V, alpha, work)
            Mi, obj = at(vq)
            maxd = None
            if dec <= 0.05 * mu * n:                           # centred for this mu
                mu = max(0.2 * mu, 0.25 * tol * obj / n)
        if maxd is None:                                       # the step limit ended the loop: the gap of the last iterate
            kvec, R = factors(Mi)
            maxd = self.aopt_stats(V, q, kvec, R, mu, obj, work)['maxd']
        t = np.diag(Mi).copy()
        return {'x': np.concatenate((q.cpu().numpy(), t)), 'q_device': q,
                'status': '%s (log-barrier Newton A-optimal design on the device; not cvxopt)' % status,
                'primal objective': float(t.sum()), 'gap': float(maxd / t.sum() - 1.0), 'iterations': steps,
                'y': np.array([float(kvec @ vq)])}
