"""NumPy reference of the sparse (inducing-point, DTC) NNGP posterior (include/nngp_sparse.h).  Test infrastructure only.

With inducing rows U, training rows X (added in any number of chunks), kernel K and noise sigma2:

    sigma2 = diag_reg * (sum_i K(x_i, x_i) / n)                     (diag_reg itself with absolute=True)
    K_uu   = K(U, U) + jitter * trace(K(U, U)) / m * I,   L_u = chol(K_uu)
    per chunk:  Vt = K(X_c, U) L_u^-T;   G += Vt^T Vt;   R += Vt^T Y_c;   tr += sum K_ii;   n += c
    finish:     B = sigma2 I + G,   L_B = chol(B),   C = L_B^-1 R
    predict:    P = K(X_t, U) L_u^-T,   Q = P L_B^-T,   mean = Q C,   var = K_tt,ii - |p_i|^2 + sigma2 |q_i|^2,
                cov = K_tt - P P^T + sigma2 Q Q^T

(the V-form: B >= sigma2 I whatever cond(K_uu) is).  ``explicit`` is the textbook form with Sigma_A = (K_uu + K_uf K_fu / sigma2)^-1
for cross-checking, and ``dtype=np.longdouble`` runs the factorisations, solves and sums in 80-bit arithmetic with hand-written
Cholesky and triangular solves (the style of tests/extended_precision.py) as a referee.  The kernel matrices always come from the
float64 kernel function handed in: ``kernel(x1, x2)`` with x2 None for the symmetric build, ``diag(x)`` for K(x, x).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

import nngp_oracle as oracle


def oracle_kernel(n_relu=1):
    """(kernel, diag) of the oracle's all-ReLU NNGP kernel with n_relu hidden layers."""
    arch = oracle.make_arch(n_relu)

    def kernel(x1, x2=None):
        return oracle.kernel_fn(x1, x2, "nngp", arch)

    def diag(x):  # the closed-form diagonal (theta = 0), as the library takes it
        x = np.asarray(x, dtype=np.float64)
        return oracle.diag_kernel(np.sum(x * x, axis=1) / x.shape[1], arch)[0]

    return kernel, diag


def _chol(a, dtype):
    if dtype == np.float64:
        return np.linalg.cholesky(a)
    n = a.shape[0]
    l = np.zeros((n, n), dtype=dtype)
    a = a.astype(dtype)
    for j in range(n):
        row = l[j, :j]
        piv = a[j, j] - row @ row
        if not piv > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % j)
        l[j, j] = np.sqrt(piv)
        if j + 1 < n:
            l[j + 1:, j] = (a[j + 1:, j] - l[j + 1:, :j] @ row) / l[j, j]
    return l


def _solve_lower(l, b, dtype):
    """L^-1 b for b [n, k]."""
    if dtype == np.float64:
        return scipy.linalg.solve_triangular(l, b, lower=True)
    x = b.astype(dtype).copy()
    for j in range(l.shape[0]):
        x[j] = (x[j] - l[j, :j] @ x[:j]) / l[j, j]
    return x


class SparseReference:
    def __init__(self, kernel, diag, diag_reg=1e-3, jitter=1e-8, absolute=False, dtype=np.float64):
        self.kernel, self.diag, self.diag_reg, self.jitter, self.absolute, self.dtype = kernel, diag, diag_reg, jitter, absolute, dtype
        self.u = None

    def set_inducing(self, u):
        self.u = np.asarray(u, dtype=np.float64)
        m = self.u.shape[0]
        kuu = self.kernel(self.u, None).astype(self.dtype)
        self.jitter_added = self.dtype(self.jitter) * (np.trace(kuu) / m)
        self.kuu = kuu + self.jitter_added * np.eye(m, dtype=self.dtype)
        self.lu = _chol(self.kuu, self.dtype)
        self.g = np.zeros((m, m), dtype=self.dtype)
        self.r = None
        self.tr, self.n = self.dtype(0.0), 0
        return self

    def add_rows(self, x, y, chunk_rows=None):
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(x.shape[0], -1)
        if self.r is None:
            self.r = np.zeros((self.u.shape[0], y.shape[1]), dtype=self.dtype)
        step = x.shape[0] if chunk_rows is None else int(chunk_rows)
        for r0 in range(0, x.shape[0], step):
            xc, yc = x[r0:r0 + step], y[r0:r0 + step]
            vt = _solve_lower(self.lu, self.kernel(xc, self.u).T.astype(self.dtype), self.dtype).T  # [c, m]
            self.g = self.g + vt.T @ vt
            self.r = self.r + vt.T @ yc.astype(self.dtype)
            self.tr = self.tr + np.sum(self.diag(xc).astype(self.dtype))
            self.n += xc.shape[0]
        return self

    def finish(self):
        self.sigma2 = self.dtype(self.diag_reg) if self.absolute else self.dtype(self.diag_reg) * (self.tr / self.n)
        self.b = self.g + self.sigma2 * np.eye(self.g.shape[0], dtype=self.dtype)
        self.lb = _chol(self.b, self.dtype)
        self.c = _solve_lower(self.lb, self.r, self.dtype)
        return self

    def fit(self, x, y, u, chunk_rows=None):
        return self.set_inducing(u).add_rows(x, y, chunk_rows).finish()

    def predict(self, xt, cov="diag"):
        """mean [M, ny] and var [M] (cov='diag'), cov [M, M] (cov='full') or nothing more (cov=None)."""
        xt = np.asarray(xt, dtype=np.float64)
        p = _solve_lower(self.lu, self.kernel(xt, self.u).T.astype(self.dtype), self.dtype)  # [m, M]
        q = _solve_lower(self.lb, p, self.dtype)
        mean = q.T @ self.c
        if cov is None:
            return mean
        if cov == "diag":
            return mean, (self.diag(xt).astype(self.dtype) - np.sum(p * p, axis=0)) + self.sigma2 * np.sum(q * q, axis=0)
        return mean, (self.kernel(xt, None).astype(self.dtype) - p.T @ p) + self.sigma2 * (q.T @ q)


def explicit(kernel, diag, x, y, u, xt, diag_reg=1e-3, jitter=1e-8, absolute=False):
    """The same posterior in the textbook form: Sigma_A = (K_uu + K_uf K_fu / sigma2)^-1, mean = K_tu Sigma_A K_uf y / sigma2,
    cov = K_tt - K_tu K_uu^-1 K_ut + K_tu Sigma_A K_ut.  Float64; loses cond(K_uu) digits, so only for well-conditioned cases."""
    x, u, xt = (np.asarray(a, dtype=np.float64) for a in (x, u, xt))
    y = np.asarray(y, dtype=np.float64).reshape(x.shape[0], -1)
    m = u.shape[0]
    kuu = kernel(u, None)
    kuu = kuu + jitter * np.trace(kuu) / m * np.eye(m)
    sigma2 = diag_reg if absolute else diag_reg * np.sum(diag(x)) / x.shape[0]
    kuf, ktu = kernel(u, x), kernel(xt, u)
    sigma_a = np.linalg.inv(kuu + kuf @ kuf.T / sigma2)
    mean = ktu @ sigma_a @ (kuf @ y) / sigma2
    cov = kernel(xt, None) - ktu @ np.linalg.solve(kuu, ktu.T) + ktu @ sigma_a @ ktu.T
    return mean, cov


def greedy_inducing(kernel, x, m):
    """Indices of the m rows of x that the partial pivoted Cholesky of the prior kernel picks (pool_greedy_reference, noise 0),
    and the smallest relative gap between the best and the second-best candidate over the picks."""
    import pool_greedy_reference as R
    idx, _, _, gaps = R.greedy(kernel(np.asarray(x, dtype=np.float64), None), m, 0.0)
    return idx, float(np.min(gaps))
