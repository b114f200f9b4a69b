"""NumPy reference of the matrix-free exact NNGP posterior (include/nngp_matfree.h).  Test infrastructure only.

Preconditioned CG on a block of right-hand sides for A = K(X, X) + sigma2 I, with the Woodbury inverse of the sparse model's
P = sigma2 I + Vt Vt^T as preconditioner (built from ``sparse_reference.SparseReference``; m = 0: P = I):

    P^-1 r = (r - Vt L_B^-T L_B^-1 Vt^T r) / sigma2

The rules are the device's: vectors are RHS-major [r, n]; per-column scalars (rho, p^T A p, |r|^2); a column that has converged
(|r| <= tol |b|), or whose p^T A p is not positive and finite, is frozen; after the loop the true residual b - A x is formed,
columns above tol restart once from it, and the reported residual is the recomputed one.  ``columnwise=True`` applies the
operator and the preconditioner one column at a time, so that a column's arithmetic cannot depend on its neighbours (NumPy's
matrix products choose their blocking by shape).
"""
from __future__ import annotations

import functools
import os

import numpy as np
import scipy.linalg

import sparse_reference as S


def pcg(apply_a, b, precond=None, tol=1e-10, max_iter=1000, columnwise=False):
    """x [r, n] with A x = b [r, n], and a dict: iterations (the loop's), col_iterations [r] (steps each column took), k_passes,
    restarts, rel_residual [r] (true), converged."""
    b = np.asarray(b, dtype=np.float64)
    r_, n = b.shape

    def rows(f, v):
        if f is None:
            return v.copy()
        return np.stack([f(v[c:c + 1])[0] for c in range(v.shape[0])]) if columnwise else f(v)

    x = np.zeros_like(b)
    r = b.copy()
    bn2 = np.sum(b * b, axis=1)
    rr = bn2.copy()
    tol2 = tol * tol
    state = np.where(rr <= tol2 * bn2, 1, 0)  # 0 iterating, 1 converged, 2 broken down
    rho = np.zeros(r_)
    p = np.zeros_like(b)
    col_it = np.zeros(r_, dtype=np.int64)
    it = passes = restarts = 0
    first = True
    while True:
        while it < max_iter and np.any(state == 0):
            act = state == 0
            z = rows(precond, r)
            rho_new = np.sum(r * z, axis=1)
            beta = np.zeros(r_) if first else np.where(act, rho_new / np.where(rho != 0, rho, 1.0), 0.0)
            p[act] = z[act] + beta[act, None] * (0.0 if first else p[act])
            rho = np.where(act, rho_new, rho)
            first = False
            ap = rows(apply_a, p)
            passes += 1
            pap = np.sum(p * ap, axis=1)
            bad = act & ~((pap > 0) & np.isfinite(pap))
            state[bad] = 2
            go = act & ~bad
            a = np.where(go, rho / np.where(go, pap, 1.0), 0.0)
            x[go] += a[go, None] * p[go]
            r[go] -= a[go, None] * ap[go]
            rr = np.where(go, np.sum(r * r, axis=1), rr)
            state[go & (rr <= tol2 * bn2)] = 1
            col_it[go] += 1
            it += 1
        ax = rows(apply_a, x)
        passes += 1
        r = b - ax
        rr = np.sum(r * r, axis=1)
        rel = np.where(bn2 > 0, np.sqrt(rr / np.where(bn2 > 0, bn2, 1.0)), np.where(rr == 0, 0.0, np.inf))
        ok = bool(np.all(rel <= tol))
        if ok or restarts >= 1 or it >= max_iter:
            break
        restarts += 1
        state = np.where(rr <= tol2 * bn2, 1, 0)
        first = True
    return x, {"iterations": it, "col_iterations": col_it, "k_passes": passes, "restarts": restarts, "rel_residual": rel,
               "converged": ok}


class MatfreeReference:
    """fit(x, y, u) / predict(xt, cov) with the device's rules; the kernel matrices come from ``kernel`` / ``diag`` as in
    SparseReference.  K is held here (it is a reference); only its products are used."""

    def __init__(self, kernel, diag, diag_reg=1e-3, jitter=1e-8, absolute=False, tol=1e-10, max_iter=1000, columnwise=False):
        self.kernel, self.diag, self.diag_reg, self.jitter, self.absolute = kernel, diag, diag_reg, jitter, absolute
        self.tol, self.max_iter, self.columnwise = tol, max_iter, columnwise

    def fit(self, x, y, u=None, chunk_rows=None):
        self.x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(self.x.shape[0], -1)
        n = self.x.shape[0]
        self.k = self.kernel(self.x, None)
        self.sparse = None
        if u is not None and len(u) > 0:
            sp = self.sparse = S.SparseReference(self.kernel, self.diag, self.diag_reg, self.jitter, self.absolute).fit(self.x, y, u, chunk_rows)
            self.sigma2 = float(sp.sigma2)
            self.vt = scipy.linalg.solve_triangular(sp.lu, self.kernel(self.x, sp.u).T, lower=True).T  # [n, m]
            self.lb = sp.lb
        else:
            self.sigma2 = float(self.diag_reg if self.absolute else self.diag_reg * (np.sum(self.diag(self.x)) / n))
        self.alpha, self.fit_info = self.solve(y.T)  # [ny, n]
        return self

    def apply(self, v):
        """(K + sigma2 I) applied to the rows of v [r, n]."""
        return v @ self.k + self.sigma2 * v

    def precond(self, r):
        t = self.vt.T @ r.T                                                    # [m, r]
        w = scipy.linalg.solve_triangular(self.lb, scipy.linalg.solve_triangular(self.lb, t, lower=True), lower=True, trans="T")
        return (r - (self.vt @ w).T) / self.sigma2

    def solve(self, b, tol=None, max_iter=None):
        return pcg(self.apply, b, self.precond if self.sparse is not None else None, self.tol if tol is None else tol,
                   self.max_iter if max_iter is None else max_iter, self.columnwise)

    def predict(self, xt, cov="diag", rhs_cap=None):
        """mean [M, ny] (+ var [M] with cov='diag', and the list of the blocks' solver infos)."""
        xt = np.asarray(xt, dtype=np.float64)
        b = self.kernel(xt, self.x)                                            # [M, n]: one right-hand side per test row
        mean = b @ self.alpha.T
        if cov is None:
            return mean
        step = xt.shape[0] if rhs_cap is None else int(rhs_cap)
        var, infos = np.zeros(xt.shape[0]), []
        for r0 in range(0, xt.shape[0], step):
            z, info = self.solve(b[r0:r0 + step])
            var[r0:r0 + step] = self.diag(xt[r0:r0 + step]) - np.sum(b[r0:r0 + step] * z, axis=1)
            infos.append(info)
        return mean, var, infos


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest_n1000_m200.npz")


@functools.lru_cache(maxsize=None)
def forest():
    g = np.load(GOLDEN)
    return g["X_train"], g["Y_train"], g["X_test"], g["Y_test"]


@functools.lru_cache(maxsize=None)
def forest_picks(n_relu, n, m):
    """The reference's greedy inducing rows of the first n forest rows."""
    return S.greedy_inducing(S.oracle_kernel(n_relu)[0], forest()[0][:n], m)[0]


@functools.lru_cache(maxsize=None)
def forest_case(n_relu, n, m, with_var=True):
    """The shared reference of a forest case: n training rows, m greedy inducing rows (0: none), chunks of 256, the 200 test
    rows, and the oracle's exact posterior of the same case.  Computed once per process; callers must not modify it.
    Returns dict(ref, idx, mean, var, infos, oracle_mean, oracle_var, e_mean, e_var)."""
    import nngp_oracle as oracle
    x, y, xt, _ = forest()
    x, y = x[:n], y[:n]
    kernel, diag = S.oracle_kernel(n_relu)
    idx = forest_picks(n_relu, n, m) if m > 0 else np.zeros(0, dtype=np.int64)
    ref = MatfreeReference(kernel, diag).fit(x, y, x[idx] if m > 0 else None, chunk_rows=256)
    o_mean, o_cov = oracle.Posterior(x, y, oracle.make_arch(n_relu), 1e-3).predict(xt, "nngp", True)
    o_var = np.diag(o_cov)
    if with_var:
        mean, var, infos = ref.predict(xt, "diag")
        e_var = float(np.max(np.abs(var / o_var - 1.0)))
    else:
        mean, var, infos, e_var = ref.predict(xt, None), None, [], None
    e_mean = float(np.abs(mean - o_mean).max() / np.abs(o_mean).max())
    return dict(ref=ref, idx=idx, mean=mean, var=var, infos=infos, oracle_mean=o_mean, oracle_var=o_var, e_mean=e_mean, e_var=e_var)
