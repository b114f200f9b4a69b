"""NumPy float64 oracle of leave-one-out cross-validation (include/nngp_loo.h).  Test infrastructure only.

A = K + r I (K from nngp_mll_reference.kernel_block; Theta from ntk_kernel below), r = lambda tr / N or lambda, held at its
full-data value when a point is left out.  With B = A^-1, alpha = B y, b = diag B:
    residual r_i = alpha_i / b_i,  mean mu_i = y_i - r_i,  variance s_i = 1 / b_i
    mse = mean r_i^2,  nlpd = mean [1/2 log(2 pi s_i) + r_i^2 / (2 s_i)]
The gradient comes from FORWARD mode, one parameter at a time: d alpha = -B dA_p alpha, d b_i = -(B dA_p B)_ii with dA_p from
kernel_block's tangents -- a different method from the device's adjoint pass.  The two cancelling halves of a component are
-abar . d alpha and -bbar . d b.  brute_force() refits without point i; long_double() repeats the closed form in long double.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_mll_reference as R  # noqa: E402
import extended_precision as EP  # noqa: E402

OBJECTIVES = ("nlpd", "mse")


def ntk_kernel(x, v, c, acts):
    """Theta of the symmetric kernel of x: Dense: Theta <- K' + v Theta; activation: Theta <- (dK'/dk) Theta.  Exact diagonal
    (theta = 0: dK'/dk = h), as for K."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    q = np.sum(x * x, axis=1) / d
    k = (x @ x.T) / d
    k[np.diag_indices(n)] = q
    q1, q2 = q[:, None].copy(), q[None, :].copy()
    t = np.zeros_like(k)
    eye = np.eye(n, dtype=bool)
    nd = len(v)
    for l in range(nd):
        k = v[l] * k + c[l]
        q1 = v[l] * q1 + c[l]
        q2 = v[l] * q2 + c[l]
        t = k + v[l] * t
        if l == nd - 1:
            break
        spec = R._spec(acts[l])
        s = np.sqrt(np.maximum(q1 * q2 - k * k, 0.0))
        th = np.arctan2(s, k)
        th = np.where((s == 0.0) & (k == 0.0), np.pi / 2, th)
        kd = (np.pi - th) / (2 * np.pi)
        kr = s / (2 * np.pi) + kd * k
        if spec[0] == "abrelu":
            a, b = spec[1], spec[2]
            kn, ck = a * b * k + (b - a) ** 2 * kr, a * b + (b - a) ** 2 * kd
        else:
            kn, ck = kr, kd
        h = R._h(spec)
        k = np.where(eye, h * k, kn)
        t = np.where(eye, h, ck) * t
        q1, q2 = h * q1, h * q2
    return t


def point_terms(alpha, b, y, objective):
    """dict: resid, mean, var, mse, nlpd and the objective's abar = dL/dalpha, bbar = dL/db."""
    n = alpha.shape[0]
    r = alpha / b
    s = 1.0 / b
    out = {"resid": r, "mean": y - r, "var": s, "mse": float(np.mean(r * r)),
           "nlpd": float(np.mean(0.5 * np.log(2 * math.pi * s) + r * r / (2 * s)))}
    if objective == "mse":
        out["abar"], out["bbar"] = 2 * r / (n * b), -2 * r * r / (n * b)
    else:
        out["abar"], out["bbar"] = alpha / (n * b), -(1 / b + alpha ** 2 / b ** 2) / (2 * n)
    out["value"] = out[objective]
    return out


class Oracle:
    """LOO predictions, objective and gradient on (x, y) (y one column, uncentred)."""

    def __init__(self, x, y, objective="nlpd", block=512, get="nngp"):
        assert objective in OBJECTIVES and get in ("nngp", "ntk")
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.objective, self.block, self.get = objective, block, get
        self._k = R.Oracle(self.x, self.y, block)

    def matrix(self, v, c, acts, lam, absolute=False):
        """(A, tr K, r)"""
        acts = [R._spec(a) for a in acts]
        k = self._k.kernel(v, c, acts) if self.get == "nngp" else ntk_kernel(self.x, v, c, acts)
        n = k.shape[0]
        tr = float(np.trace(k))
        r = lam if absolute else lam * tr / n
        return k + r * np.eye(n), tr, r

    def value_var(self, v, c, acts, lam, absolute=False, objective=None):
        """The objective as a function of the variances (for finite differences)."""
        a, _, _ = self.matrix(v, c, acts, lam, absolute)
        b = np.linalg.inv(a)
        b = 0.5 * (b + b.T)
        return point_terms(b @ self.y, np.diag(b).copy(), self.y, objective or self.objective)["value"]

    def full(self, v, c, acts, lam, absolute=False, with_grad=True, objective=None):
        """dict: value, mse, nlpd, resid, mean, var, tr_k and, with_grad: grad (2 nd + 1), half1 / half2 (as
        nngp_mll_loo_terms), a_u, tr_c, tr_dk, cond."""
        objective = objective or self.objective
        acts = [R._spec(a) for a in acts]
        n, nd = self.x.shape[0], len(v)
        a, tr_k, _ = self.matrix(v, c, acts, lam, absolute)
        cf = scipy.linalg.cho_factor(a, lower=True)
        alpha = scipy.linalg.cho_solve(cf, self.y)
        if not with_grad:  # b from the rows of L^-1, without A^-1
            linv = scipy.linalg.solve_triangular(cf[0], np.eye(n), lower=True)
            out = point_terms(alpha, np.sum(linv * linv, axis=0), self.y, objective)
            out["tr_k"] = tr_k
            return out
        core = self._tangents(cf, alpha, v, c, acts, lam, absolute, tr_k)
        binv, bsq, trdk, dalpha, db = core
        out = point_terms(alpha, np.diag(binv).copy(), self.y, objective)
        out["tr_k"] = tr_k
        abar, bbar = out["abar"], out["bbar"]
        nc = 2 * nd
        h1 = np.array([-(abar @ dalpha[p]) for p in range(nc + 1)])
        h2 = np.array([-(bbar @ db[p]) for p in range(nc + 1)])
        out.update(grad=-(h1 + h2), half1=h1, half2=h2, a_u=float(alpha @ (binv @ abar)), tr_c=float(bsq @ bbar), tr_dk=trdk)
        return out

    def _tangents(self, cf, alpha, v, c, acts, lam, absolute, tr_k):
        """(B, (B^2)_ii, tr dK_p, [d alpha / d theta_p], [d b / d theta_p]) for p = 0 .. 2 nd (the last: lambda); the last call's
        result is kept, so that both objectives at one point share the N^3 work."""
        key = (tuple(v), tuple(c), tuple(acts), lam, absolute)
        if getattr(self, "_tan_key", None) == key:
            return self._tan
        n, nc = self.x.shape[0], 2 * len(v)
        binv = scipy.linalg.cho_solve(cf, np.eye(n))
        bsq = np.sum(binv * binv, axis=1)  # (B I B)_ii
        trdk, dalpha, db = np.zeros(nc), [], []
        for p in range(nc):
            dk = np.concatenate([R.kernel_block(self.x, slice(r0, min(r0 + self.block, n)), v, c, acts, param=p)[1]
                                 for r0 in range(0, n, self.block)], axis=0)
            trdk[p] = np.trace(dk)
            ci = 0.0 if absolute else lam * trdk[p] / n
            dalpha.append(-(binv @ (dk @ alpha + ci * alpha)))
            db.append(-(np.sum((binv @ dk) * binv, axis=1) + ci * bsq))
        ci = 1.0 if absolute else tr_k / n
        dalpha.append(-ci * (binv @ alpha))
        db.append(-ci * bsq)
        self._tan_key, self._tan = key, (binv, bsq, trdk, dalpha, db)
        return self._tan

    def brute_force(self, v, c, acts, lam, absolute=False):
        """(mean, var) by refitting without point i, with r held at its full-data value."""
        a, _, _ = self.matrix(v, c, acts, lam, absolute)
        n = a.shape[0]
        mean, var = np.zeros(n), np.zeros(n)
        for i in range(n):
            keep = np.arange(n) != i
            cf = scipy.linalg.cho_factor(a[np.ix_(keep, keep)], lower=True)
            ki = a[i, keep]
            mean[i] = ki @ scipy.linalg.cho_solve(cf, self.y[keep])
            var[i] = a[i, i] - ki @ scipy.linalg.cho_solve(cf, ki)
        return mean, var

    def long_double(self, v, c, acts, lam, absolute=False):
        """dict resid, var, mse, nlpd (float64 values of a long-double evaluation of the closed form from the float64 A)."""
        a, _, _ = self.matrix(v, c, acts, lam, absolute)
        n = a.shape[0]
        l = EP.cholesky_ld(a)
        sol = EP.solve_ld(l, np.concatenate([self.y[:, None], np.eye(n)], axis=1))
        alpha, b = sol[:, 0], np.diagonal(sol[:, 1:]).copy()
        r, s = alpha / b, 1 / b
        two_pi = 2 * np.longdouble(math.pi)
        return {"resid": r.astype(np.float64), "var": s.astype(np.float64), "mse": float(np.mean(r * r)),
                "nlpd": float(np.mean(0.5 * np.log(two_pi * s) + r * r / (2 * s))), "cond": float(np.linalg.cond(a))}

    def evaluate(self, params, diag_reg, absolute=False, with_grad=True):
        """The evaluator interface of loo.tune_hyperparameters: params = (w_std, b_std, activations)."""
        w, b, acts = params
        v, c = R.variances(w, b)
        o = self.full(v, c, acts, diag_reg, absolute, with_grad)
        return o["value"], (o["grad"] if with_grad else None)
