"""NumPy float64 oracle of the NNGP marginal likelihood and its gradient (include/nngp_mll.h).  Test infrastructure only.

K is the closed form of tests/activation_reference.py (ReLU and ABRelu, exact diagonal; its ReLU case agrees with
oracle/nngp_oracle.py off the diagonal, test_nngp_mll_host.py checks it).  dK/dtheta_p comes from FORWARD-mode tangents
pushed through the layer recursion beside K -- a different method from the device's adjoint sweep -- one parameter at a time,
in blocks of rows, contracted with alpha alpha^T and A^-1 from scipy's Cholesky.  The q = 0 rule of the header holds here
too: a ReLU input with q = 0 passes no tangent on from q.  Parameters are variances: v_l = W_std_l^2, c_l = b_std_l^2.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activation_reference as AR  # noqa: E402

LOG_2PI = math.log(2.0 * math.pi)


def _spec(a):
    return AR._spec(a)


def _h(spec):
    return 0.5 * (spec[1] ** 2 + spec[2] ** 2) if spec[0] == "abrelu" else 0.5


def kernel_block(x, rows, v, c, acts, param=None):
    """K[rows, :] of the symmetric kernel of x and, with param = p (0 .. 2 nd - 1; 2 l: v_l, 2 l + 1: c_l), its tangent
    dK[rows, :] / dtheta_p."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    q_all = np.sum(x * x, axis=1) / d
    xr = x[rows]
    k = (xr @ x.T) / d
    q1 = q_all[rows][:, None].copy()
    q2 = q_all[None, :].copy()
    ri = np.arange(x.shape[0])[rows]
    diag = (ri[:, None] == np.arange(x.shape[0])[None, :])
    k[diag] = np.broadcast_to(q1, k.shape)[diag]
    dk = np.zeros_like(k)
    dq1 = np.zeros_like(q1)
    dq2 = np.zeros_like(q2)
    nd = len(v)
    for l in range(nd):
        on_v = param == 2 * l
        on_c = param == 2 * l + 1
        dk = v[l] * dk + (k if on_v else 0.0) + (1.0 if on_c else 0.0)
        dq1 = v[l] * dq1 + (q1 if on_v else 0.0) + (1.0 if on_c else 0.0)
        dq2 = v[l] * dq2 + (q2 if on_v else 0.0) + (1.0 if on_c else 0.0)
        k = v[l] * k + c[l]
        q1 = v[l] * q1 + c[l]
        q2 = v[l] * q2 + c[l]
        if l == nd - 1:
            break
        spec = _spec(acts[l])
        s = np.sqrt(np.maximum(q1 * q2 - k * k, 0.0))
        th = np.arctan2(s, k)
        th = np.where((s == 0.0) & (k == 0.0), np.pi / 2, th)
        kd = (np.pi - th) / (2 * np.pi)
        kr = s / (2 * np.pi) + kd * k
        if spec[0] == "abrelu":
            a, b = spec[1], spec[2]
            kn, ck, cs = a * b * k + (b - a) ** 2 * kr, a * b + (b - a) ** 2 * kd, (b - a) ** 2 * s
        else:
            kn, ck, cs = kr, kd, s
        h = _h(spec)
        kn[diag] = (h * k)[diag]  # theta = 0: K' = h k, dK'/dk = h, no q dependence
        ck = np.where(diag, h, ck)
        cs = np.where(diag, 0.0, cs)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = np.where(q1 > 0.0, cs / (4.0 * np.pi * np.where(q1 > 0.0, q1, 1.0)), 0.0)
            t2 = np.where(q2 > 0.0, cs / (4.0 * np.pi * np.where(q2 > 0.0, q2, 1.0)), 0.0)
        dk = ck * dk + t1 * dq1 + t2 * dq2
        k = kn
        q1, q2, dq1, dq2 = h * q1, h * q2, h * dq1, h * dq2
    return k, (dk if param is not None else None)


def variances(w_std, b_std):
    return [float(w) ** 2 for w in w_std], [float(b) ** 2 for b in b_std]


class Oracle:
    """NLML and gradient of the NNGP evidence on (x, y) (y one column, uncentred)."""

    def __init__(self, x, y, block=512):
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.block = block

    def kernel(self, v, c, acts):
        n = self.x.shape[0]
        return np.concatenate([kernel_block(self.x, slice(r, min(r + self.block, n)), v, c, acts)[0]
                               for r in range(0, n, self.block)], axis=0)

    def nlml_var(self, v, c, acts, lam, absolute=False):
        """NLML as a function of the variances (for finite differences)."""
        k = self.kernel(v, c, acts)
        n = k.shape[0]
        r = lam if absolute else lam * (np.trace(k) / n)
        cf = scipy.linalg.cho_factor(k + r * np.eye(n), lower=True)
        alpha = scipy.linalg.cho_solve(cf, self.y)
        return 0.5 * self.y @ alpha + np.sum(np.log(np.diag(cf[0]))) + 0.5 * n * LOG_2PI

    def full(self, v, c, acts, lam, absolute=False, with_grad=True):
        """dict: nlml, grad (2 nd + 1), quad / trace halves (as nngp_mll_terms), tr_k, tr_dk, a_a, tr_ainv, cond."""
        acts = [_spec(a) for a in acts]
        n = self.x.shape[0]
        nd = len(v)
        k = self.kernel(v, c, acts)
        tr_k = float(np.trace(k))
        r = lam if absolute else lam * (tr_k / n)
        a = k + r * np.eye(n)
        cf = scipy.linalg.cho_factor(a, lower=True)
        alpha = scipy.linalg.cho_solve(cf, self.y)
        out = {"tr_k": tr_k, "logdet_half": float(np.sum(np.log(np.diag(cf[0])))), "y_ainv_y": float(self.y @ alpha)}
        out["nlml"] = 0.5 * out["y_ainv_y"] + out["logdet_half"] + 0.5 * n * LOG_2PI
        if not with_grad:
            return out
        ainv = scipy.linalg.cho_solve(cf, np.eye(n))
        aa, tr_ainv = float(alpha @ alpha), float(np.trace(ainv))
        nc = 2 * nd
        qk, tk, trdk = np.zeros(nc), np.zeros(nc), np.zeros(nc)
        for p in range(nc):
            for r0 in range(0, n, self.block):
                rows = slice(r0, min(r0 + self.block, n))
                _, dk = kernel_block(self.x, rows, v, c, acts, param=p)
                qk[p] += alpha[rows] @ (dk @ alpha)
                tk[p] += np.sum(ainv[rows] * dk)
                trdk[p] += np.trace(dk[:, rows])
        quad, trace = np.zeros(nc + 1), np.zeros(nc + 1)
        for p in range(nc):
            ci = 0.0 if absolute else lam * trdk[p] / n
            quad[p], trace[p] = qk[p] + ci * aa, tk[p] + ci * tr_ainv
        ci = 1.0 if absolute else tr_k / n
        quad[nc], trace[nc] = ci * aa, ci * tr_ainv
        out.update(grad=-0.5 * quad + 0.5 * trace, quad=quad, trace=trace, tr_dk=trdk, a_a=aa, tr_ainv=tr_ainv)
        return out

    def evaluate(self, params, diag_reg, absolute=False, with_grad=True):
        """The evaluator interface of mll.tune_hyperparameters: params = (w_std, b_std, activations)."""
        w, b, acts = params
        v, c = variances(w, b)
        o = self.full(v, c, acts, diag_reg, absolute, with_grad)
        return o["nlml"], (o["grad"] if with_grad else None)
