"""NumPy float64 oracle of per-feature input relevances (include/nngp_ard.h).  Test infrastructure only.

K_s(x, x') = K(x o sqrt(s), x' o sqrt(s)): the value and the 2 n_dense + 1 gradient are nngp_mll_reference.Oracle /
nngp_loo_reference.Oracle on the scaled rows.  dK/ds_k comes from FORWARD mode -- the recursion of
nngp_mll_reference.kernel_block with a tangent seeded at the input, dK0_ij = x_ik x_jk / d, dq_i = x_ik^2 / d (the raw x), one
feature at a time -- a different method from the device's adjoint pass and contraction.  It is contracted with
alpha alpha^T and A^-1 for the NLML, and pushed through d alpha = -B dA alpha, d b = -diag(B dA B) for the leave-one-out
objectives, as nngp_loo_reference does for the other parameters.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_mll_reference as R  # noqa: E402
import nngp_loo_reference as L  # noqa: E402


def scaled(x, rel):
    return np.asarray(x, dtype=np.float64) * np.sqrt(np.asarray(rel, dtype=np.float64))[None, :]


def feature_tangent(x, rel, feat, v, c, acts):
    """dK / ds_feat [N, N] of the symmetric kernel of x at relevances rel."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    xs = scaled(x, rel)
    q = np.sum(xs * xs, axis=1) / d
    k = (xs @ xs.T) / d
    xk = x[:, feat]
    dq = xk * xk / d
    dk = np.outer(xk, xk) / d
    eye = np.eye(n, dtype=bool)
    k[eye] = q
    dk[eye] = dq
    q1, q2 = q[:, None].copy(), q[None, :].copy()
    dq1, dq2 = dq[:, None].copy(), dq[None, :].copy()
    nd = len(v)
    for l in range(nd):
        dk, dq1, dq2 = v[l] * dk, v[l] * dq1, v[l] * dq2
        k, q1, q2 = v[l] * k + c[l], v[l] * q1 + c[l], v[l] * q2 + c[l]
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
            kn, ck, cs = a * b * k + (b - a) ** 2 * kr, a * b + (b - a) ** 2 * kd, (b - a) ** 2 * s
        else:
            kn, ck, cs = kr, kd, s
        h = R._h(spec)
        kn = np.where(eye, h * k, kn)  # theta = 0: K' = h k, no q dependence
        ck = np.where(eye, h, ck)
        cs = np.where(eye, 0.0, cs)
        t1 = np.where(q1 > 0.0, cs / (4.0 * np.pi * np.where(q1 > 0.0, q1, 1.0)), 0.0)  # the q = 0 rule
        t2 = np.where(q2 > 0.0, cs / (4.0 * np.pi * np.where(q2 > 0.0, q2, 1.0)), 0.0)
        dk = ck * dk + t1 * dq1 + t2 * dq2
        k = kn
        q1, q2, dq1, dq2 = h * q1, h * q2, h * dq1, h * dq2
    return dk


class Oracle:
    """NLML (objective None) or a leave-one-out objective ('nlpd' / 'mse') on (x, y) with relevances."""

    def __init__(self, x, y, objective=None, block=512):
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.objective, self.block = objective, block

    def value(self, v, c, acts, lam, rel, absolute=False):
        xs = scaled(self.x, rel)
        if self.objective is None:
            return R.Oracle(xs, self.y, self.block).nlml_var(v, c, [R._spec(a) for a in acts], lam, absolute)
        return L.Oracle(xs, self.y, self.objective, self.block).value_var(v, c, acts, lam, absolute)

    def full(self, v, c, acts, lam, rel, absolute=False, with_grad=True):
        """The dict of nngp_mll_reference.Oracle.full (or nngp_loo_reference's) on the scaled rows and, with_grad: grad_s [d],
        half1_s / half2_s (the cancelling halves per feature, as nngp_mll_ard_terms) and tr_dk_s."""
        acts = [R._spec(a) for a in acts]
        rel = np.asarray(rel, dtype=np.float64)
        xs = scaled(self.x, rel)
        n, d = xs.shape
        if self.objective is None:
            base = R.Oracle(xs, self.y, self.block)
            out = base.full(v, c, acts, lam, absolute, with_grad)
            out["value"] = out["nlml"]
        else:
            base = L.Oracle(xs, self.y, self.objective, self.block)
            out = base.full(v, c, acts, lam, absolute, with_grad)
        if not with_grad:
            return out
        k = (base if self.objective is None else base._k).kernel(v, c, acts)
        r = lam if absolute else lam * np.trace(k) / n
        cf = scipy.linalg.cho_factor(k + r * np.eye(n), lower=True)
        alpha = scipy.linalg.cho_solve(cf, self.y)
        binv = scipy.linalg.cho_solve(cf, np.eye(n))
        h1, h2, trdk = np.zeros(d), np.zeros(d), np.zeros(d)
        if self.objective is None:
            aa, tr_b = float(alpha @ alpha), float(np.trace(binv))
        else:
            bsq = np.sum(binv * binv, axis=1)
            abar, bbar = out["abar"], out["bbar"]
        for f in range(d):
            dk = feature_tangent(self.x, rel, f, v, c, acts)
            trdk[f] = np.trace(dk)
            ci = 0.0 if absolute else lam * trdk[f] / n
            if self.objective is None:
                h1[f] = alpha @ (dk @ alpha) + ci * aa
                h2[f] = np.sum(binv * dk) + ci * tr_b
            else:
                dalpha = -(binv @ (dk @ alpha + ci * alpha))
                db = -(np.sum((binv @ dk) * binv, axis=1) + ci * bsq)
                h1[f] = -(abar @ dalpha)
                h2[f] = -(bbar @ db)
        out.update(grad_s=(-0.5 * h1 + 0.5 * h2) if self.objective is None else -(h1 + h2), half1_s=h1, half2_s=h2, tr_dk_s=trdk)
        return out

    def evaluate(self, params, diag_reg, absolute=False, with_grad=True, relevance=None):
        """The evaluator interface of mll / loo.tune_hyperparameters: params = (w_std, b_std, activations)."""
        w, b, acts = params
        v, c = R.variances(w, b)
        if relevance is None:  # the return shape of the oracles without relevances
            base = (R.Oracle(self.x, self.y, self.block) if self.objective is None
                    else L.Oracle(self.x, self.y, self.objective, self.block))
            return base.evaluate(params, diag_reg, absolute, with_grad)
        o = self.full(v, c, acts, diag_reg, relevance, absolute, with_grad)
        if not with_grad:
            return o["value"], None, None
        return o["value"], o["grad"], o["grad_s"]
