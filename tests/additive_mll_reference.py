"""NumPy float64 oracle of the additive NNGP kernel's marginal likelihood and its gradient, the term weights included
(include/nngp_additive_mll.h).  Test infrastructure only.

K = sum_t w_t K^(t): term 0 is nngp_mll_reference.kernel_block on the whole rows, term t >= 1 the same function on the column
slice of group t - 1 (its own 1 / d_t), with forward-mode tangents for the layer parameters -- a different method from the
device's adjoint sweep.  A group term takes the diagonal form wherever the two slices are identical (k_build_add's rule): value
and tangent of such an entry are those of the row's diagonal entry, which goes through the k chain alone.  A term of weight 0 is
left out of K, dK/dtheta and the traces and still gets its own d/dw_t.  scipy Cholesky; halves per weight and per layer
parameter; per-term traces.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_mll_reference as R  # noqa: E402


def term_block(x, rows, v, c, acts, group=None, param=None):
    """K^(t)[rows, :] and (with param) its tangent: the whole input (group None) or the slice ``group = (begin, end)``."""
    if group is None:
        return R.kernel_block(x, rows, v, c, acts, param)
    xs = np.ascontiguousarray(x[:, group[0]:group[1]])
    k, dk = R.kernel_block(xs, rows, v, c, acts, param)
    ri = np.arange(xs.shape[0])[rows]
    same = np.all(xs[ri][:, None, :] == xs[None, :, :], axis=2)  # identical slices, the diagonal among them
    loc = np.arange(ri.shape[0])
    k = np.where(same, k[loc, ri][:, None], k)
    if dk is not None:
        dk = np.where(same, dk[loc, ri][:, None], dk)
    return k, dk


class Oracle:
    """NLML, gradient and weight gradient of the additive evidence on (x, y) with the (begin, end) ranges ``groups``."""

    def __init__(self, x, y, groups, block=512):
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.groups = [None] + [(int(b), int(e)) for b, e in groups]
        self.block = block

    def _blocks(self):
        n = self.x.shape[0]
        return [slice(r, min(r + self.block, n)) for r in range(0, n, self.block)]

    def term(self, t, v, c, acts, param=None):
        """K^(t), or its tangent with param, as a full matrix."""
        return np.concatenate([term_block(self.x, rows, v, c, acts, self.groups[t], param)[0 if param is None else 1]
                               for rows in self._blocks()], axis=0)

    def kernel(self, v, c, acts, weights):
        """(K, [K^(t)]) -- the groups with w_g > 0 in the table's order, then the whole input (the build's order)."""
        terms = [self.term(t, v, c, acts) for t in range(len(self.groups))]
        k = np.zeros_like(terms[0])
        for t in list(range(1, len(terms))) + [0]:
            if weights[t] != 0.0:
                k = k + weights[t] * terms[t]
        return k, terms

    def nlml_var(self, v, c, acts, lam, weights, absolute=False):
        """NLML as a function of the variances and the weights (for finite differences)."""
        k, _ = self.kernel(v, c, acts, weights)
        n = k.shape[0]
        r = lam if absolute else lam * (np.trace(k) / n)
        cf = scipy.linalg.cho_factor(k + r * np.eye(n), lower=True)
        alpha = scipy.linalg.cho_solve(cf, self.y)
        return 0.5 * self.y @ alpha + np.sum(np.log(np.diag(cf[0]))) + 0.5 * n * R.LOG_2PI

    def full(self, v, c, acts, lam, weights, absolute=False, with_grad=True):
        """dict: nlml, grad (2 nd + 1), quad / trace (as nngp_mll_terms), tr_k, tr_dk, grad_w, half1_w / half2_w and tr_k_term
        (as nngp_mll_additive_terms), a_a, tr_ainv."""
        acts = [R._spec(a) for a in acts]
        weights = np.asarray(weights, dtype=np.float64).reshape(-1)
        assert weights.shape[0] == len(self.groups)
        n, nd = self.x.shape[0], len(v)
        k, terms = self.kernel(v, c, acts, weights)
        tr_k = float(np.trace(k))
        r = lam if absolute else lam * (tr_k / n)
        cf = scipy.linalg.cho_factor(k + r * np.eye(n), lower=True)
        alpha = scipy.linalg.cho_solve(cf, self.y)
        out = {"tr_k": tr_k, "logdet_half": float(np.sum(np.log(np.diag(cf[0])))), "y_ainv_y": float(self.y @ alpha)}
        out["nlml"] = 0.5 * out["y_ainv_y"] + out["logdet_half"] + 0.5 * n * R.LOG_2PI
        if not with_grad:
            return out
        ainv = scipy.linalg.cho_solve(cf, np.eye(n))
        aa, tr_ainv = float(alpha @ alpha), float(np.trace(ainv))
        nc, nt = 2 * nd, len(self.groups)
        h1w, h2w, trkt = np.zeros(nt), np.zeros(nt), np.zeros(nt)
        for t in range(nt):
            trkt[t] = np.trace(terms[t])
            ci = 0.0 if absolute else lam * trkt[t] / n
            h1w[t] = alpha @ (terms[t] @ alpha) + ci * aa
            h2w[t] = np.sum(ainv * terms[t]) + ci * tr_ainv
        qk, tk, trdk = np.zeros(nc), np.zeros(nc), np.zeros(nc)
        for p in range(nc):
            for t in range(nt):
                if weights[t] == 0.0:
                    continue
                dk = self.term(t, v, c, acts, param=p)
                qk[p] += weights[t] * (alpha @ (dk @ alpha))
                tk[p] += weights[t] * np.sum(ainv * dk)
                trdk[p] += weights[t] * np.trace(dk)
        quad, trace = np.zeros(nc + 1), np.zeros(nc + 1)
        for p in range(nc):
            ci = 0.0 if absolute else lam * trdk[p] / n
            quad[p], trace[p] = qk[p] + ci * aa, tk[p] + ci * tr_ainv
        ci = 1.0 if absolute else tr_k / n
        quad[nc], trace[nc] = ci * aa, ci * tr_ainv
        out.update(grad=-0.5 * quad + 0.5 * trace, quad=quad, trace=trace, tr_dk=trdk, a_a=aa, tr_ainv=tr_ainv,
                   grad_w=-0.5 * h1w + 0.5 * h2w, half1_w=h1w, half2_w=h2w, tr_k_term=trkt)
        return out

    def evaluate(self, params, diag_reg, absolute=False, with_grad=True, weights=None):
        """The evaluator interface of additive_mll.tune_hyperparameters: params = (w_std, b_std, activations)."""
        w, b, acts = params
        v, c = R.variances(w, b)
        o = self.full(v, c, acts, diag_reg, weights, absolute, with_grad)
        return o["nlml"], (o["grad"] if with_grad else None), (o["grad_w"] if with_grad else None)
