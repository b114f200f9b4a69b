"""NumPy float64 reference of per-feature input relevances on the sparse NNGP evidence (include/nngp_sparse_ard.h).
Test infrastructure only.

K_s(x, x') = K(x o sqrt(s), x' o sqrt(s)): the value and the 2 n_dense + 1 gradient are sparse_evidence_reference.SparseEvidence on
the scaled rows X o sqrt(s), U o sqrt(s).  dK/ds_k comes from FORWARD mode: the layer recursion of
sparse_evidence_reference.kernel_rect with a tangent seeded at its input, (dK0, dq_i, dq_j) = (1, 0, 0), (0, 1, 0), (0, 0, 1),
gives c = dK/dK0, e1 = dK/dq_i, e2 = dK/dq_j per entry, and

    dK_ij/ds_k = (1/d) [ c_ij x_ik u_jk + e1_ij x_ik^2 + e2_ij u_jk^2 ]        (the raw rows; every entry the general formula)

over the rectangular block; the symmetric K_uu takes nngp_ard_reference.feature_tangent with its exact diagonal.  quad_k and
trace_k are assembled densely -- a different method from the device's adjoint sweep and contraction.  ``dtype=np.longdouble``
reruns the linear algebra and the contractions in 80-bit arithmetic on the same float64 kernel blocks and tangents, as a referee.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_ard_reference as AR  # noqa: E402
import nngp_mll_reference as MR  # noqa: E402
import sparse_evidence_reference as E  # noqa: E402
import sparse_reference as S  # noqa: E402


def rect_tangent(x1, x2, v, c, acts, seed):
    """K(x1, x2) [n1, n2] by the general formula and its tangent for the input seed (dK0, dq_i, dq_j), each 0 or 1."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = np.asarray(x2, dtype=np.float64)
    d = x1.shape[1]
    k = (x1 @ x2.T) / d
    q1 = (np.sum(x1 * x1, axis=1) / d)[:, None]
    q2 = (np.sum(x2 * x2, axis=1) / d)[None, :]
    dk = np.full_like(k, float(seed[0]))
    dq1 = np.full_like(q1, float(seed[1]))
    dq2 = np.full_like(q2, float(seed[2]))
    nd = len(v)
    for l in range(nd):
        dk, dq1, dq2 = v[l] * dk, v[l] * dq1, v[l] * dq2
        k, q1, q2 = v[l] * k + c[l], v[l] * q1 + c[l], v[l] * q2 + c[l]
        if l == nd - 1:
            break
        spec = MR._spec(acts[l])
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
        h = MR._h(spec)
        t1 = np.where(q1 > 0.0, cs / (4.0 * np.pi * np.where(q1 > 0.0, q1, 1.0)), 0.0)  # the q = 0 rule
        t2 = np.where(q2 > 0.0, cs / (4.0 * np.pi * np.where(q2 > 0.0, q2, 1.0)), 0.0)
        dk = ck * dk + t1 * dq1 + t2 * dq2
        k = kn
        q1, q2, dq1, dq2 = h * q1, h * q2, h * dq1, h * dq2
    return k, dk


def input_tangents(x, u, rel, v, c, acts):
    """(K, c, e1, e2) of the block K(x o sqrt(rel), u o sqrt(rel)): the kernel and its derivatives with respect to K0_ij, q_i, q_j."""
    xs, us = AR.scaled(x, rel), AR.scaled(u, rel)
    k, cm = rect_tangent(xs, us, v, c, acts, (1, 0, 0))
    e1 = rect_tangent(xs, us, v, c, acts, (0, 1, 0))[1]
    e2 = rect_tangent(xs, us, v, c, acts, (0, 0, 1))[1]
    return k, cm, e1, e2


def contract_rect(seed, x, u, cm, e1, e2, dtype=np.float64):
    """sum_ij seed_ij dK_ij/ds_k for every k [d]: (1/d) [ x_k^T (seed o c) u_k + (x_k^2)^T rowsum(seed o e1) + colsum(seed o e2)^T u_k^2 ]."""
    seed = np.asarray(seed, dtype=dtype)
    x, u = np.asarray(x, dtype=dtype), np.asarray(u, dtype=dtype)
    sc = seed * cm.astype(dtype)
    r1 = np.sum(seed * e1.astype(dtype), axis=1)
    c2 = np.sum(seed * e2.astype(dtype), axis=0)
    d = x.shape[1]
    return (np.sum(x * (sc @ u), axis=0) + (x * x).T @ r1 + (u * u).T @ c2) / d


def d0v0(v, acts):
    """dK_ii/dq_i in closed form: prod of the hidden layers' h and of every v_l."""
    out = 1.0
    for l in range(len(v)):
        out *= v[l]
        if l < len(v) - 1:
            out *= MR._h(MR._spec(acts[l]))
    return out


class SparseArdEvidence:
    """Value, gradient and relevance gradient of the sparse evidence on (x, y) with the raw inducing rows u held fixed."""

    def __init__(self, x, y, u, jitter=1e-8, chunk_rows=None, dtype=np.float64):
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.u = np.asarray(u, dtype=np.float64)
        self.jitter, self.chunk_rows, self.dtype = float(jitter), chunk_rows, dtype
        self._tan = {}

    def base(self, rel):
        return E.SparseEvidence(AR.scaled(self.x, rel), self.y, AR.scaled(self.u, rel), self.jitter, self.chunk_rows, self.dtype)

    def value(self, v, c, acts, lam, rel, absolute=False, bound="vfe"):
        return self.base(rel).full(v, c, acts, lam, absolute, bound, with_grad=False)["nlml"]

    def tangents(self, v, c, acts, rel):
        """The float64 tangents, shared by every bound / absolute flag / dtype at the same kernel: (K_fu, c, e1, e2), [dK_uu/ds_k]."""
        key = (tuple(v), tuple(c), tuple(map(tuple, acts)), tuple(np.asarray(rel, dtype=np.float64)))
        if key not in self._tan:
            self._tan.clear()
            rect = input_tangents(self.x, self.u, rel, v, c, acts)
            uu = [AR.feature_tangent(self.u, rel, f, v, c, acts) for f in range(self.x.shape[1])]
            self._tan[key] = (rect, uu)
        return self._tan[key]

    def full(self, v, c, acts, lam, rel, absolute=False, bound="vfe", with_grad=True):
        """The dict of sparse_evidence_reference.SparseEvidence.full on the scaled rows and, with_grad: grad_s, quad_s, trace_s [d],
        tr_dkff_s, tr_dkuu_s [d]."""
        acts = [MR._spec(a) for a in acts]
        rel = np.asarray(rel, dtype=np.float64)
        dt = self.dtype
        base = self.base(rel)
        out = base.full(v, c, acts, lam, absolute, bound, with_grad)
        if not with_grad:
            return out
        ref = base.fit(v, c, acts, lam, absolute)
        n, m, d = ref.n, self.u.shape[0], self.x.shape[1]
        vfe = bound == "vfe"
        y = self.y.astype(dt)
        s2 = ref.sigma2
        lui, lbi = E._inv_lower(ref.lu, dt), E._inv_lower(ref.lb, dt)
        ainv = lui.T @ lui
        z = lbi @ lui
        mm = z.T @ z
        gamma = z.T @ (lbi @ ref.r[:, 0])
        (kfu64, cm, e1, e2), duu = self.tangents(v, c, acts, rel)
        kfu = kfu64.astype(dt)
        # gamma solves (K~_uu + K_uf K_fu / sigma2) gamma = K_uf y / sigma2, whose inverse is sigma2 M.  Out of the triangular inverses it
        # carries cond(K~_uu) eps, and beta = (y - K_fu gamma) / sigma2 magnifies that by |K_fu| / sigma2: enough to reach 1e-9 of the
        # halves of a feature whose halves are small.  Two steps of iterative refinement with the residual in 80-bit arithmetic remove
        # it from the float64 reference (the 80-bit rerun takes them too; they change nothing there).
        ext = np.longdouble
        kfu_x, kuu_x, y_x = kfu64.astype(ext), ref.kuu.astype(ext), self.y.astype(ext)
        for _ in range(2):
            g_x = gamma.astype(ext)
            resid = kfu_x.T @ ((y_x - kfu_x @ g_x) / ext(s2)) - kuu_x @ g_x
            gamma = gamma + s2 * (mm @ resid.astype(dt))
        beta = ((y_x - kfu_x @ gamma.astype(ext)) / ext(s2)).astype(dt)
        pm = ainv - s2 * mm
        tr_binv = np.sum(lbi * lbi)
        bb, gg = beta @ beta, gamma @ gamma
        dmat = kfu @ (mm - ainv / s2 if vfe else mm)
        emat = -pm + ((lui.T @ ref.g @ lui) / s2 if vfe else 0.0)
        ts = (n - m + s2 * tr_binv) / s2 - ((ref.tr - np.trace(ref.g)) / (s2 * s2) if vfe else 0.0)
        jm = dt(self.jitter) / m
        dv = dt(d0v0(v, acts))
        xr, ur = self.x.astype(dt), self.u.astype(dt)
        trdk_f = dv * np.sum(xr * xr, axis=0) / d
        trdk_u = dv * np.sum(ur * ur, axis=0) / d
        fu_q = contract_rect(np.outer(beta, gamma), self.x, self.u, cm, e1, e2, dt)
        fu_t = contract_rect(dmat, self.x, self.u, cm, e1, e2, dt)
        quad, trace = np.zeros(d, dtype=dt), np.zeros(d, dtype=dt)
        tr_e = np.trace(emat)
        for f in range(d):
            dk = duu[f].astype(dt)
            ds2 = 0.0 if absolute else dt(lam) * trdk_f[f] / n
            quad[f] = 2 * fu_q[f] - (gamma @ (dk @ gamma) + jm * np.trace(dk) * gg) + bb * ds2
            trace[f] = 2 * fu_t[f] + (np.sum(emat * dk) + jm * np.trace(dk) * tr_e) + ts * ds2 + (trdk_f[f] / s2 if vfe else 0.0)
        out.update(grad_s=-0.5 * quad + 0.5 * trace, quad_s=quad, trace_s=trace, tr_dkff_s=trdk_f, tr_dkuu_s=trdk_u)
        return out

    def evaluate64(self, v, c, acts, lam, rel, absolute=False, bound="vfe", with_grad=True):
        o = self.full(v, c, acts, lam, rel, absolute, bound, with_grad)
        return {k: (np.asarray(val, dtype=np.float64) if isinstance(val, np.ndarray) else float(val)) for k, val in o.items()}


class Evaluator:
    """The evaluator interface of mll.tune_loop with relevances on the NumPy reference:
    evaluate((w_std, b_std, acts), diag_reg, absolute, with_grad, relevance=) -> (value, grad, grad_s)."""

    def __init__(self, x, y, u, bound="vfe", jitter=1e-8, chunk_rows=None):
        self.ref, self.bound = SparseArdEvidence(x, y, u, jitter, chunk_rows), bound

    def evaluate(self, params, diag_reg, absolute=False, with_grad=True, relevance=None):
        w, b, acts = params
        v, c = MR.variances(w, b)
        rel = np.ones(self.ref.x.shape[1]) if relevance is None else relevance
        o = self.ref.evaluate64(v, c, acts, diag_reg, rel, absolute, self.bound, with_grad)
        if relevance is None:
            return o["nlml"], (o["grad"] if with_grad else None)
        return o["nlml"], (o["grad"] if with_grad else None), (o["grad_s"] if with_grad else None)


def distance(a, b):
    """(value, gradient, relevance gradient): sparse_evidence_reference.distance, and the largest |grad_s difference| over
    max(|quad_k|, |trace_k|)."""
    val, grad = E.distance(a, b)
    scale = np.maximum(np.abs(np.asarray(b["quad_s"], dtype=np.float64)), np.abs(np.asarray(b["trace_s"], dtype=np.float64)))
    diff = np.abs(np.asarray(a["grad_s"], dtype=np.float64) - np.asarray(b["grad_s"], dtype=np.float64))
    return val, grad, float(np.max(diff / scale))


def exact_grad_s(x, y, rel, v, c, acts, lam, absolute=False, dtype=np.float64):
    """The relevance gradient of the EXACT NLML (the method of nngp_ard_reference.Oracle) with its linear algebra in ``dtype``:
    (grad_s, half1, half2).  The referee of the exact limit U = X, jitter 0."""
    acts = [MR._spec(a) for a in acts]
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    k = MR.Oracle(AR.scaled(x, rel), y).kernel(v, c, acts).astype(dtype)
    r = dtype(lam) if absolute else dtype(lam) * np.trace(k) / n
    li = E._inv_lower(S._chol(k + r * np.eye(n, dtype=dtype), dtype), dtype)
    binv = li.T @ li
    alpha = binv @ np.asarray(y, dtype=dtype).reshape(-1)
    aa, tr_b = alpha @ alpha, np.trace(binv)
    h1, h2 = np.zeros(d, dtype=dtype), np.zeros(d, dtype=dtype)
    for f in range(d):
        dk = AR.feature_tangent(x, rel, f, v, c, acts).astype(dtype)
        ci = 0.0 if absolute else dtype(lam) * np.trace(dk) / n
        h1[f] = alpha @ (dk @ alpha) + ci * aa
        h2[f] = np.sum(binv * dk) + ci * tr_b
    return -0.5 * h1 + 0.5 * h2, h1, h2


def relevances(d, seed=11, sigma=0.3, zero_at=3):
    """Log-normal relevances from a fixed seed, one of them exactly 0."""
    s = np.exp(sigma * np.random.default_rng(seed).standard_normal(d))
    s[zero_at] = 0.0
    return s


# ---- the cases of tests/test_gpu_sparse_ard.py; test_sparse_ard_host.py checks the reference's own error on each ----
SHAPES = ((300, 70, 128), (1000, 129, 1024), (1000, 200, 256))  # n, m, chunk_rows
NETS = (  # the 2-dense, 4-dense and 3-dense-ABRelu nets of sparse_evidence_reference.cases(), each with its rows
    (([1.2] * 2, [0.0] * 2, [("relu",)]), "unit"),
    (([1.2] * 4, [0.05] * 4, [("relu",)] * 3), "centred"),
    (([1.2] * 3, [0.05] * 3, [("abrelu", 0.1, 1.0)] * 2), "unit"),
)
LAM = 1e-3


def cases():
    """[(n, m, chunk_rows, bound, absolute, (w_std, b_std, acts), rows)], the layout of sparse_evidence_reference.cases()"""
    return [(n, m, chunk, bound, absolute, net, rows) for n, m, chunk in SHAPES for net, rows in NETS for bound in E.BOUNDS
            for absolute in (False, True)]


case_id = E.case_id
_SETUP, _CASES = {}, {}


def case_setup(golden_dir, case):
    """(x, y, relevances, inducing indices, float64 evaluator, 80-bit evaluator) shared by the cases of one shape and net."""
    n, m, chunk, _, _, (w, b, acts), rows = case
    key = (n, m, chunk, len(w), rows)
    if key not in _SETUP:
        x, y = E.case_rows(golden_dir, rows, n)
        rel = relevances(x.shape[1])
        v, c = MR.variances(w, b)
        idx, _ = S.greedy_inducing(E.kernels(v, c, acts)[0], AR.scaled(x, rel), m)
        r64 = SparseArdEvidence(x, y, x[idx], E.JITTER, chunk)
        r80 = SparseArdEvidence(x, y, x[idx], E.JITTER, chunk, dtype=np.longdouble)
        r80._tan = r64._tan  # the same float64 tangents
        _SETUP[key] = (x, y, rel, idx, r64, r80)
    return _SETUP[key]


def case_reference(golden_dir, case, with_longdouble=True):
    """(x, y, relevances, inducing indices, float64 result, its distance to the 80-bit rerun) of one case, computed once."""
    key = (case_id(case), with_longdouble)
    if key not in _CASES:
        _, _, _, bound, absolute, (w, b, acts), _ = case
        x, y, rel, idx, r64, r80 = case_setup(golden_dir, case)
        v, c = MR.variances(w, b)
        ref = r64.evaluate64(v, c, acts, LAM, rel, absolute, bound)
        dist = distance(ref, r80.full(v, c, acts, LAM, rel, absolute, bound)) if with_longdouble else None
        _CASES[key] = (x, y, rel, idx, ref, dist)
    return _CASES[key]
