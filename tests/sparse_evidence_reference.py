"""NumPy float64 reference of the sparse (inducing-point) NNGP evidence and its gradient (include/nngp_sparse_evidence.h).
Test infrastructure only.

With the quantities of sparse_reference.SparseReference (L_u, G, R, sigma2, B = sigma2 I + G = L_B L_B^T, C = L_B^-1 R), ny = 1:

    NLML_dtc = 1/2 (y^T y - |C|^2) / sigma2 + 1/2 [(n - m) log sigma2 + 2 sum_i log (L_B)_ii] + (n / 2) log 2 pi
    NLML_vfe = NLML_dtc + (tr K_ff - tr G) / (2 sigma2)                                    (Titsias' collapsed bound)

The gradient with respect to v_l = W_std_l^2, c_l = b_std_l^2 and lambda = diag_reg, the inducing rows held fixed, is written
as -1/2 quad + 1/2 trace like the exact evidence's: ``quad`` = beta^T dSigma beta holds everything that comes from
beta = Sigma^-1 y and gamma = K~_uu^-1 K_uf beta, ``trace`` = tr(Sigma^-1 dSigma) (plus twice the derivative of the VFE term) the
rest.  dK/dtheta comes from FORWARD-mode tangents: ``kernel_rect`` is nngp_mll_reference.kernel_block extended to a rectangular
block K(X1, X2) with no diagonal rule (what the device's cross build computes), the symmetric K_uu is kernel_block itself -- a
different method from the device's adjoint sweeps.  ``dtype=np.longdouble`` reruns the linear algebra (factorisations, solves,
products, sums) in 80-bit arithmetic on the same float64 kernel blocks and tangents, as a referee.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_mll_reference as MR  # noqa: E402
import sparse_reference as S  # noqa: E402

LOG_2PI = math.log(2.0 * math.pi)
BOUNDS = ("dtc", "vfe")


def kernel_rect(x1, x2, v, c, acts, param=None):
    """K(x1, x2) [n1, n2] by the general formula for every entry and, with param = p, its tangent dK / dtheta_p."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = np.asarray(x2, dtype=np.float64)
    d = x1.shape[1]
    k = (x1 @ x2.T) / d
    q1 = (np.sum(x1 * x1, axis=1) / d)[:, None]
    q2 = (np.sum(x2 * x2, axis=1) / d)[None, :]
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
        t1 = np.where(q1 > 0.0, cs / (4.0 * np.pi * np.where(q1 > 0.0, q1, 1.0)), 0.0)
        t2 = np.where(q2 > 0.0, cs / (4.0 * np.pi * np.where(q2 > 0.0, q2, 1.0)), 0.0)
        dk = ck * dk + t1 * dq1 + t2 * dq2
        k = kn
        q1, q2, dq1, dq2 = h * q1, h * q2, h * dq1, h * dq2
    return k, (dk if param is not None else None)


def kernel_diag(x, v, c, acts, param=None):
    """K(x_i, x_i) [n] in closed form (theta = 0: every activation multiplies by h) and its tangent."""
    x = np.asarray(x, dtype=np.float64)
    q = np.sum(x * x, axis=1) / x.shape[1]
    dq = np.zeros_like(q)
    nd = len(v)
    for l in range(nd):
        dq = v[l] * dq + (q if param == 2 * l else 0.0) + (1.0 if param == 2 * l + 1 else 0.0)
        q = v[l] * q + c[l]
        if l < nd - 1:
            h = MR._h(MR._spec(acts[l]))
            q, dq = h * q, h * dq
    return q, (dq if param is not None else None)


def kernels(v, c, acts):
    """(kernel, diag) callables for SparseReference: the symmetric build has the exact diagonal, the cross build has not."""
    acts = [MR._spec(a) for a in acts]

    def kernel(x1, x2=None):
        if x2 is None:
            return MR.kernel_block(x1, slice(None), v, c, acts)[0]
        return kernel_rect(x1, x2, v, c, acts)[0]

    def diag(x):
        return kernel_diag(x, v, c, acts)[0]

    return kernel, diag


def _inv_lower(l, dtype):
    return S._solve_lower(l, np.eye(l.shape[0], dtype=dtype), dtype)


class SparseEvidence:
    """Value and gradient of the sparse evidence on (x, y) with the inducing rows u held fixed."""

    def __init__(self, x, y, u, jitter=1e-8, chunk_rows=None, dtype=np.float64):
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.u = np.asarray(u, dtype=np.float64)
        self.jitter, self.chunk_rows, self.dtype = float(jitter), chunk_rows, dtype

    def fit(self, v, c, acts, lam, absolute=False):
        kernel, diag = kernels(v, c, acts)
        return S.SparseReference(kernel, diag, lam, self.jitter, absolute, self.dtype).fit(self.x, self.y, self.u, self.chunk_rows)

    def value_var(self, v, c, acts, lam, absolute=False, bound="vfe"):
        """The value as a function of the variances (for finite differences)."""
        return float(self.full(v, c, acts, lam, absolute, bound, with_grad=False)["nlml"])

    def full(self, v, c, acts, lam, absolute=False, bound="vfe", with_grad=True):
        """dict: nlml, grad (2 nd + 1), quad / trace halves, and the scalar sums of nngp_sparse_evidence_terms."""
        if bound not in BOUNDS:
            raise ValueError("bound must be 'dtc' or 'vfe', got %r" % (bound,))
        acts = [MR._spec(a) for a in acts]
        dt = self.dtype
        ref = self.fit(v, c, acts, lam, absolute)
        n, m = ref.n, self.u.shape[0]
        y = self.y.astype(dt)
        vfe = bound == "vfe"
        s2 = ref.sigma2
        cvec = ref.c[:, 0]
        logdet_half = np.sum(np.log(np.diag(ref.lb)))
        yy_cc = y @ y - cvec @ cvec
        tr_kff, tr_g = ref.tr, np.trace(ref.g)
        nlml = 0.5 * yy_cc / s2 + 0.5 * (n - m) * np.log(s2) + logdet_half + dt(0.5 * n * LOG_2PI)
        if vfe:
            nlml = nlml + (tr_kff - tr_g) / (2 * s2)
        out = {"nlml": nlml, "logdet_half": logdet_half, "yy_cc": yy_cc, "tr_kff": tr_kff, "tr_g": tr_g, "sigma2": s2,
               "cond_kuu": float(np.linalg.cond(ref.kuu.astype(np.float64)))}
        if not with_grad:
            return out
        nd = len(v)
        nc = 2 * nd
        lui, lbi = _inv_lower(ref.lu, dt), _inv_lower(ref.lb, dt)
        ainv = lui.T @ lui                      # K~_uu^-1
        z = lbi @ lui
        mm = z.T @ z                            # M = L_u^-T B^-1 L_u^-1
        gamma = z.T @ (lbi @ ref.r[:, 0])       # L_u^-T L_B^-T C
        kfu = kernel_rect(self.x, self.u, v, c, acts)[0].astype(dt)
        beta = (y - kfu @ gamma) / s2
        pm = ainv - s2 * mm
        tr_binv = np.sum(lbi * lbi)
        bb = beta @ beta
        # the seeds in "trace" units (twice the S of the gradient formula): D on K_fu, E on K~_uu
        dmat = kfu @ (mm - ainv / s2 if vfe else mm)
        emat = -pm + ((lui.T @ ref.g @ lui) / s2 if vfe else 0.0)
        ts = (n - m + s2 * tr_binv) / s2 - ((tr_kff - tr_g) / (s2 * s2) if vfe else 0.0)
        jm = dt(self.jitter) / m
        quad, trace, trdk_f = np.zeros(nc + 1, dtype=dt), np.zeros(nc + 1, dtype=dt), np.zeros(nc, dtype=dt)
        for p in range(nc):
            dkfu = kernel_rect(self.x, self.u, v, c, acts, param=p)[1].astype(dt)
            dkuu = MR.kernel_block(self.u, slice(None), v, c, acts, param=p)[1].astype(dt)
            dkuu = dkuu + jm * np.trace(dkuu) * np.eye(m, dtype=dt)  # the jitter scales with tr K_uu
            trdk_f[p] = np.sum(kernel_diag(self.x, v, c, acts, param=p)[1].astype(dt))
            ds2 = 0.0 if absolute else dt(lam) * trdk_f[p] / n
            quad[p] = 2 * (beta @ (dkfu @ gamma)) - gamma @ (dkuu @ gamma) + bb * ds2
            trace[p] = 2 * np.sum(dmat * dkfu) + np.sum(emat * dkuu) + ts * ds2 + (trdk_f[p] / s2 if vfe else 0.0)
        ci = 1.0 if absolute else tr_kff / n
        quad[nc], trace[nc] = bb * ci, ts * ci
        out.update(grad=-0.5 * quad + 0.5 * trace, quad=quad, trace=trace, tr_binv=tr_binv, b_b=bb, tr_dkff=trdk_f)
        return out

    def evaluate64(self, v, c, acts, lam, absolute=False, bound="vfe", with_grad=True):
        o = self.full(v, c, acts, lam, absolute, bound, with_grad)
        return {k: (np.asarray(val, dtype=np.float64) if isinstance(val, np.ndarray) else float(val)) for k, val in o.items()}


class Evaluator:
    """The evaluator interface of mll.tune_loop on the NumPy reference: evaluate((w_std, b_std, acts), diag_reg, absolute, with_grad)."""

    def __init__(self, x, y, u, bound="vfe", jitter=1e-8, chunk_rows=None):
        self.ref, self.bound = SparseEvidence(x, y, u, jitter, chunk_rows), bound

    def evaluate(self, params, diag_reg, absolute=False, with_grad=True):
        w, b, acts = params
        v, c = MR.variances(w, b)
        o = self.ref.evaluate64(v, c, acts, diag_reg, absolute, self.bound, with_grad)
        return o["nlml"], (o["grad"] if with_grad else None)


def distance(a, b):
    """How far two results of ``full`` are apart, in the units of the GPU gate: (value, relative; gradient, the largest
    |difference| / max(|quad_p|, |trace_p|))."""
    val = abs(float(a["nlml"]) - float(b["nlml"])) / abs(float(b["nlml"]))
    scale = np.maximum(np.abs(np.asarray(b["quad"], dtype=np.float64)), np.abs(np.asarray(b["trace"], dtype=np.float64)))
    diff = np.abs(np.asarray(a["grad"], dtype=np.float64) - np.asarray(b["grad"], dtype=np.float64))
    return val, float(np.max(diff / scale))


# ---- the cases of tests/test_gpu_sparse_evidence.py; test_sparse_evidence_host.py checks the reference's own error on each ----
SHAPES = ((300, 70, 128), (1000, 200, 256), (1000, 129, 1024))  # n, m, chunk_rows
CONFIGS = (  # bound, absolute, Dense layers, b_std, rows -- every shape meets both levels of each
    ("vfe", False, 2, 0.0, "unit"),
    ("dtc", True, 4, 0.05, "centred"),
    ("vfe", True, 2, 0.05, "centred"),
    ("dtc", False, 4, 0.0, "unit"),
)
LEAKY = ((1000, 200, 256), ("vfe", False, 3, 0.05, "unit"))
JITTER = 1e-8
COND_CAP = 1e5


def cases():
    """[(n, m, chunk_rows, bound, absolute, (w_std, b_std, acts), rows)]"""
    out = []
    for n, m, chunk in SHAPES:
        for bound, absolute, nd, b_std, rows in CONFIGS:
            out.append((n, m, chunk, bound, absolute, ([1.2] * nd, [b_std] * nd, [("relu",)] * (nd - 1)), rows))
    (n, m, chunk), (bound, absolute, nd, b_std, rows) = LEAKY
    out.append((n, m, chunk, bound, absolute, ([1.2] * nd, [b_std] * nd, [("abrelu", 0.1, 1.0)] * (nd - 1)), rows))
    return out


def case_id(case):
    n, m, chunk, bound, absolute, (w, b, acts), rows = case
    return "n%d-m%d-c%d-%s-%s-%ddense-b%g-%s-%s" % (n, m, chunk, bound, "abs" if absolute else "rel", len(w), b[0], acts[0][0], rows)


def case_rows(golden_dir, rows, n):
    """Forest golden rows scaled as in test_gpu_nngp_mll.py: "unit" (x / 1000) and "centred" (x / 1000 minus the column means)."""
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    x = np.concatenate([g["X_train"], g["X_test"]])[:n] / 1000.0
    y = np.concatenate([g["Y_train"], g["Y_test"]])[:n].reshape(-1)
    return (x - x.mean(0) if rows == "centred" else x), y


_CASE_CACHE = {}


def case_reference(golden_dir, case, with_longdouble=True):
    """(x, y, inducing indices, float64 result, distance of it to the 80-bit rerun (value, gradient)) of one case, computed once."""
    key = (case_id(case), with_longdouble)
    if key not in _CASE_CACHE:
        n, m, chunk, bound, absolute, (w, b, acts), rows = case
        x, y = case_rows(golden_dir, rows, n)
        v, c = MR.variances(w, b)
        idx, _ = S.greedy_inducing(kernels(v, c, acts)[0], x, m)
        lam = 1e-3
        ref = SparseEvidence(x, y, x[idx], JITTER, chunk).evaluate64(v, c, acts, lam, absolute, bound)
        dist = None
        if with_longdouble:
            dist = distance(ref, SparseEvidence(x, y, x[idx], JITTER, chunk, dtype=np.longdouble).full(v, c, acts, lam, absolute, bound))
        _CASE_CACHE[key] = (x, y, idx, ref, dist)
    return _CASE_CACHE[key]


# ---- the exact limit (U = X, jitter 0), on the host and on the device ----
EXACT_NETS = [([1.0, 1.0], [0.0, 0.0], [("relu",)]), ([1.2, 0.9, 1.1], [0.05, 0.1, 0.02], [("relu",), ("abrelu", 0.1, 1.0)])]


def exact_limit(x, y, net, absolute, lam):
    """({bound: (sparse reference at U = X with jitter 0, 10 x its distance to its 80-bit rerun as (value, gradient))}, the exact
    reference of nngp_mll_reference.py)."""
    w, b, acts = net
    v, c = MR.variances(w, b)
    exact = MR.Oracle(x, y).full(v, c, acts, lam, absolute)
    out = {}
    for bound in BOUNDS:
        got = SparseEvidence(x, y, x, jitter=0.0).evaluate64(v, c, acts, lam, absolute, bound)
        ld = SparseEvidence(x, y, x, jitter=0.0, dtype=np.longdouble).full(v, c, acts, lam, absolute, bound)
        out[bound] = (got, tuple(10.0 * d for d in distance(got, ld)))
    return out, exact
