"""NumPy float64 restatement of the NNGP / NTK recursion of Dense,(act,Dense)* with act in {Relu, ABRelu, Erf}, and the exact
GP posterior over it (NNGP and NTK ensemble), in the way oracle/nngp_oracle.py does it for ReLU.  Test infrastructure only.

Activations are given per hidden layer as ("relu",), ("abrelu", a, b) or ("erf", a, b, c) (stax.KernelFn.activations).
Per hidden layer, after its Dense layer (k: cross entry, q1 / q2: the diagonals; NTK: Theta <- kdot Theta):
  ABRelu(a, b):  s = sqrt(max(q1 q2 - k^2, 0)), theta = atan2(s, k)
                 K' = a b k + (b - a)^2 (s + (pi - theta) k) / 2 pi,  kdot = a b + (b - a)^2 (pi - theta) / 2 pi,  q' = (a^2 + b^2) q / 2
  Erf(a, b, c):  u = 2 b^2 k,  r = 1 + 2 b^2 (q1 + q2) + 4 b^4 (q1 q2 - k^2) (bracket from exact products),  w = sqrt(r)
                 K' = a^2 (2 / pi) atan2(u, w) + c^2,  kdot = a^2 (4 / pi) b^2 / w,  q' = a^2 (2 / pi) asin(2 b^2 q / (1 + 2 b^2 q)) + c^2
The diagonal of a symmetric kernel uses the q' / diagonal kdot forms (theta = 0, q1 q2 - k^2 = 0 exactly).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg


def _spec(a):
    a = tuple(a)
    if a[0] == "abrelu" and float(a[1]) == 0.0 and float(a[2]) == 1.0:
        return ("relu",)
    return a


def act_diag(spec, q):
    """(q', kdot) of a diagonal entry q."""
    spec = _spec(spec)
    q = np.asarray(q, dtype=np.float64)
    if spec[0] == "relu":
        return 0.5 * q, np.full_like(q, 0.5)
    if spec[0] == "abrelu":
        a, b = spec[1], spec[2]
        h = 0.5 * (a * a + b * b)
        return h * q, np.full_like(q, h)
    a, b, c = spec[1], spec[2], spec[3]
    w = np.sqrt(1.0 + 4.0 * b * b * q)
    return a * a * (2.0 / np.pi) * np.arctan2(2.0 * b * b * q, w) + c * c, a * a * (4.0 / np.pi) * b * b / w


def stable_r(k, q1, q2, b):
    """r = 1 + 2 b^2 (q1 + q2) + 4 b^4 (q1 q2 - k^2), the bracket from exact products (what the kernel computes, to an ulp)."""
    p1, e1 = _two_prod(q1, q2)
    p2, e2 = _two_prod(k, k)
    br = np.maximum((p1 - p2) + (e1 - e2), 0.0)
    return 1.0 + 2.0 * b * b * (q1 + q2) + 4.0 * b ** 4 * br


def naive_r(k, q1, q2, b):
    """(1 + 2 b^2 q1)(1 + 2 b^2 q2) - u^2: the same number, formed by a cancelling difference."""
    u = 2.0 * b * b * k
    return (1.0 + 2.0 * b * b * q1) * (1.0 + 2.0 * b * b * q2) - u * u


def _two_prod(a, b):
    """(p, e) with p = fl(a b) and p + e == a b exactly (Dekker's split)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = a * b
    sp = 134217729.0
    ah = a * sp; ah = ah - (ah - a); al = a - ah
    bh = b * sp; bh = bh - (bh - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def act_cross(spec, k, q1, q2):
    """(K', kdot) of cross entries k with diagonals q1 (rows) and q2 (columns), broadcast."""
    spec = _spec(spec)
    if spec[0] in ("relu", "abrelu"):
        s = np.sqrt(np.maximum(q1 * q2 - k * k, 0.0))
        th = np.arctan2(s, k)
        th = np.where((s == 0.0) & (k == 0.0), np.pi / 2, th)
        kd = (np.pi - th) / (2 * np.pi)
        kr = s / (2 * np.pi) + kd * k
        if spec[0] == "relu":
            return kr, kd
        a, b = spec[1], spec[2]
        return a * b * k + (b - a) ** 2 * kr, a * b + (b - a) ** 2 * kd
    a, b, c = spec[1], spec[2], spec[3]
    w = np.sqrt(stable_r(k, q1, q2, b))
    return a * a * (2.0 / np.pi) * np.arctan2(2.0 * b * b * k, w) + c * c, a * a * (4.0 / np.pi) * b * b / w


def kernel_fn(x1, x2, get, w_std, b_std, acts):
    """Closed-form kernel(s) of Dense,(act,Dense)*.  x2 None: symmetric, with the exact diagonal."""
    x1 = np.asarray(x1, dtype=np.float64)
    sym = x2 is None
    x2 = x1 if sym else np.asarray(x2, dtype=np.float64)
    d = x1.shape[1]
    k = (x1 @ x2.T) / d
    q1 = np.sum(x1 * x1, axis=1) / d
    q2 = np.sum(x2 * x2, axis=1) / d
    if sym:
        k[np.diag_indices_from(k)] = q1
    t = np.zeros_like(k)
    nd = len(w_std)
    assert len(b_std) == nd and len(acts) == nd - 1
    for layer in range(nd):
        w2, b2 = float(w_std[layer]) ** 2, float(b_std[layer]) ** 2
        k = w2 * k + b2
        q1 = w2 * q1 + b2
        q2 = w2 * q2 + b2
        t = k + w2 * t
        if layer < nd - 1:
            kn, kd = act_cross(acts[layer], k, q1[:, None], q2[None, :])
            if sym:
                dq, dkd = act_diag(acts[layer], np.diag(k))
                kn[np.diag_indices_from(kn)] = dq
                kd[np.diag_indices_from(kd)] = dkd
            k, t = kn, kd * t
            q1 = act_diag(acts[layer], q1)[0]
            q2 = act_diag(acts[layer], q2)[0]
    if isinstance(get, (tuple, list)):
        return tuple({"nngp": k, "ntk": t}[g] for g in get)
    return {"nngp": k, "ntk": t}[get]


def diag_kernel(x, w_std, b_std, acts):
    """K(x, x) and Theta(x, x) per row."""
    x = np.asarray(x, dtype=np.float64)
    k = np.sum(x * x, axis=1) / x.shape[1]
    t = np.zeros_like(k)
    nd = len(w_std)
    for layer in range(nd):
        w2, b2 = float(w_std[layer]) ** 2, float(b_std[layer]) ** 2
        k = w2 * k + b2
        t = k + w2 * t
        if layer < nd - 1:
            k, kd = act_diag(acts[layer], k)
            t = kd * t
    return k, t


class Posterior:
    """Exact float64 GP posterior over the restated kernel (gradient_descent_mse_ensemble at t = inf, relative regulariser)."""

    def __init__(self, x_train, y_train, w_std, b_std, acts, diag_reg=1e-3):
        self.x = np.asarray(x_train, dtype=np.float64)
        self.y = np.asarray(y_train, dtype=np.float64).reshape(self.x.shape[0], -1)
        self.arch = (list(w_std), list(b_std), list(acts))
        self.diag_reg = diag_reg
        self._cache = {}

    def _k(self, x1, x2, get):
        return kernel_fn(x1, x2, get, *self.arch)

    def _factor(self, get):
        if get not in self._cache:
            k_dd = self._k(self.x, None, get)
            n = k_dd.shape[0]
            a = k_dd + self.diag_reg * (np.trace(k_dd) / n) * np.eye(n)
            c = scipy.linalg.cho_factor(a, lower=True)
            self._cache[get] = (k_dd, c, scipy.linalg.cho_solve(c, self.y))
        return self._cache[get]

    def predict(self, x_test, get="nngp", compute_cov=True):
        """mean [M, ny] and the full covariance [M, M] (its diagonal is the variance)."""
        k_dd, c, alpha = self._factor(get)
        x_test = np.asarray(x_test, dtype=np.float64)
        k_td = self._k(x_test, self.x, get)
        mean = k_td @ alpha
        if not compute_cov:
            return mean
        nngp_tt = self._k(x_test, None, "nngp")
        if get == "nngp":
            return mean, nngp_tt - k_td @ scipy.linalg.cho_solve(c, k_td.T)
        nngp_dd = k_dd if get == "nngp" else self._k(self.x, None, "nngp")
        nngp_td = self._k(x_test, self.x, "nngp")
        z = scipy.linalg.cho_solve(c, k_td.T)
        return mean, nngp_tt + z.T @ nngp_dd @ z - (nngp_td @ z + (nngp_td @ z).T)
