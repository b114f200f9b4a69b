"""NumPy float64 reference of the additive kernel over feature groups (include/nngp_additive.h) and the exact GP posterior
over it.  Test infrastructure only.

    K(x, x') = w0 K_arch(x, x') + sum_g w_g K_arch(x[:, b_g:e_g], x'[:, b_g:e_g])

Every term is the closed form on a column slice, with the slice's own normalisation 1 / d_g: oracle/nngp_oracle.kernel_fn for an
all-ReLU network, tests/activation_reference.kernel_fn for any other.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

import activation_reference as A
import nngp_oracle as oracle


def pair_groups(d):
    return [(i, i + 2) for i in range(0, d, 2)]


def _arch_kernel(x1, x2, get, w_std, b_std, acts):
    if acts is None or all(A._spec(a) == ("relu",) for a in acts):
        return oracle.kernel_fn(x1, x2, get, oracle.make_arch(len(w_std) - 1, list(w_std), list(b_std)))
    return A.kernel_fn(x1, x2, get, w_std, b_std, acts)


def same_slices(a, c):
    """[i, j]: row i of a and row j of c are the same vector, bit for bit."""
    return np.all(a[:, None, :] == c[None, :, :], axis=2)


def _terms(d, groups, weights, full_weight):
    weights = [1.0] * len(groups) if weights is None else list(weights)
    return [((b, e), w) for (b, e), w in list(zip(groups, weights)) + [((0, d), full_weight)] if w != 0.0]


def kernel_fn(x1, x2, get, w_std, b_std, acts, groups, weights=None, full_weight=1.0, exact_same=False):
    """The summed kernel (one of 'nngp', 'ntk').  x2 None: symmetric.  exact_same: an entry of a term whose two slices are
    bit-identical takes the diagonal form (theta = 0, q q' - k^2 = 0 exactly) instead of the square root of the Gram product's
    rounding noise -- what the oracle's formula means there, and what the ReLU oracle does not do even on its own diagonal."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = None if x2 is None else np.asarray(x2, dtype=np.float64)
    n2 = x1.shape[0] if x2 is None else x2.shape[0]
    out = np.zeros((x1.shape[0], n2))
    hidden = [("relu",)] * (len(w_std) - 1) if acts is None else acts
    for (b, e), w in _terms(x1.shape[1], groups, weights, full_weight):
        a, c = x1[:, b:e], None if x2 is None else x2[:, b:e]
        term = _arch_kernel(a, c, get, w_std, b_std, acts)
        if exact_same:
            same = same_slices(a, a if c is None else c)
            dn, dt = A.diag_kernel(a, w_std, b_std, hidden)
            term = np.where(same, (dn if get == "nngp" else dt)[:, None], term)
        out += w * term
    return out


def diag_kernel(x, w_std, b_std, acts, groups, weights=None, full_weight=1.0):
    """K(x, x) and Theta(x, x) per row of the summed kernel."""
    x = np.asarray(x, dtype=np.float64)
    acts = [("relu",)] * (len(w_std) - 1) if acts is None else acts
    dn, dt = np.zeros(x.shape[0]), np.zeros(x.shape[0])
    for (b, e), w in _terms(x.shape[1], groups, weights, full_weight):
        kn, kt = A.diag_kernel(x[:, b:e], w_std, b_std, acts)
        dn += w * kn
        dt += w * kt
    return dn, dt


def degenerate(x1, x2, groups, weights=None, full_weight=1.0, tol=1e-12, exclude_same=False):
    """Entries (i, j) at which some term of the sum sees two collinear, non-zero slices: there q q' - k^2 is pure rounding noise of
    the Gram product, so any two float64 evaluations of sqrt(q q' - k^2) differ at first order (the rule of the gate of
    tests/test_gpu_activations.py for rows that are the same vector, applied per term).  exclude_same: for a reference built with
    exact_same and a kernel that gives bit-identical slices the diagonal form.  The group terms do that for every pair of
    identical slices, so those do not count; the whole-input term (the kernel build of kernel_build.hip) does it on the diagonal
    of a symmetric build only (x2 None), so there only that diagonal does not count."""
    x1 = np.asarray(x1, dtype=np.float64)
    sym = x2 is None
    x2 = x1 if sym else np.asarray(x2, dtype=np.float64)
    mask = np.zeros((x1.shape[0], x2.shape[0]), dtype=bool)
    terms = _terms(x1.shape[1], groups, weights, 0.0) + ([((0, x1.shape[1]), None)] if full_weight != 0.0 else [])
    for (b, e), w in terms:
        a, c = x1[:, b:e], x2[:, b:e]
        k = a @ c.T
        qq = np.sum(a * a, axis=1)[:, None] * np.sum(c * c, axis=1)[None, :]
        term = (qq > 0.0) & (np.abs(qq - k * k) <= tol * qq)
        if exclude_same and w is not None:
            term &= ~same_slices(a, c)
        elif exclude_same and sym:
            term &= ~np.eye(x1.shape[0], dtype=bool)
        mask |= term
    return mask


def erf_ntk_conditioning(x1, x2, w_std, b_std, act, groups, weights=None, full_weight=1.0):
    """Dense, Erf(a, b, c), Dense: by how much two float64 evaluations of Theta may differ, entry by entry, because each rounds
    what enters r = 1 + 2 b^2 (q1' + q2') + 4 b^4 (q1' q2' - k'^2) in its own way.  With u = 2^-53: a Gram entry or squared norm
    over d_g features summed in some order is within (d_g + 1) u / 2 of its value in either evaluation, and the Dense layer's
    affine map w2 k + b2 adds up to 2 u more (two roundings; one in an fma, none when it is compensated).  So k', q1', q2' differ
    by up to (d_g + 3) u each between the two, the bracket q1' q2' - k'^2 by up to 4 (d_g + 3) u q1' q2', and that reaches
    Theta = w2_1 (kdot k' + K') through kdot = a^2 (4 / pi) b^2 / sqrt(r) and K' = a^2 (2 / pi) atan2(2 b^2 k', sqrt(r)).
    Large only where two slices are nearly parallel at a large norm, where r ~ 4 b^2 q is all that is left of r; nothing is added
    for a term whose two slices are bit-identical."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = x1 if x2 is None else np.asarray(x2, dtype=np.float64)
    _, ea, eb, _ = act
    w0, b0, w1 = float(w_std[0]) ** 2, float(b_std[0]) ** 2, float(w_std[1]) ** 2
    out = np.zeros((x1.shape[0], x2.shape[0]))
    for (b, e), w in _terms(x1.shape[1], groups, weights, full_weight):
        a, c = x1[:, b:e], x2[:, b:e]
        k = w0 * (a @ c.T) / (e - b) + b0
        q1 = (w0 * np.sum(a * a, axis=1) / (e - b) + b0)[:, None]
        q2 = (w0 * np.sum(c * c, axis=1) / (e - b) + b0)[None, :]
        r = A.stable_r(k, q1, q2, eb)
        dr = 4.0 * eb ** 4 * 4.0 * (e - b + 3) * 2.0 ** -53 * q1 * q2
        kdot = ea * ea * (4.0 / np.pi) * eb * eb / np.sqrt(r)
        u = 2.0 * eb * eb * np.abs(k)
        dk = ea * ea * (2.0 / np.pi) * u / (u * u + r) * dr / (2.0 * np.sqrt(r))
        # (bit-identical slices take the diagonal form in both evaluations: no bracket, nothing to add)
        out += np.where(same_slices(a, c), 0.0, w * w1 * (np.abs(k) * kdot * dr / (2.0 * r) + dk))
    return out


def erf_kernel_extended(x1, x2, get, w_std, b_std, act, groups, weights=None, full_weight=1.0):
    """Dense, Erf(a, b, c), Dense in np.longdouble (64-bit significand on x86): the same formulas with 11 more bits, to tell which
    of two float64 evaluations is nearer the value.  Returned in float64."""
    L = np.longdouble
    x1 = np.asarray(x1, dtype=np.float64).astype(L)
    x2 = x1 if x2 is None else np.asarray(x2, dtype=np.float64).astype(L)
    _, ea, eb, ec = (act[0],) + tuple(L(v) for v in act[1:])
    w0, b0, w1, b1 = L(w_std[0]) ** 2, L(b_std[0]) ** 2, L(w_std[1]) ** 2, L(b_std[1]) ** 2
    pi = L(np.pi) + L(1.2246467991473532e-16)  # pi to the longdouble's precision
    out = np.zeros((x1.shape[0], x2.shape[0]), dtype=L)
    for (b, e), w in _terms(x1.shape[1], groups, weights, full_weight):
        a, c = x1[:, b:e], x2[:, b:e]
        k = w0 * (a @ c.T) / L(e - b) + b0
        q1 = (w0 * np.sum(a * a, axis=1) / L(e - b) + b0)[:, None]
        q2 = (w0 * np.sum(c * c, axis=1) / L(e - b) + b0)[None, :]
        r = 1 + 2 * eb * eb * (q1 + q2) + 4 * eb ** 4 * np.maximum(q1 * q2 - k * k, 0)
        kn = ea * ea * (2 / pi) * np.arctan2(2 * eb * eb * k, np.sqrt(r)) + ec * ec
        kd = ea * ea * (4 / pi) * eb * eb / np.sqrt(r)
        out += L(w) * ((w1 * kn + b1) if get == "nngp" else (w1 * kn + b1 + w1 * kd * k))
    return out.astype(np.float64)


class Posterior:
    """Exact float64 GP posterior over the summed kernel (mean, full covariance; NNGP and NTK-ensemble formulas; regulariser
    relative to trace(K) / N)."""

    def __init__(self, x_train, y_train, w_std, b_std, acts, groups, weights=None, full_weight=1.0, diag_reg=1e-3):
        self.x = np.asarray(x_train, dtype=np.float64)
        self.y = np.asarray(y_train, dtype=np.float64).reshape(self.x.shape[0], -1)
        self.args = (w_std, b_std, acts, groups, weights, full_weight)
        self.diag_reg = diag_reg
        self._cache = {}

    def _k(self, x1, x2, get):
        return kernel_fn(x1, x2, get, *self.args)

    def _factor(self, get):
        if get not in self._cache:
            k_dd = self._k(self.x, None, get)
            n = k_dd.shape[0]
            c = scipy.linalg.cho_factor(k_dd + self.diag_reg * (np.trace(k_dd) / n) * np.eye(n), lower=True)
            self._cache[get] = (k_dd, c, scipy.linalg.cho_solve(c, self.y))
        return self._cache[get]

    def alpha(self, get="nngp"):
        return self._factor(get)[2]

    def predict(self, x_test, get="nngp", compute_cov=True):
        """mean [M, ny] and the full covariance [M, M] (its diagonal is the variance)."""
        k_dd, c, alpha = self._factor(get)
        x_test = np.asarray(x_test, dtype=np.float64)
        k_td = self._k(x_test, self.x, get)
        mean = k_td @ alpha
        if not compute_cov:
            return mean
        nngp_tt = self._k(x_test, None, "nngp")
        z = scipy.linalg.cho_solve(c, k_td.T)
        if get == "nngp":
            return mean, nngp_tt - k_td @ z
        nngp_td = self._k(x_test, self.x, "nngp")
        return mean, nngp_tt + z.T @ self._k(self.x, None, "nngp") @ z - (nngp_td @ z + (nngp_td @ z).T)
