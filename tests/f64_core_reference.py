"""Referee, float64 restatement, matrix families and per-entry gates for the float64 Cholesky core (csrc/gp_f64.hip: k_chol_diag,
potrf_f64, trsm_fwd_f64, k_rowdot, factor_and_solve).  Test infrastructure only: never imported by the product.  CPU only.

The referee is tests/extended_precision.py (80-bit): cholesky_ld for L, the forward half of solve_ld for L^-1 B, dinv and L^-T,
solve_ld for A^-1, its diagonal and alpha.  The restatement (potrf, trsm_fwd, factor_and_solve below) follows the device's blocked
algorithm in float64 NumPy -- the unblocked right-looking factor of a 128 x 128 block, its inverse by forward substitution, the
panel as a product with dinv^T, the full trailing update, the left-looking solve of two products per block column with the row
ranges of the triangular mode -- with every block step vectorised, so its sums run in NumPy's order, not the device's.  It
exists to measure what honest float64 code of this method gives, not to be compared with the device bit for bit.

Every error is a per-entry maximum in units of u = 2^-53 times a scale that comes from the referee or from the operands:
  *_bwd   |L L^T - A|_ij               over (|L| |L|^T)_ij            (lower triangle; the product in 80-bit)
  L_fwd   |L - L*|_ij                  over max_j |L*_ij|             (row scale: invariant under D A D)
  dinv_fwd|dinv - L*_kk^-1|_ij         over max_i |.|_ij              (column scale: dinv of D A D is dinv D^-1)
  dinv_res|dinv L_kk - I|_ij           over (|dinv| |L_kk|)_ij        (the solver's own L_kk)
  *_res   |X L^T - B|_ij               over (|X| |L^T|)_ij            (the solver's own L; s128 / s384 / tri: B random / I; w: B = y)
  s*_fwd  |X - B L*^-T|_ij             over (|B| |L*^-T|)_ij          (likewise w_fwd with B = y)
  tri_fwd, zt_fwd  |Z - L*^-T|_ij      over max_j |L*^-T|_ij
  ainv_fwd|. - A*^-1|_ij               over sqrt(A*^-1_ii A*^-1_jj)
  alpha_fwd |. - A*^-1 y|_i            over (|L*^-T| |L*^-1 y|)_i
  nrs_fwd |neg_rowsq + A*^-1_ii|       over A*^-1_ii
(* = the referee's).  The gate of a quantity is max(4 x the larger of the restatement's and float64 LAPACK / NumPy's figure, 4) u
for that family and size, both measured on the CPU against the referee (MEASURED below; tests/test_f64_core_host.py measures
them again, prints them and holds both to the gate).  4 x is the margin of the adjoint tests: the device sums the same terms in
another order on the MFMA with fused accumulation, and rounding bounds do not depend on the order beyond a small constant.
No device result took part in any figure.  "LAPACK" is numpy.linalg.cholesky, scipy.linalg.solve_triangular and cho_solve; its
figures were recorded with one BLAS thread and move by up to 1.5 x with the thread count (another blocking), inside the gate.

Families (n rows): rbf (4-d uniform points, length scale 0.7, noise 1e-2 / 1e-6 / 1e-10: rbf2, rbf6, rbf10), nngp (the oracle's
one-hidden-layer ReLU kernel of the forest fixture's rows / 1000 plus 1e-3 / 1e-8 of its mean diagonal: nngp3, nngp8), scaled
(D rbf6 D, D = diag(2^e), e uniform integers in [-100, 100]) and exact (L0 = diag(2^e) + N, see exact()).

Measured figures, largest over the sizes of the family (units of u; restatement / LAPACK; MEASURED at the end of the file holds
every size and every quantity, as tests/test_f64_core_host.py prints them):
  potrf and trsm_fwd, n in {128, 256, 384, 640}
          L_bwd         L_fwd             dinv_fwd          dinv_res    s384_res    s384_fwd          tri_res     tri_fwd
  rbf2    33 / 23       3.0e2 / 3.8e2     1.1e3 / 1.4e3     11 / 9.8    5.0 / 4.3   7.0e3 / 6.8e3     7.9 / 12    1.8e3 / 1.7e3
  rbf6    4.3e2 / 25    2.7e5 / 2.0e5     1.6e7 / 9.3e6     14 / 18     4.3 / 3.7   2.7e7 / 2.7e7     11 / 5.9    8.4e7 / 3.2e7
  rbf10   3.2e2 / 21    1.3e7 / 6.8e6     6.6e9 / 4.8e9     7.9 / 12    11 / 4.0    4.4e9 / 5.1e9     16 / 5.6    2.1e10 / 1.8e10
  nngp3   27 / 25       8.4e2 / 8.1e2     2.0e4 / 1.6e4     3.7 / 7.3   3.6 / 2.6   4.3e4 / 5.2e4     6.9 / 8.1   2.0e4 / 2.2e4
  nngp8   28 / 25       4.0e3 / 3.2e3     1.2e5 / 9.2e4     4.0 / 6.1   4.5 / 3.2   5.0e5 / 3.2e5     7.2 / 7.8   3.6e5 / 1.6e5
  scaled  4.3e2 / 25    2.7e5 / 2.0e5     1.6e7 / 9.3e6     14 / 18     5.0 / 6.2   8.5e8 / 1.1e9     11 / 5.9    8.4e7 / 3.2e7
  factor_and_solve, n in {1, 127, 130, 384}
          w_res         w_fwd             zt_fwd            ainv_fwd          alpha_fwd         nrs_fwd
  rbf2    2.2 / 1.4     1.6e3 / 2.8e3     1.4e3 / 1.4e3     9.5e2 / 9.5e2     3.6e4 / 2.2e4     9.5e2 / 8.5e2
  rbf6    1.7 / 1.1     1.0e7 / 2.4e6     8.4e7 / 1.2e7     4.3e7 / 4.9e6     6.3e7 / 2.6e7     1.8e7 / 4.3e6
  rbf10   1.4 / 1.5     6.5e7 / 2.5e7     5.1e8 / 2.2e8     2.7e8 / 1.4e8     3.4e8 / 2.1e8     2.5e8 / 1.4e8
  nngp3   1.8 / 1.3     1.4e4 / 1.2e4     1.0e4 / 2.2e4     1.1e4 / 2.0e4     7.7e4 / 7.9e4     1.1e4 / 1.9e4
  nngp8   1.7 / 1.3     2.1e5 / 6.5e4     3.6e5 / 1.3e5     2.5e5 / 1.3e5     9.8e5 / 4.9e5     2.5e5 / 1.3e5
  scaled  2.3 / 1.7     1.3e8 / 2.1e7     8.4e7 / 1.2e7     4.3e7 / 4.9e6     5.2e8 / 6.9e7     1.8e7 / 4.3e6
The constant of a quantity is 4 x the larger figure of its own row of MEASURED (never below 4): for L_bwd at rbf6, n = 384, that is
4 x 429 = 1716 u = 1.9e-13 of (|L| |L|^T)_ij; for the residuals of the solves 9 .. 66 u.  The residuals sit at a few u whatever
the conditioning; the componentwise backward error of the factor grows with it on the blocked method (the restatement's 33 ..
429 u against LAPACK's 6 .. 25 u: the panel is a product with the explicit block inverse) and the forward errors follow
cond(A) (2e4 .. 1e13) for both.  The scaled family repeats rbf6's figures wherever the scaling commutes with the rounding.
"""
import functools
import os
import sys

import numpy as np
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extended_precision as E  # noqa: E402
import gp_reference as R  # noqa: E402

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the referee needs a long double of at least 64 significant bits (x87's 80-bit format)"
U = 2.0 ** -53
NB = 128
SOLVE_W, SOLVE_INVERSE, SOLVE_ROWS = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("rbf2", "rbf6", "rbf10", "nngp3", "nngp8", "scaled")
POTRF_SIZES = (128, 256, 384, 640)
SOLVE_SIZES = (1, 127, 130, 384)


class NotPositiveDefinite(ArithmeticError):
    def __init__(self, column):
        super().__init__("the pivot of column %d is not positive" % column)
        self.column = column


# ------------------------------------------------------------------------------------------------------------- the referee
def forward_ld(l, b):
    """L^-1 b for b [n, m] in longdouble: the forward half of extended_precision.solve_ld."""
    x = b.astype(LD).copy()
    for j in range(l.shape[0]):
        x[j] = (x[j] - l[j, :j] @ x[:j]) / l[j, j]
    return x


class Referee:
    """Everything the gates need of one matrix, in 80-bit, computed on demand and once."""

    def __init__(self, a, y=None):
        self.a = np.asarray(a, dtype=np.float64)
        self.n = self.a.shape[0]
        self.y = None if y is None else np.asarray(y, dtype=np.float64)

    @functools.cached_property
    def l(self):
        return E.cholesky_ld(np.tril(self.a) + np.tril(self.a, -1).T)

    @functools.cached_property
    def zt(self):  # L^-T
        return forward_ld(self.l, np.eye(self.n)).T.copy()

    @functools.cached_property
    def ainv(self):
        return E.solve_ld(self.l, np.eye(self.n))

    @functools.cached_property
    def w(self):
        return forward_ld(self.l, self.y[:, None])[:, 0]

    @functools.cached_property
    def alpha(self):
        return E.solve_ld(self.l, self.y[:, None])[:, 0]

    def dinv(self, kb):
        s = slice(kb * NB, (kb + 1) * NB)
        return forward_ld(self.l[s, s], np.eye(NB))

    def solve_rows(self, b):  # B L^-T
        return forward_ld(self.l, b.T).T


# ---------------------------------------------------------------------------------------------------------- the restatement
def chol_block(a):
    """k_chol_diag's factor: unblocked right-looking Cholesky of one block (the lower triangle is read), zeros above."""
    s = np.tril(np.array(a, dtype=np.float64))
    nb = s.shape[0]
    for j in range(nb):
        p = s[j, j]
        if not (p > 0.0) or not np.isfinite(p):
            raise NotPositiveDefinite(j)
        ljj = np.sqrt(p)
        s[j, j] = ljj
        s[j + 1:, j] = s[j + 1:, j] / ljj
        col = s[j + 1:, j]
        s[j + 1:, j + 1:] -= np.tril(np.outer(col, col))
    return s


def block_inverse(l11):
    """k_chol_diag's inverse: forward substitution, X(i, c) = -(L(i, c) / L(c, c) + sum_{c < k < i} L(i, k) X(k, c)) / L(i, i)."""
    nb = l11.shape[0]
    dc = 1.0 / np.diag(l11)
    x = np.zeros((nb, nb))  # strictly lower part while the rows are formed
    for i in range(1, nb):
        x[i, :i] = -(l11[i, :i] * dc[:i] + l11[i, :i] @ x[:i, :i]) / l11[i, i]
    return x + np.diag(dc)


def potrf(a):
    """potrf_f64 on a copy of a [n, n], n a multiple of 128: (L with zeros above the diagonal, dinv [n / 128, 128, 128]).
    NotPositiveDefinite names the global column."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    assert n % NB == 0
    dinv = np.zeros((n // NB, NB, NB))
    for kb in range(n // NB):
        k0, k1 = kb * NB, (kb + 1) * NB
        try:
            a[k0:k1, k0:k1] = chol_block(a[k0:k1, k0:k1])
        except NotPositiveDefinite as e:
            raise NotPositiveDefinite(k0 + e.column) from None
        dinv[kb] = block_inverse(a[k0:k1, k0:k1])
        if k1 < n:
            a[k1:, k0:k1] = a[k1:, k0:k1] @ dinv[kb].T
            a[k1:, k1:] -= a[k1:, k0:k1] @ a[k1:, k0:k1].T
    return np.tril(a), dinv


def trsm_fwd(bt, l, dinv, tri=False):
    """trsm_fwd_f64 on a copy of bt [r, n]: B^T L^-T, left-looking by block columns; tri: block step kb reads and writes the
    rows < (kb + 1) 128 only (bt is the identity, or whatever the caller left below the block diagonal)."""
    bt = np.array(bt, dtype=np.float64)
    n = l.shape[0]
    for kb in range(n // NB):
        k0, k1 = kb * NB, (kb + 1) * NB
        m = k1 if tri else bt.shape[0]
        t = bt[:m, k0:k1]
        if kb > 0:
            t = t - bt[:m, :k0] @ l[k0:k1, :k0].T
        bt[:m, k0:k1] = t @ dinv[kb].T
    return bt


def pad_identity(a, n):
    np_ = -(-n // NB) * NB
    p = np.eye(np_)
    p[:n, :n] = a[:n, :n]
    return p


def factor_and_solve(a, y, mode):
    """factor_and_solve on a [n, n] and y [n], padded to Np with the identity: a dict of l, w and, by mode, zt, ainv, alpha, nrs."""
    n = a.shape[0]
    l, dinv = potrf(pad_identity(a, n))
    np_ = l.shape[0]
    wrow = np.zeros((NB, np_))
    wrow[0, :n] = y
    out = {"l": l, "w": trsm_fwd(wrow, l, dinv)[0]}
    if mode == SOLVE_W:
        return out
    zt = trsm_fwd(np.eye(np_), l, dinv, tri=True)
    out["zt"] = zt
    if mode == SOLVE_INVERSE:
        out["ainv"] = zt @ zt.T
    out["alpha"] = zt @ out["w"]
    out["nrs"] = 0.0 - np.sum(zt * zt, axis=1)
    return out


# ------------------------------------------------------------------------------------------------------------ the families
@functools.lru_cache(maxsize=None)
def _forest_rows():
    return np.load(os.path.join(GOLDEN, "forest_n1000_m200.npz"))["X_train"] / 1000.0


@functools.lru_cache(maxsize=None)
def matrix(family, n):
    """The family's n x n matrix (read-only; symmetric, both triangles filled)."""
    if family.startswith("rbf"):
        x = np.random.default_rng(1000 + n).uniform(0.0, 1.0, size=(n, 4))
        a = R.rbf(x, x, 0.7)
        a = 0.5 * (a + a.T) + 10.0 ** -int(family[3:]) * np.eye(n)
    elif family.startswith("nngp"):
        import nngp_oracle
        k = nngp_oracle.kernel_fn(_forest_rows()[:n], None, "nngp")
        k = 0.5 * (k + k.T)
        a = k + 10.0 ** -int(family[4:]) * (np.trace(k) / n) * np.eye(n)
    elif family == "scaled":
        d = scaling(n)
        a = matrix("rbf6", n) * d[:, None] * d[None, :]
    else:
        raise KeyError(family)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scaling(n):
    """The diagonal of D of the scaled family: 2^e, e uniform integers in [-100, 100]."""
    return 2.0 ** np.random.default_rng(2000 + n).integers(-100, 101, size=n).astype(np.float64)


def rhs(rows, n, seed=0):
    return np.random.default_rng(3000 + 7 * rows + n + seed).standard_normal((rows, n))


def exact(n, first_only=False, seed=0):
    """L0 = diag(2^e) + N, e integers in [-2, 2], N strictly block-lower (first_only: in the first block column alone) with
    integer entries in [-3, 3]; A = L0 L0^T.  Every intermediate of the blocked algorithm is an exact float64: the factor is L0,
    dinv the inverted diagonal, a solve of X L0^T returns X.  Returns (A, L0)."""
    rng = np.random.default_rng(4000 + n + seed)
    l0 = np.zeros((n, n))
    for rb in range(1, n // NB):
        cols = NB if first_only else rb * NB
        l0[rb * NB:(rb + 1) * NB, :cols] = rng.integers(-3, 4, size=(NB, cols))
    l0 += np.diag(2.0 ** rng.integers(-2, 3, size=n))
    return l0 @ l0.T, l0


def exact_inverse_t(l0):
    """L0^-T in closed form for N confined to the first block column: L0^-1 = D^-1 - D^-1 N D^-1."""
    di = 1.0 / np.diag(l0)
    nn = np.tril(l0, -1)
    assert not np.any(nn[:, NB:])
    return (np.diag(di) - di[:, None] * nn * di[None, :]).T


def exact_tri_with_sentinels(l0, seed=0):
    """(B, what the triangular mode must leave in its place) for B = I + S, S strictly block-lower with integer entries in
    [-3, 3], on an exact L0 whose N lies in the first block column.  The mode reads the rows of S inside its row range as part
    of B^T (for the identity they are its zeros) and writes none of them, so with N_k = L0[block k, block 0], D = diag(L0):
    block (0, k) = -D_0^-1 N_k^T D_k^-1, block (r, k) = -S_r0 N_k^T D_k^-1 for 0 < r < k, block (k, k) = (I - S_k0 N_k^T) D_k^-1,
    and S itself below.  All of it exact in float64.  A NaN there would be read too: no sentinel can be one."""
    n = l0.shape[0]
    rng = np.random.default_rng(5000 + n + seed)
    s = np.zeros((n, n))
    for rb in range(1, n // NB):
        s[rb * NB:(rb + 1) * NB, :rb * NB] = rng.integers(-3, 4, size=(NB, rb * NB))
    di = 1.0 / np.diag(l0)
    want = np.eye(n) + s
    want[:NB, :NB] = np.diag(di[:NB])
    for kb in range(1, n // NB):
        k = slice(kb * NB, (kb + 1) * NB)
        nk = l0[k, :NB]
        for rb in range(kb + 1):
            left = np.diag(di[:NB]) if rb == 0 else s[rb * NB:(rb + 1) * NB, :NB]
            want[rb * NB:(rb + 1) * NB, k] = ((np.eye(NB) if rb == kb else 0.0) - left @ nk.T) * di[k][None, :]
    return np.eye(n) + s, want


# ----------------------------------------------------------------------------------------------------------------- errors
def _worst(err, scale):
    """max err / (u scale) over the entries: only an error that IS zero counts as 0 (also over a zero scale); x / 0 is inf, and
    so is any entry whose error or scale is NaN or infinite -- a NaN in a result must miss every gate, not pass as no error."""
    err, scale = np.asarray(err, dtype=LD), np.asarray(scale, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.where(err == 0, 0.0, err / (U * scale))
    r = np.where(np.isfinite(r) & np.isfinite(err) & np.isfinite(scale), r, np.inf)
    return float(np.max(r))


def _times_upper(x, lt):
    """x @ lt in 80-bit for an upper triangular lt, by block columns (the zero half is not multiplied: NumPy's longdouble
    product is a plain loop, and these products are most of the tests' time)."""
    x, lt = np.asarray(x).astype(LD), np.asarray(lt).astype(LD)
    out = np.empty((x.shape[0], lt.shape[1]), dtype=LD)
    for j0 in range(0, lt.shape[1], NB):
        j1 = min(j0 + NB, lt.shape[1])
        out[:, j0:j1] = x[:, :j1] @ lt[:j1, j0:j1]
    return out


def _bwd(l, a):
    l = np.tril(l)
    low = np.tril(np.ones(a.shape, dtype=bool))
    return _worst(np.abs(_times_upper(l, l.T) - a)[low], (np.abs(l) @ np.abs(l).T)[low])


def _res(x, l, b):
    lt = np.tril(l).T
    return _worst(np.abs(_times_upper(x, lt) - b), np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(lt))


def _rowmax(ref):
    return np.broadcast_to(np.max(np.abs(ref), axis=1)[:, None], ref.shape)


def potrf_errors(ref, l, dinv):
    """L_bwd, L_fwd, dinv_fwd, dinv_res of a factor (l [n, n], lower triangle read; dinv [n / 128, 128, 128])."""
    n = ref.n
    low = np.tril(np.ones((n, n), dtype=bool))
    out = {"L_bwd": _bwd(l, ref.a), "L_fwd": _worst(np.abs(l - ref.l)[low], _rowmax(ref.l)[low]), "dinv_fwd": 0.0, "dinv_res": 0.0}
    for kb in range(n // NB):
        s = slice(kb * NB, (kb + 1) * NB)
        want = ref.dinv(kb)
        d, l11 = dinv[kb].astype(LD), np.tril(l[s, s]).astype(LD)
        out["dinv_fwd"] = max(out["dinv_fwd"], _worst(np.abs(d - want), _rowmax(want.T).T))
        out["dinv_res"] = max(out["dinv_res"], _worst(np.abs(d @ l11 - np.eye(NB)), np.abs(d) @ np.abs(l11)))
    return out


def solve_errors(ref, l, b, x, name):
    """<name>_res and <name>_fwd of x = b L^-T (b, x [r, n])."""
    want = ref.solve_rows(b)
    return {name + "_res": _res(x, l, b), name + "_fwd": _worst(np.abs(x - want), np.abs(b) @ np.abs(ref.zt).astype(np.float64))}


def tri_errors(ref, l, zt, name="tri"):
    z = np.triu(zt)
    return {name + "_res": _res(z, l, np.eye(ref.n)), name + "_fwd": _worst(np.abs(z - ref.zt), _rowmax(ref.zt))}


def factor_solve_errors(ref, out):
    """The errors of a factor_and_solve result cut to the n unpadded rows (keys l, w and whichever of zt, ainv, alpha, nrs)."""
    n = ref.n
    l = out["l"][:n, :n]
    low = np.tril(np.ones((n, n), dtype=bool))
    e = {"L_bwd": _bwd(l, ref.a), "L_fwd": _worst(np.abs(l - ref.l)[low], _rowmax(ref.l)[low])}
    w = out["w"][:n]
    e["w_res"] = _res(w[None, :], l, ref.y[None, :])
    e["w_fwd"] = _worst(np.abs(w - ref.w), np.abs(ref.zt).T @ np.abs(ref.y))
    if "zt" in out:
        e.update(tri_errors(ref, l, out["zt"][:n, :n], "zt"))
    if "ainv" in out:
        dg = np.sqrt(np.diag(ref.ainv))
        e["ainv_fwd"] = _worst(np.abs(out["ainv"][:n, :n] - ref.ainv), np.outer(dg, dg))
    if "alpha" in out:
        e["alpha_fwd"] = _worst(np.abs(out["alpha"][:n] - ref.alpha), np.abs(ref.zt) @ np.abs(ref.w))
    if "nrs" in out:
        e["nrs_fwd"] = _worst(np.abs(out["nrs"][:n] + np.diag(ref.ainv)), np.diag(ref.ainv))
    return e


# ------------------------------------------------------------------------------------------ LAPACK / NumPy on the same cases
def lapack_potrf(a):
    l = np.linalg.cholesky(a)
    n = a.shape[0]
    dinv = np.stack([scipy.linalg.solve_triangular(l[k:k + NB, k:k + NB], np.eye(NB), lower=True) for k in range(0, n, NB)])
    return l, dinv


def lapack_trsm(bt, l):
    return scipy.linalg.solve_triangular(l, bt.T, lower=True).T


def lapack_factor_and_solve(a, y):
    l = np.linalg.cholesky(a)
    n = a.shape[0]
    zt = scipy.linalg.solve_triangular(l, np.eye(n), lower=True).T
    ainv = scipy.linalg.cho_solve((l, True), np.eye(n))
    return {"l": l, "w": scipy.linalg.solve_triangular(l, y, lower=True), "zt": zt, "ainv": ainv,
            "alpha": scipy.linalg.cho_solve((l, True), y), "nrs": -np.diag(ainv)}


# ------------------------------------------------------------------------------------------------- the cases of the tests
@functools.lru_cache(maxsize=None)
def potrf_case(family, n):
    """(A, referee, {rows: B}) of the potrf / trsm_fwd tests."""
    a = matrix(family, n)
    return a, Referee(a), {r: rhs(r, n) for r in (128, 384)}


@functools.lru_cache(maxsize=None)
def solve_case(family, n):
    """(A, y, referee) of the factor_and_solve tests."""
    a = matrix(family, n)
    y = rhs(1, n, seed=1)[0]
    return a, y, Referee(a, y)


def measure_potrf(family, n, factor, solve):
    """The errors of (factor, solve) on potrf_case: factor(a) -> (l, dinv); solve(bt, l, dinv, tri) -> x."""
    a, ref, bs = potrf_case(family, n)
    l, dinv = factor(a)
    e = potrf_errors(ref, l, dinv)
    for r, b in bs.items():
        e.update(solve_errors(ref, l, b, solve(b, l, dinv, False), "s%d" % r))
    e.update(tri_errors(ref, l, solve(np.eye(n), l, dinv, True)))
    return e


def cpu_figures(stage, family, n):
    """(restatement's errors, LAPACK's errors) of one case, both against the referee."""
    if stage == "potrf":
        return (measure_potrf(family, n, potrf, trsm_fwd),
                measure_potrf(family, n, lapack_potrf, lambda b, l, dinv, tri: lapack_trsm(b, l)))
    a, y, ref = solve_case(family, n)
    return factor_solve_errors(ref, factor_and_solve(a, y, SOLVE_INVERSE)), factor_solve_errors(ref, lapack_factor_and_solve(a, y))


def gate(stage, family, n, key):
    """max(4 x the larger measured figure, 4), in units of u."""
    return max(4.0 * max(MEASURED[stage, family, n][key]), 4.0)


def ratios(stage, family, n, errors):
    """{key: error / gate} and the worst of them as (ratio, key)."""
    r = {k: v / gate(stage, family, n, k) for k, v in errors.items()}
    k = max(r, key=r.get)
    return r, (r[k], k)


# (stage, family, n) -> {key: (restatement, LAPACK)} in units of u, as printed by tests/test_f64_core_host.py
MEASURED = {
    ('potrf', 'rbf2', 128): {"L_bwd": (4.24, 7.6), "L_fwd": (62.3, 93.6), "dinv_fwd": (402, 531), "dinv_res": (10.8, 6.5), "s128_res": (3.04, 3.77), "s128_fwd": (613, 1.03e+03), "s384_res": (3.08, 3.47), "s384_fwd": (521, 1.1e+03), "tri_res": (2.15, 3.26), "tri_fwd": (402, 531)},
    ('potrf', 'rbf2', 256): {"L_bwd": (26.2, 13.9), "L_fwd": (298, 204), "dinv_fwd": (994, 819), "dinv_res": (4.88, 5.05), "s128_res": (2.74, 2.54), "s128_fwd": (3.09e+03, 2.4e+03), "s384_res": (3.31, 3.2), "s384_fwd": (3.32e+03, 2.66e+03), "tri_res": (4.54, 6.48), "tri_fwd": (1.36e+03, 1.01e+03)},
    ('potrf', 'rbf2', 384): {"L_bwd": (31.5, 15.4), "L_fwd": (270, 255), "dinv_fwd": (1.11e+03, 913), "dinv_res": (9.29, 9.76), "s128_res": (3.51, 3.03), "s128_fwd": (4.24e+03, 3.27e+03), "s384_res": (3.2, 3.74), "s384_fwd": (4.3e+03, 3.82e+03), "tri_res": (6.08, 7.04), "tri_fwd": (1.43e+03, 1.4e+03)},
    ('potrf', 'rbf2', 640): {"L_bwd": (33, 23.1), "L_fwd": (296, 381), "dinv_fwd": (1.11e+03, 1.39e+03), "dinv_res": (6.23, 7.89), "s128_res": (2.97, 4.87), "s128_fwd": (6e+03, 5.85e+03), "s384_res": (4.96, 4.28), "s384_fwd": (6.96e+03, 6.85e+03), "tri_res": (7.9, 11.5), "tri_fwd": (1.76e+03, 1.68e+03)},
    ('potrf', 'rbf6', 128): {"L_bwd": (3.68, 6.26), "L_fwd": (2.85e+03, 6.39e+03), "dinv_fwd": (4.55e+04, 1.2e+05), "dinv_res": (9.8, 11.5), "s128_res": (2.8, 3.08), "s128_fwd": (2.27e+04, 8.02e+04), "s384_res": (3.21, 3.06), "s384_fwd": (3.19e+04, 8.61e+04), "tri_res": (1.73, 2.82), "tri_fwd": (4.55e+04, 1.2e+05)},
    ('potrf', 'rbf6', 256): {"L_bwd": (142, 10.7), "L_fwd": (9.39e+04, 1.06e+05), "dinv_fwd": (5.49e+06, 3.75e+06), "dinv_res": (4.98, 6.95), "s128_res": (3.16, 2.85), "s128_fwd": (4.11e+06, 2.51e+06), "s384_res": (2.9, 2.92), "s384_fwd": (5.25e+06, 3.02e+06), "tri_res": (4.96, 4.81), "tri_fwd": (5.49e+06, 3.84e+06)},
    ('potrf', 'rbf6', 384): {"L_bwd": (429, 16), "L_fwd": (2.73e+05, 1.28e+05), "dinv_fwd": (1.64e+07, 6.54e+06), "dinv_res": (14, 18), "s128_res": (4.92, 3.15), "s128_fwd": (2.57e+07, 9.1e+06), "s384_res": (4.34, 3.68), "s384_fwd": (2.71e+07, 8.6e+06), "tri_res": (7.99, 4.88), "tri_fwd": (8.35e+07, 1.23e+07)},
    ('potrf', 'rbf6', 640): {"L_bwd": (81.7, 25.1), "L_fwd": (2e+05, 1.97e+05), "dinv_fwd": (8.48e+06, 9.32e+06), "dinv_res": (5.55, 8.31), "s128_res": (2.92, 2.73), "s128_fwd": (2.14e+07, 2.85e+07), "s384_res": (2.77, 2.85), "s384_fwd": (2.31e+07, 2.68e+07), "tri_res": (10.7, 5.88), "tri_fwd": (2.45e+07, 3.24e+07)},
    ('potrf', 'rbf10', 128): {"L_bwd": (4.03, 6.95), "L_fwd": (725, 3.08e+03), "dinv_fwd": (4.6e+04, 8.66e+04), "dinv_res": (7.24, 11.5), "s128_res": (3.19, 2.38), "s128_fwd": (1.84e+04, 6.16e+04), "s384_res": (3.99, 3.14), "s384_fwd": (2.47e+04, 8.73e+04), "tri_res": (2.04, 3.25), "tri_fwd": (4.6e+04, 8.66e+04)},
    ('potrf', 'rbf10', 256): {"L_bwd": (149, 12.8), "L_fwd": (1e+06, 2.4e+05), "dinv_fwd": (1.86e+07, 1.45e+07), "dinv_res": (4.49, 7.36), "s128_res": (2.92, 2.68), "s128_fwd": (1.38e+07, 1.35e+07), "s384_res": (3.95, 3.02), "s384_fwd": (1.62e+07, 1.76e+07), "tri_res": (3.92, 4.57), "tri_fwd": (2.32e+07, 2.48e+07)},
    ('potrf', 'rbf10', 384): {"L_bwd": (317, 15.9), "L_fwd": (1.82e+06, 4.43e+05), "dinv_fwd": (3.26e+08, 9.91e+07), "dinv_res": (7.9, 10.8), "s128_res": (4.34, 4.51), "s128_fwd": (1.38e+08, 7.28e+07), "s384_res": (10.7, 3.99), "s384_fwd": (1.63e+08, 7.98e+07), "tri_res": (16.4, 4.03), "tri_fwd": (5.12e+08, 2.25e+08)},
    ('potrf', 'rbf10', 640): {"L_bwd": (92.5, 21.1), "L_fwd": (1.27e+07, 6.83e+06), "dinv_fwd": (6.62e+09, 4.81e+09), "dinv_res": (5.53, 8.75), "s128_res": (2.58, 2.73), "s128_fwd": (5.76e+09, 5.37e+09), "s384_res": (3.79, 2.61), "s384_fwd": (4.39e+09, 5.07e+09), "tri_res": (5.73, 5.59), "tri_fwd": (2.08e+10, 1.79e+10)},
    ('potrf', 'nngp3', 128): {"L_bwd": (1.2, 9.77), "L_fwd": (26.9, 157), "dinv_fwd": (662, 2.44e+03), "dinv_res": (3.09, 4.07), "s128_res": (2.18, 2.05), "s128_fwd": (414, 2.76e+03), "s384_res": (3.6, 2.14), "s384_fwd": (413, 3.3e+03), "tri_res": (2.01, 2.98), "tri_fwd": (662, 2.44e+03)},
    ('potrf', 'nngp3', 256): {"L_bwd": (19.7, 16.7), "L_fwd": (714, 499), "dinv_fwd": (2.04e+04, 4.61e+03), "dinv_res": (3.69, 4.59), "s128_res": (2.2, 3.26), "s128_fwd": (2.39e+04, 1.04e+04), "s384_res": (2.44, 2.4), "s384_fwd": (2.68e+04, 1.54e+04), "tri_res": (3.89, 4.98), "tri_fwd": (2.04e+04, 5.99e+03)},
    ('potrf', 'nngp3', 384): {"L_bwd": (21.8, 18), "L_fwd": (601, 743), "dinv_fwd": (7.66e+03, 1.62e+04), "dinv_res": (3.1, 5.22), "s128_res": (2.24, 2.84), "s128_fwd": (2.48e+04, 2.57e+04), "s384_res": (3.42, 2.64), "s384_fwd": (2.79e+04, 2.42e+04), "tri_res": (6.36, 8), "tri_fwd": (1.04e+04, 2.24e+04)},
    ('potrf', 'nngp3', 640): {"L_bwd": (26.6, 25.4), "L_fwd": (841, 811), "dinv_fwd": (1.73e+04, 1.07e+04), "dinv_res": (3.25, 7.34), "s128_res": (2.67, 2.53), "s128_fwd": (3.99e+04, 4.72e+04), "s384_res": (2.98, 2.61), "s384_fwd": (4.31e+04, 5.24e+04), "tri_res": (6.89, 8.1), "tri_fwd": (1.73e+04, 1.56e+04)},
    ('potrf', 'nngp8', 128): {"L_bwd": (1.29, 8.88), "L_fwd": (36.4, 270), "dinv_fwd": (1.05e+03, 5.07e+03), "dinv_res": (3.05, 4.34), "s128_res": (2.47, 2.24), "s128_fwd": (829, 5.07e+03), "s384_res": (2.22, 2.75), "s384_fwd": (836, 5.34e+03), "tri_res": (2.05, 3.65), "tri_fwd": (1.05e+03, 5.07e+03)},
    ('potrf', 'nngp8', 256): {"L_bwd": (20.3, 14.4), "L_fwd": (4e+03, 2.76e+03), "dinv_fwd": (4.51e+04, 4.03e+04), "dinv_res": (3.09, 4.52), "s128_res": (2.18, 2.72), "s128_fwd": (1.42e+05, 1.06e+05), "s384_res": (2.62, 2.29), "s384_fwd": (1.65e+05, 1.43e+05), "tri_res": (4.31, 4.74), "tri_fwd": (7.43e+04, 5.26e+04)},
    ('potrf', 'nngp8', 384): {"L_bwd": (27.8, 18.3), "L_fwd": (2.53e+03, 2.82e+03), "dinv_fwd": (1.25e+05, 4.8e+04), "dinv_res": (3.56, 6.08), "s128_res": (2.39, 3), "s128_fwd": (6.83e+05, 2.21e+05), "s384_res": (2.75, 3.18), "s384_fwd": (4.97e+05, 2e+05), "tri_res": (5.54, 6.28), "tri_fwd": (3.62e+05, 1.28e+05)},
    ('potrf', 'nngp8', 640): {"L_bwd": (25, 25.4), "L_fwd": (2.97e+03, 3.16e+03), "dinv_fwd": (8.31e+04, 9.25e+04), "dinv_res": (4, 5.3), "s128_res": (2.77, 2.63), "s128_fwd": (2.67e+05, 3.56e+05), "s384_res": (4.52, 2.78), "s384_fwd": (3.5e+05, 3.18e+05), "tri_res": (7.17, 7.83), "tri_fwd": (1.62e+05, 1.6e+05)},
    ('potrf', 'scaled', 128): {"L_bwd": (3.68, 6.26), "L_fwd": (2.85e+03, 6.39e+03), "dinv_fwd": (4.55e+04, 1.2e+05), "dinv_res": (9.8, 11.5), "s128_res": (1.75, 3.78), "s128_fwd": (7.89e+04, 2.65e+05), "s384_res": (2.09, 6.17), "s384_fwd": (2.07e+05, 3.2e+05), "tri_res": (1.73, 2.82), "tri_fwd": (4.55e+04, 1.2e+05)},
    ('potrf', 'scaled', 256): {"L_bwd": (142, 10.7), "L_fwd": (9.39e+04, 1.06e+05), "dinv_fwd": (5.49e+06, 3.75e+06), "dinv_res": (4.98, 6.95), "s128_res": (3.44, 3.08), "s128_fwd": (5.44e+07, 4.69e+07), "s384_res": (4.7, 3.24), "s384_fwd": (9.63e+07, 7.73e+07), "tri_res": (4.96, 4.81), "tri_fwd": (5.49e+06, 3.84e+06)},
    ('potrf', 'scaled', 384): {"L_bwd": (429, 16), "L_fwd": (2.73e+05, 1.28e+05), "dinv_fwd": (1.64e+07, 6.54e+06), "dinv_res": (14, 18), "s128_res": (3.46, 4.64), "s128_fwd": (2.84e+08, 4.9e+07), "s384_res": (5, 4.35), "s384_fwd": (3.14e+08, 1e+08), "tri_res": (7.99, 4.88), "tri_fwd": (8.35e+07, 1.23e+07)},
    ('potrf', 'scaled', 640): {"L_bwd": (81.7, 25.1), "L_fwd": (2e+05, 1.97e+05), "dinv_fwd": (8.48e+06, 9.32e+06), "dinv_res": (5.55, 8.31), "s128_res": (3.76, 6.48), "s128_fwd": (8.5e+08, 1.27e+09), "s384_res": (4.82, 4.61), "s384_fwd": (8.5e+08, 1.09e+09), "tri_res": (10.7, 5.88), "tri_fwd": (2.45e+07, 3.24e+07)},
    ('solve', 'rbf2', 1): {"L_bwd": (1.46, 1.46), "L_fwd": (0.729, 0.729), "w_res": (1.32, 0.525), "w_fwd": (2.05, 0.204), "zt_res": (0.474, 0.474), "zt_fwd": (1.2, 1.2), "ainv_fwd": (2.02, 2.02), "alpha_fwd": (3.12, 3.12), "nrs_fwd": (2.02, 2.02)},
    ('solve', 'rbf2', 127): {"L_bwd": (4.84, 6.4), "L_fwd": (52.9, 99.4), "w_res": (2.24, 0.927), "w_fwd": (223, 290), "zt_res": (1.92, 4.04), "zt_fwd": (242, 512), "ainv_fwd": (183, 373), "alpha_fwd": (1.62e+03, 9.79e+03), "nrs_fwd": (170, 340)},
    ('solve', 'rbf2', 130): {"L_bwd": (13.2, 5.93), "L_fwd": (156, 90), "w_res": (1.1, 1.16), "w_fwd": (241, 394), "zt_res": (2.13, 3.53), "zt_fwd": (702, 495), "ainv_fwd": (687, 432), "alpha_fwd": (3.34e+03, 1.7e+04), "nrs_fwd": (546, 432)},
    ('solve', 'rbf2', 384): {"L_bwd": (31.5, 15.4), "L_fwd": (270, 255), "w_res": (1.79, 1.38), "w_fwd": (1.64e+03, 2.85e+03), "zt_res": (6.08, 7.04), "zt_fwd": (1.43e+03, 1.4e+03), "ainv_fwd": (949, 947), "alpha_fwd": (3.59e+04, 2.15e+04), "nrs_fwd": (952, 847)},
    ('solve', 'rbf6', 1): {"L_bwd": (1.8, 1.8), "L_fwd": (0.899, 0.899), "w_res": (0.342, 0.342), "w_fwd": (0.558, 0.558), "zt_res": (0.202, 0.202), "zt_fwd": (0.697, 0.697), "ainv_fwd": (1.19, 1.19), "alpha_fwd": (1.81, 1.81), "nrs_fwd": (1.19, 1.19)},
    ('solve', 'rbf6', 127): {"L_bwd": (3.98, 7.33), "L_fwd": (1.47e+03, 3.83e+03), "w_res": (1.67, 0.926), "w_fwd": (1.45e+03, 7.16e+03), "zt_res": (1.77, 3.27), "zt_fwd": (1.72e+04, 1e+05), "ainv_fwd": (2.63e+04, 1.5e+05), "alpha_fwd": (1.45e+04, 6.18e+04), "nrs_fwd": (2.63e+04, 1.5e+05)},
    ('solve', 'rbf6', 130): {"L_bwd": (56.5, 8.02), "L_fwd": (3.96e+03, 3.38e+03), "w_res": (1.17, 0.814), "w_fwd": (4.63e+04, 4.05e+04), "zt_res": (1.8, 5.24), "zt_fwd": (9.8e+04, 2.3e+05), "ainv_fwd": (1.47e+05, 1.35e+05), "alpha_fwd": (3.31e+05, 3.43e+05), "nrs_fwd": (1.47e+05, 1.35e+05)},
    ('solve', 'rbf6', 384): {"L_bwd": (429, 16), "L_fwd": (2.73e+05, 1.28e+05), "w_res": (1.42, 1.05), "w_fwd": (1.05e+07, 2.38e+06), "zt_res": (7.99, 4.88), "zt_fwd": (8.35e+07, 1.23e+07), "ainv_fwd": (4.34e+07, 4.86e+06), "alpha_fwd": (6.29e+07, 2.6e+07), "nrs_fwd": (1.82e+07, 4.27e+06)},
    ('solve', 'rbf10', 1): {"L_bwd": (0, 0), "L_fwd": (0, 0), "w_res": (0.179, 0.179), "w_fwd": (0.179, 0.179), "zt_res": (0, 0), "zt_fwd": (0, 0), "ainv_fwd": (0, 0), "alpha_fwd": (0.358, 0.358), "nrs_fwd": (0, 0)},
    ('solve', 'rbf10', 127): {"L_bwd": (4.21, 7.61), "L_fwd": (1.62e+03, 4.82e+03), "w_res": (1.14, 1.04), "w_fwd": (2.21e+03, 5.24e+03), "zt_res": (1.91, 3.73), "zt_fwd": (3.37e+04, 8.51e+04), "ainv_fwd": (2.83e+04, 7.9e+04), "alpha_fwd": (1.25e+05, 9.41e+04), "nrs_fwd": (2.73e+04, 7.9e+04)},
    ('solve', 'rbf10', 130): {"L_bwd": (70.3, 10.4), "L_fwd": (1.45e+03, 6.26e+03), "w_res": (1.35, 0.965), "w_fwd": (1.85e+04, 5.02e+04), "zt_res": (1.87, 2.38), "zt_fwd": (4.99e+04, 1.37e+05), "ainv_fwd": (6.35e+04, 1.75e+05), "alpha_fwd": (1.33e+05, 3.63e+05), "nrs_fwd": (6.35e+04, 1.75e+05)},
    ('solve', 'rbf10', 384): {"L_bwd": (317, 15.9), "L_fwd": (1.82e+06, 4.43e+05), "w_res": (1.4, 1.46), "w_fwd": (6.48e+07, 2.52e+07), "zt_res": (16.4, 4.03), "zt_fwd": (5.12e+08, 2.25e+08), "ainv_fwd": (2.73e+08, 1.38e+08), "alpha_fwd": (3.39e+08, 2.07e+08), "nrs_fwd": (2.49e+08, 1.38e+08)},
    ('solve', 'nngp3', 1): {"L_bwd": (1.02, 1.02), "L_fwd": (0.512, 0.512), "w_res": (0.434, 0.434), "w_fwd": (0.946, 0.946), "zt_res": (0.529, 0.529), "zt_fwd": (1.04, 1.04), "ainv_fwd": (1.7, 1.7), "alpha_fwd": (1.4, 1.4), "nrs_fwd": (1.7, 1.7)},
    ('solve', 'nngp3', 127): {"L_bwd": (1.2, 9.66), "L_fwd": (33.8, 170), "w_res": (1.07, 1.18), "w_fwd": (167, 1.8e+03), "zt_res": (1.94, 3.6), "zt_fwd": (689, 2.35e+03), "ainv_fwd": (331, 1.82e+03), "alpha_fwd": (1.48e+03, 2.23e+04), "nrs_fwd": (245, 1.39e+03)},
    ('solve', 'nngp3', 130): {"L_bwd": (11.3, 9.96), "L_fwd": (162, 173), "w_res": (1.81, 0.823), "w_fwd": (692, 1.1e+03), "zt_res": (2.34, 3.25), "zt_fwd": (2.04e+03, 2.26e+03), "ainv_fwd": (1.28e+03, 1.29e+03), "alpha_fwd": (2.52e+03, 5.47e+03), "nrs_fwd": (863, 1.29e+03)},
    ('solve', 'nngp3', 384): {"L_bwd": (21.8, 18), "L_fwd": (601, 743), "w_res": (1.18, 1.33), "w_fwd": (1.36e+04, 1.25e+04), "zt_res": (6.36, 8), "zt_fwd": (1.04e+04, 2.24e+04), "ainv_fwd": (1.14e+04, 1.96e+04), "alpha_fwd": (7.67e+04, 7.94e+04), "nrs_fwd": (1.14e+04, 1.93e+04)},
    ('solve', 'nngp8', 1): {"L_bwd": (0.663, 0.663), "L_fwd": (0.331, 0.331), "w_res": (0.413, 0.413), "w_fwd": (0.0816, 0.0816), "zt_res": (0.33, 0.33), "zt_fwd": (0.661, 0.661), "ainv_fwd": (1.68, 1.68), "alpha_fwd": (1.03, 1.03), "nrs_fwd": (1.68, 1.68)},
    ('solve', 'nngp8', 127): {"L_bwd": (1.11, 9.08), "L_fwd": (44, 343), "w_res": (1.17, 0.879), "w_fwd": (287, 1.16e+03), "zt_res": (2.11, 3.62), "zt_fwd": (943, 3.25e+03), "ainv_fwd": (785, 2.63e+03), "alpha_fwd": (2.17e+03, 9.83e+03), "nrs_fwd": (784, 2.43e+03)},
    ('solve', 'nngp8', 130): {"L_bwd": (17.7, 9.46), "L_fwd": (293, 191), "w_res": (1.73, 1.29), "w_fwd": (1.11e+03, 2.47e+03), "zt_res": (1.79, 3.5), "zt_fwd": (3.34e+03, 4.52e+03), "ainv_fwd": (3.01e+03, 3.79e+03), "alpha_fwd": (4.59e+03, 9.95e+03), "nrs_fwd": (2.08e+03, 3.79e+03)},
    ('solve', 'nngp8', 384): {"L_bwd": (27.8, 18.3), "L_fwd": (2.53e+03, 2.82e+03), "w_res": (1.39, 1.34), "w_fwd": (2.12e+05, 6.5e+04), "zt_res": (5.54, 6.28), "zt_fwd": (3.62e+05, 1.28e+05), "ainv_fwd": (2.47e+05, 1.33e+05), "alpha_fwd": (9.78e+05, 4.88e+05), "nrs_fwd": (2.47e+05, 1.33e+05)},
    ('solve', 'scaled', 1): {"L_bwd": (1.8, 1.8), "L_fwd": (0.899, 0.899), "w_res": (0.342, 0.342), "w_fwd": (0.558, 0.558), "zt_res": (0.202, 0.202), "zt_fwd": (0.697, 0.697), "ainv_fwd": (1.19, 1.19), "alpha_fwd": (1.81, 1.81), "nrs_fwd": (1.19, 1.19)},
    ('solve', 'scaled', 127): {"L_bwd": (3.98, 7.33), "L_fwd": (1.47e+03, 3.83e+03), "w_res": (1.53, 1.7), "w_fwd": (2.45e+04, 1.57e+05), "zt_res": (1.77, 3.27), "zt_fwd": (1.72e+04, 1e+05), "ainv_fwd": (2.63e+04, 1.5e+05), "alpha_fwd": (5.28e+05, 2.63e+05), "nrs_fwd": (2.63e+04, 1.5e+05)},
    ('solve', 'scaled', 130): {"L_bwd": (56.5, 8.02), "L_fwd": (3.96e+03, 3.38e+03), "w_res": (1.26, 0.875), "w_fwd": (1.06e+05, 2e+05), "zt_res": (1.8, 5.24), "zt_fwd": (9.8e+04, 2.3e+05), "ainv_fwd": (1.47e+05, 1.35e+05), "alpha_fwd": (8.31e+04, 2.74e+05), "nrs_fwd": (1.47e+05, 1.35e+05)},
    ('solve', 'scaled', 384): {"L_bwd": (429, 16), "L_fwd": (2.73e+05, 1.28e+05), "w_res": (2.32, 1.18), "w_fwd": (1.28e+08, 2.08e+07), "zt_res": (7.99, 4.88), "zt_fwd": (8.35e+07, 1.23e+07), "ainv_fwd": (4.34e+07, 4.86e+06), "alpha_fwd": (5.2e+08, 6.93e+07), "nrs_fwd": (1.82e+07, 4.27e+06)},
}
