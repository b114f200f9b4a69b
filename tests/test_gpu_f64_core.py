"""The float64 Cholesky core (csrc/gp_f64.hip) entry by entry on the MI355X (-m gpu): k_chol_diag and potrf_f64 through
nngp_potrf_dinv_f64, trsm_fwd_f64 (both modes) through nngp_trsm_fwd_f64, factor_and_solve (all three modes) and k_rowdot through
nngp_factor_solve_f64 -- the factor, every inverted diagonal block, the solves, L^-T, A^-1, alpha and -diag(A^-1) held to the
per-entry gates of tests/f64_core_reference.py (80-bit referee; each gate is 4 x what the CPU restatement and LAPACK give on the
same matrix, no device result took part), then what no gate can see: the exact family (every intermediate an exact float64, so
the device must give the closed forms by value, at 768 rows and at 2304, where the solve's product takes the split-K path), the
power-of-two scaling (no absolute threshold anywhere), the untouched strict upper triangle, the row range of the triangular mode,
and the failed pivot named for every kind and place of pivot.

Worst device error / gate on the MI355X (this file's printout): factor, blocks and solves 0.35 (rbf2), 0.38 (rbf6), 0.38 (rbf10),
0.40 (nngp3), 0.63 (nngp8, n = 256: tri_fwd), 0.41 (scaled); ld = n + 6 gave the bits of ld = n in all 24 cases; factor_and_solve
0.31 (rbf2), 0.48 (rbf6), 0.44 (rbf10), 0.55 (nngp3), 0.34 (nngp8), 0.46 (scaled) -- the device sits where the CPU restatement of
its method sits (0.25 of its own gate by construction).  DESIGN.md section 19 has the CPU-measured constants, the value-only
mutations of the device code with the tests that see each, and the cost.

The triangular mode and NaN: block step kb of trsm_fwd_f64 reads rows < (kb + 1) 128 of ALL earlier block columns, so the rows of
an earlier block column that it never writes (below the block diagonal) are operands of later steps -- for the identity they are
its zeros.  A NaN prefilled there would spread into the diagonal blocks of the result on a correct library.  The row range is
therefore pinned in the exact family with integer sentinels instead: they must come back bit for bit, and the block-upper part
must be the closed form that reading them implies (f64_core_reference.exact_tri_with_sentinels) -- one row too many overwrites a
sentinel, one too few leaves part of the closed form out.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_core_reference as F  # noqa: E402
import gpu_util as G  # noqa: E402
from nngp_src_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
NB = F.NB


def _factor(a, ld=None):
    rc, out, dinv = G.potrf_dinv_f64(a, ld)
    assert rc == 0, _lib.load().nngp_last_error()
    return out, dinv


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _strictly_lower_blocks(n):
    """True below the 128 x 128 diagonal blocks."""
    b = np.arange(n) // NB
    return b[:, None] > b[None, :]


# ------------------------------------------------------------------------------------------------ potrf_f64 and trsm_fwd_f64
@pytest.mark.parametrize("n", F.POTRF_SIZES)
@pytest.mark.parametrize("family", F.FAMILIES)
def test_factor_blocks_and_solves_meet_the_gates(family, n):
    """ld = n and ld = n + 6 (the factor, the right-hand sides and the identity alike).  The second run is measured again only
    where it differs from the first in any bit."""
    a = F.matrix(family, n)
    kept = {}

    def run(ld):
        got = {}

        def factor(a_):
            got["l"], got["dinv"] = _factor(a_, ld)
            return got["l"], got["dinv"]

        def solve(bt, l, dinv, tri):
            x = G.trsm_fwd_f64(bt, l, dinv, tri, ldb=ld, ldl=ld)
            assert x.shape == bt.shape and np.all(np.isfinite(x)), ("tri" if tri else bt.shape[0])
            got["tri" if tri else "s%d" % bt.shape[0]] = x
            return x

        return got, factor, solve

    for ld in (n, n + 6):
        got, factor, solve = run(ld)
        if kept:
            factor(a)
            _, _, bs = F.potrf_case(family, n)
            for r, b in bs.items():
                solve(b, got["l"], got["dinv"], False)
            solve(np.eye(n), got["l"], got["dinv"], True)
            if all(_same(np.tril(got[k]) if k == "l" else got[k], np.tril(kept[k]) if k == "l" else kept[k]) for k in kept):
                print("%s n = %d ld = %d: the same bits as ld = %d" % (family, n, ld, n))
                continue
        errors = F.measure_potrf(family, n, factor, solve)
        kept = kept or got
        # what the gates do not say: dinv is exactly zero above the diagonal, the diagonal blocks of L likewise, and the
        # triangular mode leaves the identity's zeros below the block diagonal and exact zeros inside the diagonal blocks
        assert np.all(np.isfinite(np.tril(got["l"]))) and np.all(np.isfinite(got["dinv"]))
        assert not np.any(np.triu(got["dinv"], 1)) and got["dinv"].shape == (n // NB, NB, NB)
        for kb in range(n // NB):
            s = slice(kb * NB, (kb + 1) * NB)
            assert not np.any(np.triu(got["l"][s, s], 1))
        assert np.all(np.isfinite(got["tri"])) and not np.any(np.tril(got["tri"], -1))
        r, (worst, key) = F.ratios("potrf", family, n, errors)
        print("%s n = %d ld = %d: worst error / gate %.3f (%s: %.3g u, gate %.3g u);  %s"
              % (family, n, ld, worst, key, errors[key], F.gate("potrf", family, n, key), "  ".join("%s %.2f" % kv for kv in r.items())))
        assert worst <= 1.0, (family, n, ld, r)


# ---------------------------------------------------------------------------------------------------------- factor_and_solve
@pytest.mark.parametrize("n", F.SOLVE_SIZES)
@pytest.mark.parametrize("family", F.FAMILIES)
def test_factor_and_solve_meets_the_gates_in_every_mode(family, n):
    a, y, ref = F.solve_case(family, n)
    np_ = -(-n // NB) * NB
    full = G.factor_solve_f64(a, y, F.SOLVE_INVERSE)
    rows = G.factor_solve_f64(a, y, F.SOLVE_ROWS, lda=n + 3)
    only_w = G.factor_solve_f64(a, y, F.SOLVE_W)
    assert set(full) == {"l", "w", "zt", "ainv", "alpha", "nrs"} and set(rows) == set(full) - {"ainv"} and set(only_w) == {"l", "w"}
    worst_of = {}
    for name, out in (("inverse", full), ("rows", rows), ("w", only_w)):
        assert all(np.all(np.isfinite(np.tril(v) if k == "l" else (np.triu(v) if k == "zt" else v))) for k, v in out.items())
        # the padding: the identity in L, zeros in w and alpha
        low = np.tril(out["l"])
        assert not np.any(low[n:, :n]) and np.array_equal(low[n:, n:], np.eye(np_ - n)) and not np.any(out["w"][n:])
        if "alpha" in out:
            assert not np.any(out["alpha"][n:])
        errors = F.factor_solve_errors(ref, out)
        r, (worst, key) = F.ratios("solve", family, n, errors)
        worst_of[name] = worst
        print("%s n = %d mode %s: worst error / gate %.3f (%s: %.3g u, gate %.3g u);  %s"
              % (family, n, name, worst, key, errors[key], F.gate("solve", family, n, key), "  ".join("%s %.2f" % kv for kv in r.items())))
    assert max(worst_of.values()) <= 1.0, (family, n, worst_of)
    # -diag(A^-1) from the pass that forms alpha against the A^-1 product of the same run.  Against the referee both carry the
    # forward error of L^-T (nrs_fwd above, which follows cond(A)); against each other they are two float64 sums of the same Np
    # non-negative squares of the same L^-T, each within gamma_(Np + 1) of the exact sum whatever its order: 2 (Np + 2) u.
    d = np.diag(full["ainv"])[:n]
    own = float(np.max(np.abs(full["nrs"][:n] + d) / (F.U * np.abs(d)))) / (2.0 * (np_ + 2))
    print("%s n = %d: neg_rowsq against -diag of the device's A^-1: %.3f of 2 (Np + 2) u" % (family, n, own))
    assert own <= 1.0 and np.array_equal(rows["nrs"], full["nrs"])
    # the header's promises: alpha has the same bits in both gradient modes, with or without neg_rowsq; a second run repeats
    assert _same(full["alpha"], rows["alpha"])
    for mode, out in ((F.SOLVE_INVERSE, full), (F.SOLVE_ROWS, rows)):
        assert _same(G.factor_solve_f64(a, y, mode, want=("alpha",))["alpha"], out["alpha"])
    again = G.factor_solve_f64(a, y, F.SOLVE_INVERSE)
    for k in full:
        assert _same(np.tril(again[k]), np.tril(full[k])) if k == "l" else _same(again[k], full[k]), k


# --------------------------------------------------------------------------------------------------------------- metamorphic
@pytest.mark.parametrize("n", [384, 640])
def test_power_of_two_scaling_gives_the_scaled_factor_exactly(n):
    """D A D with D = diag(2^e), e in [-100, 100]: nothing under- or overflows, so every rounding commutes with the scaling and
    the factor is D L, dinv is dinv D^-1 -- by value.  An absolute threshold anywhere would break it."""
    d = F.scaling(n)
    l, dinv = _factor(F.matrix("rbf6", n))
    ls, dinvs = _factor(F.matrix("scaled", n))
    assert np.array_equal(np.tril(ls), np.tril(l) * d[:, None])
    for kb in range(n // NB):
        assert np.array_equal(dinvs[kb], dinv[kb] / d[kb * NB:(kb + 1) * NB][None, :])
    b = F.rhs(128, n)
    # (B D) (D L)^-T = B L^-T, and every partial sum of block column k is the unscaled one times D_k until dinv D_k^-1 takes it off
    assert np.array_equal(G.trsm_fwd_f64(b * d[None, :], ls, dinvs), G.trsm_fwd_f64(b, l, dinv))
    assert np.array_equal(G.trsm_fwd_f64(np.diag(d), ls, dinvs, tri=True), G.trsm_fwd_f64(np.eye(n), l, dinv, tri=True))


@pytest.mark.parametrize("family,n", [("rbf6", 384), ("nngp8", 640)])
def test_the_strict_upper_triangle_is_never_read(family, n):
    a = np.array(F.matrix(family, n))
    l, dinv = _factor(a, n + 6)
    a[np.triu(np.ones((n, n), dtype=bool), 1)] = np.nan
    ln, dinvn = _factor(a, n + 6)
    assert _same(np.tril(ln), np.tril(l)) and _same(dinvn, dinv)


# ------------------------------------------------------------------------------------------- exact results at many blocks
@pytest.mark.parametrize("n", [768, 2304])
@pytest.mark.parametrize("first_only", [False, True])
def test_exact_family_gives_the_closed_forms_by_value(n, first_only):
    """By value, not by bytes: -0 appears in dinv.  At n = 2304 the product of the last two block steps of trsm_fwd_f64 has
    k = 2048 and 2176 and one or two row tiles: the split-K path of the float64 GEMM, which nothing smaller takes."""
    a, l0 = F.exact(n, first_only)
    l, dinv = _factor(a)
    assert np.array_equal(np.tril(l), l0)
    di = 1.0 / np.diag(l0)
    for kb in range(n // NB):
        assert np.array_equal(dinv[kb], np.diag(di[kb * NB:(kb + 1) * NB]))
    for rows in (128, 256):
        x = np.random.default_rng(rows).integers(-8, 9, size=(rows, n)).astype(np.float64)
        assert np.array_equal(G.trsm_fwd_f64(x @ l0.T, l, dinv), x), rows
    if first_only:
        zt = G.trsm_fwd_f64(np.eye(n), l, dinv, tri=True)
        assert np.array_equal(zt, F.exact_inverse_t(l0))
        # the row range of the triangular mode: what lies below the block diagonal is read as part of B^T (a NaN there would
        # spread; for the identity it is zero) and must come back as it was, and nothing short of the range may be left out
        b, want = F.exact_tri_with_sentinels(l0)
        got = G.trsm_fwd_f64(b, l, dinv, tri=True, ldb=n + 6)
        below = _strictly_lower_blocks(n)
        assert _same(got[below], b[below])
        assert np.array_equal(got, want)


# --------------------------------------------------------------------------------------------------------- failure reporting
def _named(lib, col):
    return (b"the pivot of column %d is not positive" % col) in lib.nngp_last_error()


@pytest.mark.parametrize("value", [-1.0, 0.0, float("nan"), float("inf")])
def test_a_failed_pivot_is_named_wherever_it_is(value):
    """Error codes the library returns on purpose (k_chol_diag stops at the pivot and every later block returns at once)."""
    lib = _lib.load()
    good = F.matrix("rbf2", 384)
    l0, dinv0 = _factor(good)
    for col in (0, 127, 128, 255, 300, 383):
        a = 2.0 * np.eye(384)
        a[col, col] = value
        rc, _, _ = G.potrf_dinv_f64(a)
        assert rc < 0 and _named(lib, col), (col, lib.nngp_last_error())
        for second in (c for c in (128, 300, 383) if c > col):  # two bad pivots: the first is named
            a2 = a.copy()
            a2[second, second] = -1.0
            rc, _, _ = G.potrf_dinv_f64(a2, 390)
            assert rc < 0 and _named(lib, col), (col, second, lib.nngp_last_error())
        ad = _lib.to_device_f64(a, G.dev())
        assert lib.nngp_potrf_f64(_lib.ptr(ad), 384, 384, _lib.stream_ptr()) < 0 and _named(lib, col)
        out = G.factor_solve_f64  # the same report through the evaluation sequence
        with pytest.raises(_lib.NngpError, match="the pivot of column %d is not positive" % col):
            out(a, np.ones(384), F.SOLVE_W)
        l1, dinv1 = _factor(good)  # and the next call is as before
        assert _same(np.tril(l1), np.tril(l0)) and _same(dinv1, dinv0)


def test_arguments_are_rejected_before_any_launch():
    import torch
    lib = _lib.load()
    n = 256
    buf = torch.zeros(n * (n + 8) + 2, dtype=torch.float64, device=G.dev())
    l = torch.eye(n, dtype=torch.float64, device=G.dev())
    dinv = torch.eye(NB, dtype=torch.float64, device=G.dev()).repeat(n // NB, 1)
    p, s = buf.data_ptr(), _lib.stream_ptr()
    bad = [
        ((p, n + 1, n, l.data_ptr(), n, dinv.data_ptr(), n, 0, s), b"even"),              # odd ldb
        ((p, n, n, l.data_ptr(), n + 1, dinv.data_ptr(), n, 0, s), b"even"),              # odd ldl
        ((p + 8, n + 2, n, l.data_ptr(), n, dinv.data_ptr(), n, 0, s), b"aligned"),       # bt off a 16-byte boundary
        ((p, n, n, l.data_ptr(), n, dinv.data_ptr() + 8, n, 0, s), b"aligned"),
        ((p, n - 2, n, l.data_ptr(), n, dinv.data_ptr(), n, 0, s), b">= n"),
        ((p, n, 100, l.data_ptr(), n, dinv.data_ptr(), n, 0, s), b"multiples of 128"),
        ((p, n, 128, l.data_ptr(), n, dinv.data_ptr(), n, 1, s), b"rows must equal n"),
        ((None, n, n, l.data_ptr(), n, dinv.data_ptr(), n, 0, s), b"NULL"),
    ]
    for args, word in bad:
        assert lib.nngp_trsm_fwd_f64(*args) < 0 and word in lib.nngp_last_error(), (args, lib.nngp_last_error())
    assert not torch.any(buf).item()
    assert lib.nngp_potrf_dinv_f64(p, 100, 100, dinv.data_ptr(), s) < 0 and b"multiple of 128" in lib.nngp_last_error()
    y = torch.ones(n, dtype=torch.float64, device=G.dev())
    for mode, outs, word in ((0, (0, 0, p, 0, 0, 0), b"mode 0"), (0, (0, 0, 0, 0, p, 0), b"mode 0"), (0, (0, 0, 0, 0, 0, p), b"mode 0"),
                             (2, (0, 0, 0, p, 0, 0), b"only mode 1"), (0, (0, 0, 0, p, 0, 0), b"only mode 1"), (3, (0,) * 6, b"unknown mode")):
        assert lib.nngp_factor_solve_f64(l.data_ptr(), n, y.data_ptr(), n, mode, *outs, s) < 0 and word in lib.nngp_last_error()
    assert lib.nngp_factor_solve_f64(l.data_ptr(), n, y.data_ptr(), 0, 0, *(0,) * 6, s) < 0
    assert not torch.any(buf).item()
