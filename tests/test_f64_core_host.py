"""CPU checks behind tests/test_gpu_f64_core.py: every figure the gates of tests/f64_core_reference.py are 4 x of is measured
again (restatement and float64 LAPACK / NumPy against the 80-bit referee), printed next to its gate, and held to it; the
restatement gives the exact family's closed forms exactly, names the failed pivot, commutes with the power-of-two scaling, and
misses the gates once a last-digit error is put into it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_core_reference as F  # noqa: E402

CASES = [("potrf", f, n) for f in F.FAMILIES for n in F.POTRF_SIZES] + [("solve", f, n) for f in F.FAMILIES for n in F.SOLVE_SIZES]


@pytest.mark.parametrize("stage,family,n", CASES)
def test_restatement_and_lapack_sit_inside_their_own_gates(stage, family, n):
    rest, lap = F.cpu_figures(stage, family, n)
    assert set(rest) == set(lap) == set(F.MEASURED[stage, family, n])
    for k in rest:
        g = F.gate(stage, family, n, k)
        print("%s %s n = %d %-9s restatement %.3g u, LAPACK %.3g u (recorded %.3g, %.3g)  ->  gate %.3g u = %.2e"
              % ((stage, family, n, k, rest[k], lap[k]) + F.MEASURED[stage, family, n][k] + (g, g * F.U)))
        assert g >= 4.0 and g == max(4.0 * max(F.MEASURED[stage, family, n][k]), 4.0)
        assert rest[k] <= g and lap[k] <= g, (stage, family, n, k, rest[k], lap[k], g)


def test_the_referee_factors_its_own_matrix():
    """L* L*^T - A in 80-bit arithmetic: 2^-64 relative, three orders below anything it is asked to judge."""
    a = F.matrix("rbf10", 256)
    l = F.Referee(a).l
    assert float(np.max(np.abs(l @ l.T - a) / (np.abs(l) @ np.abs(l).T))) <= 2.0 ** -58


@pytest.mark.parametrize("first_only", [False, True])
def test_the_restatement_is_exact_on_the_exact_family(first_only):
    n = 768
    a, l0 = F.exact(n, first_only)
    assert np.max(np.abs(a)) < 2.0 ** 15
    l, dinv = F.potrf(a)
    assert np.array_equal(l, l0)
    for kb in range(n // F.NB):
        s = slice(kb * F.NB, (kb + 1) * F.NB)
        assert np.array_equal(dinv[kb], np.diag(1.0 / np.diag(l0)[s]))
    x = np.random.default_rng(5).integers(-8, 9, size=(256, n)).astype(np.float64)
    assert np.array_equal(F.trsm_fwd(x @ l0.T, l, dinv), x)
    if first_only:
        zt = F.trsm_fwd(np.eye(n), l, dinv, tri=True)
        assert np.array_equal(zt, F.exact_inverse_t(l0))
        assert np.array_equal(F.exact_inverse_t(l0).T @ l0, np.eye(n))
        # what the caller leaves below the block diagonal is read as part of B^T and never written
        b, want = F.exact_tri_with_sentinels(l0)
        got = F.trsm_fwd(b, l, dinv, tri=True)
        assert np.array_equal(got, want) and not np.array_equal(np.triu(got), zt)


@pytest.mark.parametrize("value", [-1.0, 0.0, float("nan"), float("inf")])
def test_the_restatement_names_the_failed_pivot(value):
    for col in (0, 127, 128, 255, 300, 383):
        a = 2.0 * np.eye(384)
        a[col, col] = value
        a[383, 383] = a[383, 383] if col == 383 else -3.0
        with pytest.raises(F.NotPositiveDefinite) as e:
            F.potrf(a)
        assert e.value.column == col


def test_the_restatement_commutes_with_the_power_of_two_scaling():
    n = 384
    d = F.scaling(n)
    l, dinv = F.potrf(F.matrix("rbf6", n))
    ls, dinvs = F.potrf(F.matrix("scaled", n))
    assert np.array_equal(ls, l * d[:, None])
    for kb in range(n // F.NB):
        assert np.array_equal(dinvs[kb], dinv[kb] / d[kb * F.NB:(kb + 1) * F.NB][None, :])


def test_the_operators_check_their_arguments_before_any_device_work():
    """No GPU here: an answer that names the argument came from the check, not from a failed launch."""
    from nngp_src_amd import _lib
    lib = _lib.load()
    assert lib.nngp_potrf_dinv_f64(None, 128, 128, None, None) < 0 and b"potrf_dinv_f64" in lib.nngp_last_error()
    assert lib.nngp_potrf_dinv_f64(16, 100, 100, 16, None) < 0 and b"multiple of 128" in lib.nngp_last_error()
    assert lib.nngp_trsm_fwd_f64(16, 129, 128, 16, 128, 16, 128, 0, None) < 0 and b"even" in lib.nngp_last_error()
    assert lib.nngp_trsm_fwd_f64(24, 128, 128, 16, 128, 16, 128, 0, None) < 0 and b"aligned" in lib.nngp_last_error()
    assert lib.nngp_trsm_fwd_f64(16, 256, 128, 16, 256, 16, 256, 1, None) < 0 and b"rows must equal n" in lib.nngp_last_error()
    assert lib.nngp_factor_solve_f64(16, 5, 16, 5, 0, None, None, 16, None, None, None, None) < 0 and b"mode 0" in lib.nngp_last_error()
    assert lib.nngp_factor_solve_f64(16, 5, 16, 5, 2, None, None, None, 16, None, None, None) < 0 and b"only mode 1" in lib.nngp_last_error()
    assert lib.nngp_factor_solve_f64(16, 4, 16, 5, 1, None, None, None, None, None, None, None) < 0 and b"lda >= n" in lib.nngp_last_error()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_entry_misses_every_gate_it_touches(bad):
    """One NaN or Inf in a result is an infinite error, not no error: in a solve, in the factor, in dinv, in every output of
    factor_and_solve."""
    family, n = "rbf2", 128
    a, ref, bs = F.potrf_case(family, n)
    l, dinv = F.potrf(a)
    x = F.trsm_fwd(bs[128], l, dinv)
    x[77, 5] = bad
    e = F.solve_errors(ref, l, bs[128], x, "s128")
    assert e["s128_res"] == np.inf and e["s128_fwd"] == np.inf
    assert F._worst(np.array([0.0, bad]), np.array([1.0, 1.0])) == np.inf and F._worst(np.array([0.0, 0.0]), np.array([1.0, bad])) == np.inf
    assert F._worst(np.array([0.0, 3 * F.U]), np.array([0.0, 1.0])) == 3.0 and F._worst(np.array([1e-30]), np.array([0.0])) == np.inf
    lb, db = l.copy(), dinv.copy()
    lb[100, 3], db[0, 9, 2] = bad, bad
    e = F.potrf_errors(ref, lb, db)
    assert all(v == np.inf for v in e.values()), e
    zt = F.trsm_fwd(np.eye(n), l, dinv, tri=True)
    zt[3, 100] = bad
    assert all(v == np.inf for v in F.tri_errors(ref, l, zt).values())
    a, y, ref = F.solve_case(family, 127)
    good = F.factor_and_solve(a, y, F.SOLVE_INVERSE)
    for key, at in (("w", 5), ("zt", (3, 100)), ("ainv", (7, 9)), ("alpha", 11), ("nrs", 13)):
        out = {k: v.copy() for k, v in good.items()}
        out[key][at] = bad
        e = F.factor_solve_errors(ref, out)
        hit = {"w": ("w_res", "w_fwd"), "zt": ("zt_res", "zt_fwd"), "ainv": ("ainv_fwd",), "alpha": ("alpha_fwd",), "nrs": ("nrs_fwd",)}[key]
        assert all(e[k] == np.inf for k in hit), (key, e)
        _, (worst, _) = F.ratios("solve", family, 127, e)
        assert worst == np.inf


def test_a_last_digit_error_in_the_restatement_misses_the_gates():
    """The sub-diagonal of dinv times (1 + 1e-12), 9e3 u: the factor's panels and every solve see it."""
    family, n = "rbf2", 256

    def factor(a):
        l, dinv = F.potrf(a)
        return l, dinv

    def solve(bt, l, dinv, tri):
        bad = dinv * np.where(np.tril(np.ones((F.NB, F.NB)), -1) > 0, 1.0 + 1e-12, 1.0)
        return F.trsm_fwd(bt, l, bad, tri)

    _, (worst, key) = F.ratios("potrf", family, n, F.measure_potrf(family, n, factor, solve))
    print("dinv's sub-diagonal (1 + 1e-12) in the solves: worst error / gate %.1f (%s)" % (worst, key))
    assert worst > 10.0
