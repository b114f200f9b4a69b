"""CPU checks behind tests/test_gpu_i8s.py: the header and the binding name the same symbols, the operators refuse bad arguments
before any device work, the figures the gates of tests/i8s_reference.py are 4 x of are measured again and printed, the exact
digit-plane sum sits inside the analytic truncation bound of the header's accuracy claim, no kernel-family matrix puts its
diagonal bound near a scale decision point, and the referee checks itself (digits, rounding, a wrapped top digit)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i8s_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_name_the_same_symbols():
    from nngp_src_amd import _lib
    with open(os.path.join(ROOT, "include", "nngp_i8s.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.I8S_ABI_SYMBOLS)
    assert "GPU library only (no host build)" in text
    lib = _lib.load()
    for name in _lib.I8S_ABI_SYMBOLS:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "nngp_hip.h")) as f:
        assert "nngp_i8s_" not in f.read()  # that header's symbol set is pinned to ABI_SYMBOLS


def test_the_operators_check_their_arguments_before_any_device_work():
    """No GPU here: an answer that names the argument came from the check, not from a failed launch."""
    from nngp_src_amd import _lib
    lib = _lib.load()
    err = lib.nngp_last_error
    assert lib.nngp_i8s_cut_rows(None, 128, 1, 128, 5, None, 16, 16, 128, None, None) < 0 and b"NULL" in err()
    for ns in (1, 8):
        assert lib.nngp_i8s_cut_rows(16, 128, 1, 128, ns, None, 16, 16, 128, None, None) < 0 and b"2..7 planes" in err()
    assert lib.nngp_i8s_cut_rows(16, 129, 1, 128, 5, None, 16, 16, 128, None, None) < 0 and b"even" in err()
    assert lib.nngp_i8s_cut_rows(16, 126, 1, 128, 5, None, 16, 16, 128, None, None) < 0 and b">= cols" in err()
    assert lib.nngp_i8s_cut_rows(16, 130, 1, 129, 5, None, 16, 16, 128, None, None) < 0 and b"ldp" in err()
    assert lib.nngp_i8s_cut_rows(16, 130, 1, 129, 5, None, 16, 16, 264, None, None) < 0 and b"multiple of 16" in err()
    assert lib.nngp_i8s_cut_rows(24, 128, 1, 128, 5, None, 16, 16, 128, None, None) < 0 and b"aligned" in err()
    assert lib.nngp_i8s_cut_rows(16, 128, 1, 128, 5, None, 16, 16, 128, 8, None) < 0 and b"aligned" in err()
    assert lib.nngp_i8s_cut_sym(16, 128, 128, 6, 16, 16, 128, 0, None, None) < 0 and b"5 or 7 planes" in err()
    assert lib.nngp_i8s_cut_sym(16, 128, 100, 5, 16, 16, 128, 0, None, None) < 0 and b"multiple of 128" in err()
    assert lib.nngp_i8s_cut_sym(16, 129, 128, 5, 16, 16, 144, 0, None, None) < 0 and b"even" in err()

    def residual(ns_z=5, ns_k=5, cut=4, ld=128, out=16, sym=0, fused=(None,) * 5, floors=(None, None), mp=128):
        return lib.nngp_i8s_residual(out, ld, 16, ld, 16, ld, 16, ld, mp, 128, -1.0, 1.0, 0.0, ns_z, ns_k, cut, 0, sym, *fused, *floors, None)

    assert residual(7, 7, 7) < 0 and b"too many slice pairs" in err()
    assert residual(ns_z=1) < 0 and b"2..7 planes" in err()
    assert residual(ns_k=8) < 0 and b"2..7 planes" in err()
    assert residual(cut=-1) < 0 and b"cut must be >= 0" in err()
    assert residual(ld=129) < 0 and b"even" in err()
    assert residual(out=24) < 0 and b"aligned" in err()
    assert residual(ns_k=6, sym=1) < 0 and b"5 or 7 planes" in err()
    assert residual(mp=100) < 0 and b"multiples of 128" in err()
    assert residual(fused=(16, 16, 16, None, 16)) < 0 and b"all or none" in err()
    assert residual(floors=(16, None)) < 0 and b"need the fused outputs" in err()
    # the general product names the same plan refusals
    gemm = lambda sa, sb, cut: lib.nngp_gemm_nt_i8s(16, 128, None, 0, 16, 128, 16, 128, 128, 128, 128, 1.0, 0.0, sa, sb, cut, None)
    assert gemm(7, 7, 7) < 0 and b"too many slice pairs" in err()
    assert gemm(5, 5, -1) < 0 and b"planes per operand" in err()
    assert gemm(8, 5, 4) < 0 and b"planes per operand" in err()


@pytest.mark.parametrize("plan", R.PLANS)
def test_the_restatement_sits_inside_its_own_gate(plan):
    for family in R.FAMILIES:
        got, rec, g = R.measure(plan, family), R.MEASURED[plan][family], R.gate(plan, family)
        counted = len(R.plan_diagonals(*plan)) + 4
        print("plan %r %-11s restatement %.3f u (recorded %.3f)  counted %d u  ->  gate %.3f u" % (plan, family, got, rec, counted, g))
        assert g == min(float(counted), 4.0 * rec)
        assert got <= g and abs(got - rec) <= 1e-3 * rec + 1e-3, (plan, family, got, rec)   # the recorded figure IS this measurement


def test_eight_diagonals_and_the_clamped_cut():
    assert [len(p) for _, p in R.plan_diagonals(4, 7, 7)] == [3, 4, 4, 4, 4, 3, 2, 1] and sum(len(p) for _, p in R.plan_diagonals(4, 7, 7)) == 25
    assert sum(len(p) for _, p in R.plan_diagonals(7, 7, 7)) == 34   # more than 32 pairs: refused
    assert R.plan_diagonals(2, 2, 9) == R.plan_diagonals(2, 2, 2)
    assert max(len(p) for _, p in R.plan_diagonals(7, 7, 6)) == 7    # a diagonal holds at most min(nsa, nsb) <= 7 pairs


@pytest.mark.parametrize("plan", R.PLANS)
def test_the_exact_plane_sum_is_inside_the_analytic_truncation_bound(plan):
    """digit rounding k (h_a max|b| + h_b max|a| + h_a h_b) + the dropped pairs: a worst-case bound (random rows sit at a few per cent)."""
    pc, _ = R.gemm_case("spread", *R.MEASURE_GEMM_SHAPE, plan)
    hi, lo, _ = pc.exact(1.0, 0.0, None)
    err = np.abs((hi.astype(R.LD) + lo.astype(R.LD)) - pc.true_product())
    bound = R.truncation_bound(pc.a, pc.b, pc.sa, pc.sb, *plan)
    ratio = float(np.max(err / bound))
    print("plan %r: exact digit-plane sum against the 80-bit product: %.3f of the bound" % (plan, ratio))
    assert ratio <= 1.0 + 1e-6   # 80-bit product of k = 200 terms: 2^-64 k relative, far below the bound
    assert ratio > 1e-4


@pytest.mark.parametrize("n", [128, 384])
def test_no_kernel_family_bound_is_near_a_scale_decision_point(n):
    for kind in ("gram", "edges", "psd_small"):
        k = R.kernel_matrix(kind, n)
        margin = R.decision_margin(R.kernel_bounds(k))
        print("%s n = %d: the diagonal bound stays %.2e (relative) away from f = 126/128" % (kind, n, margin))
        assert margin > 1e-12
        assert np.array_equal(k, k.T) and np.linalg.eigvalsh(k).min() > -1e-6 * np.abs(k).max()
    k = R.kernel_matrix("edges", n)
    b = R.kernel_bounds(k)
    assert k[3, 3] == np.diag(k).max() and k[3, 7] == k[3, 3] and k[3, 11] == -k[3, 3] and k[5, 5] == 0 and not k[5].any()
    assert abs(float(b[3]) / k[3, 7] - 1.0) < 2e-9 and (k < 0).any() and (k > 0).any()
    assert not k[-20:].any() and not k[:, -20:].any()   # padding


@pytest.mark.parametrize("ns", [2, 3, 4, 5, 6, 7])
def test_the_referee_checks_itself(ns):
    x = R.digit_edges(4, 256, ns)
    scale, xi, dig = R.cut(x, ns)
    assert dig.dtype == np.int8 and np.all(dig[1:].astype(int) >= -128) and np.all(dig[1:].astype(int) <= 127)
    assert R.check_planes(dig, xi) == 0                                       # the digits reconstruct X
    back = R.rounded_rows(xi, scale, ns)
    assert np.all(np.abs(back - x) <= scale[:, None] * 256.0 ** -ns / 2)      # X reconstructs the row within half a last digit
    assert np.all(np.abs(x).max(axis=1) / scale <= 126 / 256) and np.all(np.abs(x).max(axis=1) / (scale / 2) > 126 / 256)
    xs, ties = R.edge_values(ns)
    want = {0.5: 0, 1.5: 2, 2.5: 2, -0.5: 0, -1.5: -2, 127.5: 128, 128.5: 128, -128.5: -128}
    r0 = np.ldexp(x[0], 8 * ns)                                               # row 0 has the scale 1
    assert scale[0] == 1.0
    for t, w in want.items():
        assert np.all(xi[0][r0 == t] == w)
    # a wrapped top digit is rejected: 127 + 1 stored as int8 is -128, 256^ns off
    bad = dig.copy()
    xi2 = xi.copy()
    xi2[0, 0] = 128 * 256 ** (ns - 1)
    bad[:, 0, 0] = R.digits(xi2, ns)[:, 0, 0].astype(np.int8)
    assert bad[0, 0, 0] == -128 and R.check_planes(bad, xi2) == 1
    # and so is a lower digit one off with the difference pushed into its neighbour's range
    bad = dig.copy()
    bad[ns - 1, 1, 5] = np.int8((int(bad[ns - 1, 1, 5]) + 1 + 128) % 256 - 128)
    assert R.check_planes(bad, xi) == 1


def test_rows_the_planes_cannot_hold():
    assert R.scale_of(0.0) == 1.0 and R.scale_of(1e-300) == 1.0 and R.scale_of(2.0 ** -960) == 2.0 ** -958
    for v in (1e300, float("inf"), float("nan")):
        assert np.isnan(R.scale_of(v))
    x = np.array([[1.0, float("nan")], [1.0, 2.0], [0.0, -float("inf")]])
    s = R.row_scales(x)
    assert np.isnan(s[0]) and s[1] == 8.0 and np.isnan(s[2])


def test_a_non_finite_entry_is_an_infinite_error():
    one = np.ones((2, 2))
    for bad in (float("nan"), float("inf")):
        got = one.copy()
        got[1, 0] = bad
        assert R.worst(got, one, 0 * one, one) == np.inf
    assert R.worst(one + 3 * R.U, one, 0 * one, one) == pytest.approx(3.0, rel=0.4)
    assert R.worst(one, one, 0 * one, 0 * one) == 0.0 and R.worst(one + 1e-9, one, 0 * one, 0 * one) == np.inf


def test_the_integer_family_is_exact_in_the_restatement():
    """3 x 3 planes, all nine pairs: the combination of integer operands is the integer result, on the shapes the GPU test uses."""
    for mp, n in ((128, 128), (128, 384)):
        pc, cin = R.residual_case("integers", mp, n, (3, 3, 4))
        for alpha, beta, gamma in ((-1.0, 1.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 1.0, -2.0)):
            want = beta * cin + alpha * (pc.a @ pc.b.T) + gamma * pc.a
            assert np.abs(want).max() < 2.0 ** 53
            assert np.array_equal(pc.restated(alpha, beta, cin, gamma, pc.a_rounded), want)
            hi, lo, _ = pc.exact(alpha, beta, cin, gamma, pc.a_rounded)
            assert np.array_equal(hi, want) and not lo.any()
        assert np.array_equal(pc.a_rounded, pc.a)
    pc, cin = R.gemm_case("integers", 128, 128, 200, (3, 3, 4))
    assert np.array_equal(pc.restated(-1.0, 1.0, cin), cin - pc.a @ pc.b.T)


def test_a_last_digit_error_in_the_restatement_misses_the_gate():
    """The Horner factor times (1 + 2^-30): every plan with more than one diagonal sees it."""
    for plan in ((5, 5, 4), (7, 7, 6), (2, 2, 2)):
        pc, cin = R.residual_case("spread", 128, 128, plan)
        t = np.zeros(pc.sums[pc.diags[0][0]].shape)
        for e, _ in pc.diags:
            t = t * (0.00390625 * (1 + 2.0 ** -30)) + pc.sums[e].astype(np.float64)
        v = ((-1.0 * pc.sa) * (1.0 / 65536.0))[:, None] * pc.sb[None, :] * t + cin
        w = R.worst(v, *pc.exact(-1.0, 1.0, cin))
        print("plan %r: Horner factor (1 + 2^-30): %.1f u against the gate %.2f u" % (plan, w, R.gate(plan, "spread")))
        assert w > R.gate(plan, "spread")
