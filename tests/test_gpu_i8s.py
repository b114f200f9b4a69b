"""The int8 digit-plane residual product (csrc/gemm_i8s.hip) through its stand-alone operators (include/nngp_i8s.h) and
nngp_gemm_nt_i8s, held to the integer referee of tests/i8s_reference.py: scales, planes, the written-back rows and out32 bit for
bit, the combined result against the exact E under the counted / measured gate, the fused row statistics against exact sums over
the device's own result, the floor ratios against their formula, every entry of every shape.  DESIGN.md 20 has the method, the
figures and the mutations each test sees.  Rows the planes cannot hold (a maximum below 2^-960; a NaN, an Inf, 1e300) are pinned
to the contract of the header: zero, or NaN throughout -- never a finite wrong value."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i8s_reference as R  # noqa: E402
import gpu_util as G  # noqa: E402
from nngp_src_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = np.int8(G.I8S_SENTINEL)
CUT_COLS = (1, 2, 127, 128, 129, 4095, 4096, 4097, 4226)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _err():
    return _lib.load().nngp_last_error()


def _cut_inputs(family, rows, cols, ns):
    return {"digit_edges": lambda: R.digit_edges(rows, cols, ns), "spread": lambda: R.spread(rows, cols),
            "integers": lambda: R.integers(rows, cols)}[family]()


def _check_cut(src, ns, scale_in=None, writeback=None):
    """One nngp_i8s_cut_rows call against the referee: scales, planes, zero fill, sentinels, source and write-back."""
    rows, cols = src.shape
    kp = -(-cols // 128) * 128
    ld, ldp = cols + 2 + (cols & 1), kp + 16
    rc, scale, planes, tail, after, wb = G.i8s_cut_rows(src, ns, ld=ld, ldp=ldp, scale_in=scale_in, writeback=writeback)
    assert rc == 0, _err()
    want_scale, xi, dig = R.cut(src, ns, scale_in)
    assert _same(scale, want_scale), (scale, want_scale)
    assert R.check_planes(np.ascontiguousarray(planes[:, :, :cols]), xi) == 0      # the digits of X, the top one read as int8
    assert _same(np.ascontiguousarray(planes[:, :, :cols]), dig)
    assert not planes[:, :, cols:kp].any()                                         # zero up to the next multiple of 128
    assert np.all(planes[:, :, kp:] == SENT) and np.all(tail == SENT)              # nothing beyond, no row too many
    rounded = R.rounded_rows(xi, want_scale, ns)
    if writeback == "inplace":
        assert _same(after[:, :cols], rounded) and np.isnan(after[:, cols:]).all()
    else:
        assert _same(after[:, :cols], src) and np.isnan(after[:, cols:]).all()     # the source is read only
        if writeback == "other":
            assert _same(wb[:, :cols], rounded) and np.isnan(wb[:, cols:]).all()
    return want_scale, dig, rounded


# ------------------------------------------------------------------------------------------------------------ 1. planes
@pytest.mark.parametrize("ns", [2, 3, 4, 5, 6, 7])
def test_planes_and_scales_are_the_referees_bit_for_bit(ns):
    """Every family, rows in {1, 3}, every column count around the 128-column padding and the 4096-column segment; odd counts;
    ld > cols with NaN behind the row, ldp > kp with a sentinel behind the planes."""
    for family in ("digit_edges", "spread", "integers"):
        for cols in CUT_COLS:
            for rows in (1, 3):
                _check_cut(_cut_inputs(family, rows, cols, ns), ns)


@pytest.mark.parametrize("ns", [2, 5, 7])
def test_planes_with_given_scales(ns):
    """scale_in: twice and 2^10 times the row's own scale (what the diagonal bound of a kernel matrix may give a small row)."""
    for cols in (129, 4097):
        src = R.digit_edges(3, cols, ns)
        own = R.row_scales(src)
        for f in (2.0, 1024.0):
            _check_cut(src, ns, scale_in=own * f)


# -------------------------------------------------------------------------------------------------------- 2. write-back
@pytest.mark.parametrize("ns", [2, 3, 4, 5, 6, 7])
def test_the_written_back_row_is_what_the_planes_hold(ns):
    for family in ("digit_edges", "spread"):
        for cols in (2, 129, 4097):
            src = _cut_inputs(family, 3, cols, ns)
            for mode in ("inplace", "other"):
                scale, dig, rounded = _check_cut(src, ns, writeback=mode)
            # "the planes are then the row itself": cutting the rounded row again gives the same row, and the same scales and planes
            # -- but for a row whose maximum sat above 126/128 of a power of two by less than half a last digit: rounded, it IS
            # 126/128, the scale halves and every X doubles (the same numbers one bit further up)
            scale2, dig2, rounded2 = _check_cut(rounded, ns, writeback="inplace")
            assert _same(rounded2, rounded)
            moved = scale2 != scale
            mx, mx2 = np.abs(src).max(axis=1), np.abs(rounded).max(axis=1)
            assert np.all(scale2[moved] == scale[moved] / 2) and np.all(mx2[moved] == scale2[moved] * (126 / 256))
            assert np.all(mx[moved] > mx2[moved]) and np.all(mx[moved] - mx2[moved] <= scale[moved] * 256.0 ** -ns / 2)
            assert _same(dig2[:, ~moved], dig[:, ~moved])
            assert np.array_equal(R.planes_value(dig2[:, moved]), 2 * R.planes_value(dig[:, moved]))
            if family == "digit_edges" and cols == 129 and ns <= 6:   # (at ns = 7 a float64 that large is an integer X already)
                assert moved.any() and not moved.all()      # (r + cols) % 4 == 2: the row one ulp above 126/128


# ------------------------------------------------------------------------------------------------- 3. kernel-matrix cut
def _check_kernel_cut(k, ns):
    n = k.shape[0]
    assert R.decision_margin(R.kernel_bounds(k)) > 1e-12
    want_scale, xi, dig = R.cut(k, ns, R.kernel_scales(k))
    got = {}
    for by_rows in (0, 1):
        rc, scale, planes, sq = G.i8s_cut_sym(k, ns, by_rows, ld=n + 2, ldp=n + 16)
        assert rc == 0, _err()
        assert _same(scale, want_scale)
        assert R.check_planes(np.ascontiguousarray(planes[:, :, :n]), xi) == 0 and _same(np.ascontiguousarray(planes[:, :, :n]), dig)
        assert np.all(planes[:, :, n:] == SENT)
        exact = sum(int(s) ** 2 for s in want_scale) if np.all(want_scale >= 1) else float(np.sum(want_scale.astype(R.LD) ** 2))
        assert abs(sq - float(exact)) <= n * R.U * float(exact)   # n exact squares of powers of two, n additions
        got[by_rows] = planes
    assert _same(got[0], got[1])
    return dig


@pytest.mark.parametrize("ns", [5, 7])
@pytest.mark.parametrize("n", [128, 384])
def test_kernel_matrix_cut_symmetric_and_by_rows(n, ns):
    """Scales from the diagonal bound; the symmetric kernel's planes (its transposed half included: negative entries, the
    duplicated and antiparallel rows, zero rows and the zero padding) are the referee's and the row kernel's."""
    for kind in ("gram", "edges"):
        k = R.kernel_matrix(kind, n)
        _check_kernel_cut(k, ns)


def test_kernel_matrix_cut_of_a_built_kernel_with_both_signs(golden_dir):
    """nngp_kernel_build on the forest fixture's first 256 rows, every second row and column negated (D K D: symmetric PSD, real
    rounded entries of both signs)."""
    x = np.load(os.path.join(golden_dir, "forest_n256_m64.npz"))["X_train"][:256]
    k = G.kernel_build(x, None, [1.0, 1.0], [0.1, 0.1], get=("nngp",))["nngp"]
    k = np.tril(k) + np.tril(k, -1).T
    d = np.where(np.arange(256) % 2 == 0, 1.0, -1.0)
    k = k * d[:, None] * d[None, :]
    assert np.array_equal(k, k.T) and (k < 0).any() and (k > 0).any()
    for ns in (5, 7):
        _check_kernel_cut(k, ns)


# ------------------------------------------------------------------------------------------------ 4. product and combine
@functools.lru_cache(maxsize=4)
def _residual_case(family, mp, n, plan):
    return R.residual_case(family, mp, n, plan)


def _residual_against_E(pc, cin, plan, coeffs, round_z=False, sym=False, inplace=False):
    alpha, beta, gamma = coeffs
    res = G.i8s_residual(pc.a, pc.b, cin if beta != 0.0 else None, alpha, beta, gamma, *plan, round_z=round_z, sym=sym, inplace=inplace,
                         ld_pad=2)
    assert res["rc"] == 0, _err()
    assert _same(res["z"], pc.a_rounded if round_z else pc.a)          # z rounded to its planes, or left alone
    g = pc.a_rounded if round_z else pc.a
    # the planes are the same either way, so with round_z the exact product IS that of the rounded z
    hi, lo, unit = pc.exact(alpha, beta, cin, gamma, g)
    w = R.worst(res["out"], hi, lo, unit)
    return w, res["out"]


@pytest.mark.parametrize("plan", R.PLANS)
def test_residual_against_the_exact_combination(plan):
    """Every family and coefficient set at 128 x 128; (4,7,7) and (7,4,7) have eight diagonals.  The symmetric cut (5 or 7 planes
    of K) gives the same bits, and so does a second call."""
    for family in R.FAMILIES:
        pc, cin = _residual_case(family, 128, 128, plan)
        g = R.gate(plan, family)
        for coeffs in R.COEFFS:
            w, out = _residual_against_E(pc, cin, plan, coeffs)
            print("plan %r %-11s alpha, beta, gamma = %r: %.3f u (gate %.3f)" % (plan, family, coeffs, w, g))
            assert w <= g, (plan, family, coeffs, w, g)
        w2, out2 = _residual_against_E(pc, cin, plan, R.COEFFS[2], sym=plan[1] in (5, 7), round_z=True)
        assert w2 <= g, (plan, family, w2, g)
        if plan[1] in (5, 7):
            _, out3 = _residual_against_E(pc, cin, plan, R.COEFFS[2], sym=False, round_z=True)
            assert _same(out2, out3)
        _, again = _residual_against_E(pc, cin, plan, R.COEFFS[2])
        assert _same(again, out)


@pytest.mark.parametrize("mp,n", [(128, 384), (384, 640), (128, 1152), (128, 2176)])
def test_residual_shapes(mp, n):
    """More than one tile, edge tiles, 2 and 3 column blocks; the model's two grades of z (rounded to 3 planes against 5 of K,
    cut 4) and the widest plans, the model's coefficients."""
    for plan, family in (((3, 5, 4), "spread"), ((7, 7, 6), "kernel"), ((4, 7, 7), "digit_edges")):
        pc, cin = R.residual_case(family, mp, n, plan)
        w, _ = _residual_against_E(pc, cin, plan, R.COEFFS[2], round_z=plan[0] == 3, sym=plan[1] == 5)
        print("(%d, %d) plan %r %s: %.3f u (gate %.3f)" % (mp, n, plan, family, w, R.gate(plan, family)))
        assert w <= R.gate(plan, family), (mp, n, plan, family, w)


def test_cin_variants_and_the_clamped_cut():
    """beta = 0 with cin = NULL; cin = out in place; a cut beyond ns_z + ns_k - 2 is the full product."""
    plan = (5, 5, 4)
    pc, cin = _residual_case("spread", 128, 128, plan)
    w, out = _residual_against_E(pc, cin, plan, (0.7, 0.0, 0.0))
    assert w <= R.gate(plan, "spread")
    w, out = _residual_against_E(pc, cin, plan, R.COEFFS[1])
    w2, out2 = _residual_against_E(pc, cin, plan, R.COEFFS[1], inplace=True)
    assert _same(out, out2)
    pc2, cin2 = _residual_case("spread", 128, 128, (2, 2, 2))
    a = G.i8s_residual(pc2.a, pc2.b, cin2, -1.0, 1.0, 0.0, 2, 2, 2)
    b = G.i8s_residual(pc2.a, pc2.b, cin2, -1.0, 1.0, 0.0, 2, 2, 9)
    assert a["rc"] == 0 and b["rc"] == 0 and _same(a["out"], b["out"])


def _gemm(pc, cin, alpha, beta, plan):
    import torch
    k = pc.a.shape[1]
    c = torch.full((pc.a.shape[0], pc.b.shape[0]), float("nan"), device=G.dev(), dtype=torch.float64)
    ld = k + 2 - (k & 1)   # even and > k, NaN behind every row
    G.gemm_nt_i8s(c, torch.from_numpy(np.ascontiguousarray(cin)).to(G.dev()) if beta != 0.0 else None, G._padded_f64(pc.a, ld)[:, :k],
                  G._padded_f64(pc.b, ld)[:, :k], alpha, beta, *plan)
    return c.cpu().numpy()


@pytest.mark.parametrize("k", [1, 127, 128, 129, 200])
def test_general_product_against_the_exact_combination(k):
    for plan in R.PLANS:
        for family in ("digit_edges", "spread"):
            pc, cin = R.gemm_case(family, 128, 128, k, plan)
            for alpha, beta, _ in R.COEFFS[:2]:
                w = R.worst(_gemm(pc, cin, alpha, beta, plan), *pc.exact(alpha, beta, cin))
                assert w <= R.gate(plan, family), (k, plan, family, alpha, beta, w)


@pytest.mark.parametrize("m,n,k,plan", [(128, 128, 16384 + 130, (5, 5, 4)), (128, 256, 40960 + 128, (3, 5, 4))])
def test_general_product_over_two_k_chunks(m, n, k, plan):
    """Two ordinary chunks (5 x 5: up to 5 pairs on a diagonal) and two long ones (3 x 5: at most 3)."""
    pc, cin = R.gemm_case("spread", m, n, k, plan)
    for alpha, beta, _ in R.COEFFS[:2]:
        w = R.worst(_gemm(pc, cin, alpha, beta, plan), *pc.exact(alpha, beta, cin))
        print("k = %d plan %r alpha, beta = %r, %r: %.3f u (gate %.3f)" % (k, plan, alpha, beta, w, R.gate(plan, "spread")))
        assert w <= R.gate(plan, "spread"), (k, plan, alpha, beta, w)


def test_integers_are_exact_on_every_route():
    """|x| < 2^23, three planes, all nine pairs: the integer result bit for bit from nngp_gemm_nt_i8s, and (K = G G^T with
    small-integer G, three planes of z against five or seven of K, every pair) from nngp_i8s_residual with sym and round_z 0 / 1."""
    for m, n, k in ((128, 128, 200), (256, 384, 129)):
        pc, cin = R.gemm_case("integers", m, n, k, (3, 3, 4))
        want = cin - pc.a @ pc.b.T
        assert np.abs(want).max() < 2.0 ** 53 and np.array_equal(pc.restated(-1.0, 1.0, cin), want)
        assert _same(_gemm(pc, cin, -1.0, 1.0, (3, 3, 4)), want)
    for mp, n in ((128, 128), (128, 384)):
        z, kmat, cin = R.product_inputs("integers", mp, n)
        want = cin - z @ kmat - 2.0 * z
        assert np.abs(want).max() < 2.0 ** 53
        for ns_k in (3, 5, 7):
            cut = 7   # at most eight diagonals; with 7 planes of K the pair (2, 6) is left out, and K's digits 3.. are zero
            pc = R.ProductCase(z, kmat, 3, ns_k, cut, sb=R.kernel_scales(kmat))
            assert np.array_equal(pc.restated(-1.0, 1.0, cin, -2.0, z), want)
            for sym in ((0, 1) if ns_k != 3 else (0,)):
                for round_z in (0, 1):
                    res = G.i8s_residual(z, kmat, cin, -1.0, 1.0, -2.0, 3, ns_k, cut, round_z=bool(round_z), sym=bool(sym))
                    assert res["rc"] == 0, _err()
                    assert _same(res["out"], want), (mp, n, ns_k, sym, round_z, np.abs(res["out"] - want).max())
                    assert _same(res["z"], z)


def test_plan_refusals_name_the_reason():
    """On real buffers: nothing is launched, the output keeps its NaN.  A diagonal of 8 pairs cannot be built with <= 7 planes."""
    pc, cin = _residual_case("spread", 128, 128, (5, 5, 4))
    for kw, text in ((dict(ns_z=7, ns_k=7, cut=7), b"too many slice pairs"), (dict(ns_z=1, ns_k=5, cut=4), b"2..7 planes"),
                     (dict(ns_z=5, ns_k=8, cut=4), b"2..7 planes"), (dict(ns_z=5, ns_k=5, cut=-1), b"cut must be >= 0"),
                     (dict(ns_z=5, ns_k=5, cut=4, ld_pad=1), b"even")):
        ld_pad = kw.pop("ld_pad", 0)
        res = G.i8s_residual(pc.a, pc.b, cin, -1.0, 1.0, 0.0, kw["ns_z"], kw["ns_k"], kw["cut"], ld_pad=ld_pad)
        assert res["rc"] < 0 and text in _err(), (kw, _err())
        assert np.isnan(res["out"]).all()
    import torch
    lib = _lib.load()
    t = torch.zeros(128 * 130 + 8, dtype=torch.float64, device=G.dev())
    p = t.data_ptr()
    assert lib.nngp_i8s_residual(p + 8, 128, p, 128, p, 128, p, 128, 128, 128, -1.0, 1.0, 0.0, 5, 5, 4, 0, 0,
                                 None, None, None, None, None, None, None, None) < 0 and b"aligned" in _err()


# --------------------------------------------------------------------------------------------------- 5. fused statistics
@pytest.mark.parametrize("n", [128, 1152, 2176])
def test_fused_statistics(n):
    """1, 2 and 3 column blocks (the last with 128 live columns): out32, var, delta, zstat and both floor ratios; the fused and
    the plain pass give the same out."""
    mp, plan = 128, (3, 5, 4)
    for family in ("spread", "kernel"):
        pc, cin = R.residual_case(family, mp, n, plan)
        alpha, beta, gamma = R.COEFFS[2]
        rest_out = pc.restated(alpha, beta, cin, gamma, pc.a_rounded)
        base = (1.5 + np.abs(np.random.default_rng(n).standard_normal(mp))) * np.sum(np.abs(pc.a_rounded) * np.abs(cin + rest_out), axis=1)
        res = G.i8s_residual(pc.a, pc.b, cin, alpha, beta, gamma, *plan, round_z=True, sym=True, base=base)
        assert res["rc"] == 0, _err()
        plain = G.i8s_residual(pc.a, pc.b, cin, alpha, beta, gamma, *plan, round_z=True, sym=True)
        out, g = res["out"], pc.a_rounded
        assert _same(out, plain["out"]) and _same(res["z"], g)
        assert R.worst(out, *pc.exact(alpha, beta, cin, gamma, g)) <= R.gate(plan, family)
        assert _same(res["out32"], out.astype(np.float32))
        # the row statistics against exact sums over the device's own out
        exact, units = R.rowstats_exact(base, g, cin, out)
        rexact, runits = R.rowstats_exact(base, g, cin, rest_out)
        rvar, rdelta, rzs = R.rowstats(base, g, cin, rest_out)
        for name, got, rgot, i in (("var", res["var"], rvar, 0), ("delta", res["delta"], rdelta, 1), ("zstat", res["zstat"][:, 0], rzs[:, 0], 2)):
            figure = R.worst(rgot, *rexact[i], runits[i])
            gate = min(float(n + 8), 4.0 * figure)
            w = R.worst(got, *exact[i], units[i])
            print("n = %d %-7s %-6s %.3f u (restatement %.3f u, gate %.3f)" % (n, family, name, w, figure, gate))
            assert w <= gate, (n, family, name, w, gate)
        assert _same(res["zstat"][:, 1], np.abs(g).max(axis=1))
        # the floor ratios: the formula in 80-bit arithmetic with the exact var of the device's out (no device var in the referee;
        # the device's own var is within its gate of it, which the tolerance below counts as n + 8 more u of var's unit)
        var_exact = exact[0][0].astype(R.LD) + exact[0][1].astype(R.LD)
        ref = R.floor_reference(g, var_exact, pc.sb, plan[0], plan[1], plan[2])
        want = float(ref.max())
        pos = var_exact > 0
        # (cols + 10) u of the formula, and var itself: the device divides by its own var, (cols + 8) u of var's unit off the exact one
        tol = (n + 10) * R.U + (n + 8) * R.U * float(np.max(units[0][pos].astype(R.LD) / var_exact[pos]))
        for name in ("floor_rows", "floor_z"):
            got = float(res[name][0])
            print("n = %d %-7s %-10s %.6e (formula %.6e, %.2f u)" % (n, family, name, got, want, abs(got - want) / (R.U * want)))
            assert np.isfinite(got) and abs(got - want) <= tol * want, (n, family, name, got, want)


# ------------------------------------------------------------------------------------- rows the planes cannot hold (header)
def test_a_row_below_the_representable_range_counts_as_zero():
    src = R.spread(4, 128)
    src[1] = 0.0
    src[1, 5], src[1, 77] = 1e-300, -3e-301
    src[3] = np.where(np.arange(128) % 2 == 0, 2.0 ** -961, 0.0)
    for ns in (2, 5, 7):
        rc, scale, planes, _, _, wb = G.i8s_cut_rows(src, ns, writeback="other")
        assert rc == 0, _err()
        want_scale, xi, dig = R.cut(src, ns)
        assert scale[1] == 1.0 and scale[3] == 1.0 and _same(scale, want_scale)
        assert not planes[:, 1].any() and not planes[:, 3].any() and _same(planes, dig)
        assert not wb[1].any() and not wb[3].any() and np.isfinite(wb).all()
    z, kmat, cin = R.product_inputs("spread", 128, 128)
    z2 = z.copy()
    z2[7] = src[1]
    z0 = z.copy()
    z0[7] = 0.0
    a = G.i8s_residual(z2, kmat, cin, -1.0, 1.0, -1e-3, 5, 5, 4, round_z=True)
    b = G.i8s_residual(z0, kmat, cin, -1.0, 1.0, -1e-3, 5, 5, 4, round_z=True)
    assert a["rc"] == 0 and b["rc"] == 0
    assert _same(a["out"], b["out"]) and _same(a["out"][7], cin[7]) and not a["z"][7].any()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e300, -1.7e308])
def test_a_row_that_is_not_finite_never_yields_a_finite_value(bad):
    """One entry: every out entry of that row of z is non-finite (for a row of the B operand: of that column), the other rows
    keep their bits, and the write-back leaves no finite number where the entry was."""
    z, kmat, cin = R.product_inputs("spread", 128, 128)
    clean = G.i8s_residual(z, kmat, cin, -1.0, 1.0, -1e-3, 5, 5, 4, round_z=True)
    z2 = z.copy()
    z2[9, 40] = bad
    res = G.i8s_residual(z2, kmat, cin, -1.0, 1.0, -1e-3, 5, 5, 4, round_z=True)
    assert clean["rc"] == 0 and res["rc"] == 0
    others = np.arange(128) != 9
    assert not np.isfinite(res["out"][9]).any() and _same(res["out"][others], clean["out"][others])
    assert not np.isfinite(res["z"][9]).any() and _same(res["z"][others], clean["z"][others])
    # the cut alone: scale NaN, write-back NaN in every column of the row, in place and into a second buffer
    for mode in ("inplace", "other"):
        rc, scale, _, _, after, wb = G.i8s_cut_rows(z2[8:11], 5, writeback=mode)
        row = (after if mode == "inplace" else wb)[1, :128]
        assert rc == 0 and np.isnan(scale[1]) and np.isnan(row).all() and np.isfinite(scale[[0, 2]]).all()
    # a row of the B operand
    pc, c0 = R.gemm_case("spread", 128, 128, 200, (5, 5, 4))
    want = _gemm(pc, c0, -1.0, 1.0, (5, 5, 4))
    b2 = pc.b.copy()
    b2[17, 199] = bad
    pc.b = b2
    got = _gemm(pc, c0, -1.0, 1.0, (5, 5, 4))
    cols = np.arange(128) != 17
    assert not np.isfinite(got[:, 17]).any() and _same(got[:, cols], want[:, cols])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e300, 1e200])
def test_a_kernel_diagonal_the_bound_cannot_hold(bad):
    """The kernel-matrix route makes no pass over K.  A diagonal entry that is not finite or reaches 1e300 becomes the largest
    diagonal: every row's bound, every scale and every entry of the product is NaN.  A finite one whose product with the largest
    diagonal overflows (1e200) gives its own row the scale NaN -- that column of the product -- and the other rows a finite
    scale from a finite bound (include/nngp_i8s.h)."""
    z, kmat, cin = R.product_inputs("spread", 128, 128)
    k2 = kmat.copy()
    k2[9, 9] = bad
    hit = np.arange(128) == 9 if bad == 1e200 else np.ones(128, dtype=bool)
    for by_rows in (0, 1):
        rc, scale, _, sq = G.i8s_cut_sym(k2, 5, by_rows)
        assert rc == 0 and np.isnan(scale[hit]).all() and np.isfinite(scale[~hit]).all() and np.isnan(sq)
    res = G.i8s_residual(z, k2, cin, -1.0, 1.0, -1e-3, 3, 5, 4, round_z=True, sym=True)
    assert res["rc"] == 0 and not np.isfinite(res["out"][:, hit]).any() and np.isfinite(res["out"][:, ~hit]).all()
    assert np.isfinite(res["z"]).all()           # z itself is finite and stays so
