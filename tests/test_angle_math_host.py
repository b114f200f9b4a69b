"""CPU checks behind tests/test_gpu_kernel_angles.py: the rotation table of the kernel build's arctangent (csrc/trig_tab.h)
against mpmath and against its generator, the coverage of the generated inputs (every table entry, every seam, every composite
interval and boundary -- asserted, so that the GPU test cannot pass by not looking), the gate of angle_reference.py held to honest
float64 code (the host restatement of the device arithmetic and the float64 oracles), and the composite table's self-check.

Composite table, port of comp_build_host on numpy.longdouble (x86-64, glibc; worst check error against the 4e-16 limit):
  ReLU layers   2        3        4        5        6        7        8        9        10       12       15
  worst         9.9e-17  1.1e-16  1.1e-16  1.0e-16  1.1e-16  2.2e-16  4.7e-16  1.4e-15  3.8e-15  2.2e-14  1.7e-13
  accepted      yes      yes      yes      yes      yes      yes      no       no       no       no       no
Depths 7 and 8 sit next to the limit, so which of them fall back to the per-layer recursion may differ with the host's libm; the
test asserts what must hold everywhere (2..4 accepted, every accepted table within the limit) and prints the rest.
"""
import math
import os
import shutil
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activation_reference as R  # noqa: E402
import angle_reference as A  # noqa: E402
import nngp_oracle as oracle  # noqa: E402

ROOT = A.ROOT


# ------------------------------------------------------------------------------------------------------ the rotation table
def _is_nearest(got, want):
    """got is a double nearest to the mpmath value want: no further from it than half the gap to its neighbour on that side."""
    if want == 0:
        return got == 0.0
    nb = math.nextafter(got, math.inf if mp.mpf(got) < want else -math.inf)
    return abs(mp.mpf(got) - want) * 2 <= abs(mp.mpf(nb) - mp.mpf(got))


def table_problems(tab):
    """Entries (i, column) of a [65, 4] table that are not the correctly rounded a_i = double(i pi / 64), cos a_i, sin a_i,
    pi - a_i (the last three of the ROUNDED a_i: the angle the rotation really turns by)."""
    bad = []
    with mp.workdps(60):
        for i in range(A.NT + 1):
            if not _is_nearest(float(tab[i, 2]), mp.mpf(i) * mp.pi / A.NT):
                bad.append((i, 2))
            a = mp.mpf(float(tab[i, 2]))
            for c, want in ((0, mp.cos(a)), (1, mp.sin(a)), (3, mp.pi - a)):
                if not _is_nearest(float(tab[i, c]), want):
                    bad.append((i, c))
    return bad


def test_trig_table_is_the_correctly_rounded_table():
    tab, lits = A.parse_trig_tab()
    assert tab.shape == (65, 4) and len(lits) == 260
    assert table_problems(tab) == []
    # the check sees a last-digit change of any literal
    rng = np.random.default_rng(0)
    for i, c in [(48, 2), (48, 3), (0, 0), (64, 3), (31, 1)] + [(int(rng.integers(1, 64)), int(rng.integers(0, 4))) for _ in range(8)]:
        for to in (math.inf, -math.inf):
            t = tab.copy()
            t[i, c] = math.nextafter(t[i, c], to)
            assert (i, c) in table_problems(t), (i, c)


def test_generator_reproduces_the_committed_table(tmp_path):
    """scripts/make_trig_table.py, run from a copy so that it writes next to the copy and not into the tree."""
    os.makedirs(tmp_path / "scripts")
    os.makedirs(tmp_path / "nngp-src_amd" / "csrc")
    shutil.copy(os.path.join(ROOT, "scripts", "make_trig_table.py"), tmp_path / "scripts" / "make_trig_table.py")
    before = open(A.TRIG_TAB_H, "rb").read()
    subprocess.check_call([sys.executable, str(tmp_path / "scripts" / "make_trig_table.py")], cwd=str(tmp_path))
    assert open(tmp_path / "nngp-src_amd" / "csrc" / "trig_tab.h", "rb").read() == before
    assert open(A.TRIG_TAB_H, "rb").read() == before


# ------------------------------------------------------------------------------------------------------------- coverage
BLOCKS = sorted({b for _, blocks, _ in A.cases().values() for b in blocks if b[1] not in ("sym", "ends")})


@pytest.mark.parametrize("family,kind", BLOCKS)
def test_inputs_reach_every_table_entry_seam_interval_and_boundary(family, kind):
    a, s = A.block_ab(family, kind)
    problems, fig = A.coverage(family, a, s)
    print(family, kind, a.shape[0], "x", s.shape[0], fig)
    assert problems == []
    assert fig["entries"] == 65 and fig["intervals"] == 16 and fig["max_residual"] <= 0.03 and fig["max_comp_u"] <= 1.0 + 1e-9


@pytest.mark.parametrize("family", ["d2", "d16"])
def test_symmetric_rows_reach_every_table_entry(family):
    ab = A.symmetric_ab(family)
    assert ab.shape[0] > 64
    _, fig = A.coverage(family, ab, ab)
    assert fig["entries"] == 65 and fig["intervals"] == 16 and fig["max_residual"] <= 0.03


def test_the_coverage_check_notices_what_is_left_out():
    a, s = A.block_ab("d2", "one")  # one anchor, direction 0: theta = phi
    assert A.coverage("d2", a, s)[0] == []
    eps = 8.0 / A.FAMILIES["d2"][1]
    phi = np.arctan2(s[:, 1], s[:, 0])
    for i in (0, 17, 48, 63):  # a seam without its points just above it, then just below it
        sm = A.seam_angles()[i]
        problems, _ = A.coverage("d2", a, s[~((phi > sm) & (phi < sm + 2 * eps))])
        assert "seam %d + 1/2 not approached from above" % i in problems, (i, problems)
        problems, _ = A.coverage("d2", a, s[~((phi < sm) & (phi > sm - 2 * eps))])
        assert "seam %d + 1/2 not approached from below" % i in problems, (i, problems)
    for i in (1, 8, 15):  # an interval boundary without its neighbourhood
        tb = math.pi - A.boundary_angles()[i - 1]
        problems, _ = A.coverage("d2", a, s[np.abs(phi - tb) > 3 * eps])
        assert any("interval boundary %d " % i in p for p in problems), (i, problems)
    # the far end of the sweep left out: the last entries and the first intervals are never selected
    problems, _ = A.coverage("d2", a, s[phi < 2.9])
    assert any("table entries never selected" in p for p in problems) and any("composite intervals never" in p for p in problems)
    # a table index shifted by one is seen by the counter ...
    assert A.coverage("d2", a, s, shift=1)[0]


# ------------------------------------------------------------------------------------------- the gate and honest float64
def oracle_values(net, x1, x2):
    if net.family == "relu":
        arch = oracle.Arch(tuple(net.w_std), tuple(net.b_std))
        k, t = oracle.kernel_fn(x1, x2, ("nngp", "ntk"), arch)
        if x2 is None:  # the oracle's diagonal is the cross-entry form; the exact one is diag_kernel
            d = x1.shape[1]
            kd, td = oracle.diag_kernel(np.sum(x1 * x1, axis=1) / d, arch)
            k[np.diag_indices_from(k)], t[np.diag_indices_from(t)] = kd, td
        return {"nngp": k, "ntk": t}
    k, t = R.kernel_fn(x1, x2, ("nngp", "ntk"), net.w_std, net.b_std, net.acts)
    return {"nngp": k, "ntk": t}


def restatement_values(net, blk, shift=0):
    """The device's per-layer path and, for a bias-free ReLU network of >= 2 layers, its composite path (None: no such path)."""
    if net.family != "relu":
        return None, None
    tab, _ = A.parse_trig_tab()
    dg = np.eye(blk.k.shape[0], dtype=bool) if blk.sym else None
    k, t, _ = A.device_relu(blk.k, blk.q1, blk.q2, net, tab, dg, shift)
    comp = None
    if net.nd >= 3 and all(b == 0.0 for b in net.b2):
        comp = A.device_composite(blk.k, blk.q1, blk.q2, net, tab, dg, shift)[0]
    return {"nngp": k, "ntk": t}, comp


@pytest.mark.parametrize("name", list(A.cases()))
def test_restatement_and_oracle_meet_the_gate(name):
    """If honest float64 code could not meet the gate, the gate would be wrong.  Prints, per block and output, the plain worst
    error over scale and the worst error / gate of the oracle (extra = 1: its unfused q q'), of the restatement of the per-layer
    path and of the composite path (extra = 0: the gate a device result is held to)."""
    net, blocks, outs = A.cases()[name]
    for family, kind in blocks:
        x1, x2, blk = A.block(family, kind, net, extras=(0.0, 1.0))
        want = oracle_values(net, x1, x2)
        rest, comp = restatement_values(net, blk)
        accepted = comp is not None and A.comp_table(net.nd - 1)[2]
        for g in outs:
            line = "%s %s %s %s:" % (name, family, kind, g)
            for who, got, extra in (("oracle", want[g], 1.0), ("per-layer", rest and rest[g], 0.0), ("composite", comp if accepted and g == "nngp" else None, 0.0)):
                if got is None:
                    continue
                err = blk.error_abs(got, g)
                ratio, at = blk.ratio(got, g, extra)
                over = float(blk.of_scale(err - blk.carry[(g, extra)], g).max())
                line += "  %s %.2e of scale, over the carried allowance %.2e, worst / gate %.3f at %s;" % (
                    who, blk.of_scale(err, g).max(), over, ratio, at)
                assert ratio <= 1.0, (name, family, kind, g, who, ratio, at)
            print(line)
        if kind not in ("sym", "ends") and net.family == "relu":
            for g in outs:  # zero rows: exactly zero without biases; duplicates and antiparallel rows are inside the gate above
                z1, z2 = blk.q1 == 0.0, blk.q2 == 0.0
                if all(b == 0.0 for b in net.b2):
                    assert np.all(rest[g][z1] == 0.0) and np.all(rest[g][:, z2] == 0.0)


def test_a_shifted_table_index_misses_the_gate():
    """... and by the gate: with entry i + 1 in place of entry i the residual (up to 0.078 rad) leaves the range the series is
    sized for, and the restated kernel misses the gate (its next term, u^11 / 11, is then 6e-14 rad)."""
    net = A.relu_net(1)
    _, _, blk = A.block("d2", "few", net, extras=(0.0, 1.0))
    rest, _ = restatement_values(net, blk, shift=1)
    rk, rt = blk.ratio(rest["nngp"], "nngp")[0], blk.ratio(rest["ntk"], "ntk")[0]
    print("shifted index: worst / gate %.1f (NNGP), %.1f (NTK)" % (rk, rt))
    assert rk > 2.0 and rt > 2.0


def test_a_changed_table_literal_misses_the_gate():
    """The mutation the GPU file is run against on a scratch copy (entry 48's angle pair moved by 1e-12), on the restatement."""
    net = A.relu_net(1)
    _, _, blk = A.block("d2", "few", net, extras=(0.0, 1.0))
    tab, _ = A.parse_trig_tab()
    tab[48, 2] += 1e-12
    tab[48, 3] -= 1e-12
    k, t, stats = A.device_relu(blk.k, blk.q1, blk.q2, net, tab)
    assert (stats[0][0] == 48).any()
    rk, rt = blk.ratio(k, "nngp")[0], blk.ratio(t, "ntk")[0]
    print("entry 48 moved by 1e-12: worst / gate %.1f (NNGP), %.1f (NTK)" % (rk, rt))
    assert rk > 10.0 and rt > 10.0


# ------------------------------------------------------------------------------------------- the composite table's check
def test_composite_table_self_check():
    accepted, refused = [], []
    for n_relu in range(2, 16):
        coef, worst, ok = A.comp_table(n_relu)
        (accepted if ok else refused).append((n_relu, worst))
        if ok:  # an accepted table meets its limit against an independent evaluation too (mpmath, other points than the check's)
            u = np.linspace(-1.0, 1.0, 41)
            for i in (0, 1, 7, 15):
                p = np.full(u.shape, coef[i, A.COMP_DEG])
                for e in range(A.COMP_DEG - 1, -1, -1):
                    p = A.fma(p, u, coef[i, e])
                for uu, pp in zip(u, p):
                    t = (2 * i + 1 + mp.mpf(float(uu))) * mp.pi / (2 * A.COMP_NI)
                    th, c = mp.pi - t, mp.mpf(0)
                    for l in range(n_relu):
                        if l > 0:
                            th = mp.acos(c)
                        c = (mp.sin(th) + (mp.pi - th) * mp.cos(th)) / mp.pi
                    assert abs(mp.mpf(float(pp)) - c) <= A.COMP_LIMIT + 1e-17, (n_relu, i, uu)
    print("accepted:", ["%d: %.2e" % a for a in accepted], "refused:", ["%d: %.2e" % r for r in refused])
    assert all(w <= A.COMP_LIMIT for _, w in accepted)
    assert {2, 3, 4} <= {n for n, _ in accepted}  # the headline path must not fall back unnoticed on the build host
