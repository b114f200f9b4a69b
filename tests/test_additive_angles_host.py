"""CPU checks behind tests/test_gpu_additive_angles.py: the gate of tests/additive_angle_reference.py held to honest float64 code
(the float64 reference additive_reference.kernel_fn at extra = 1, the NumPy restatement of k_build_add at extra = 0) on every block
the GPU file uses, the coverage of the generated inputs asserted (so that the GPU test cannot pass by not looking), and the
entries the older gate of tests/test_gpu_additive.py left at 1e-6 shown to be held tightly now.  No device takes part.

Measured (this file's printout; worst error / gate over every block of a network, float64 reference | restatement):
  relu1 NNGP 0.26 | 0.29, NTK 0.87 | 0.90 (the symmetric block, nearly parallel width-16 slices: the rounding of k k, as in the plain
  angle tests); relu2_bias 0.26 | 0.22, 0.37 | 0.30; relu3_ntk 0.15 | 0.23, 0.74 | 0.24; leaky 0.37 | 0.35, 0.52 | 0.37; abs 0.48 | 0.48,
  0.46 | 0.47; erf 0.30 | 0.37, 0.16 | 0.67; erf_abc 0.57 | 0.38, 0.41 | 0.30; comp3 (whole-input term by the composite map) 0.23 | 0.23.
  The widths that are no power of two (3, 7, 9, 17, 40: the tables chunks, whole, whole_full, w37) stay below 0.41 | 0.36 with
  entry()'s initial count of 2 and nothing else.
The composed gate of the issue (C1 scale + carry per term, the sum term) held everywhere but for Theta of an Erf term on identical
slices: there the restatement exceeded it by up to 1.891e-15 of that term's scale (the float64 reference stayed inside, -2.4e-16), so
additive_angle_reference.CD = 4 x 1.891e-15 was added for those entries alone, as A.CONSTANTS were set; see its docstring.
The entries the older gate leaves at 1e-6 max |want|: 1791 of the 2151 of the width-1 block (new gate there <= 7.8e-16 of
max |want|), 10 of the width-2 block (8.9e-16), 1794 with the three groups together (2.1e-15).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import additive_angle_reference as AA  # noqa: E402
import additive_reference as R  # noqa: E402
import angle_reference as A  # noqa: E402

GOLDEN = os.path.join(A.ROOT, "tests", "golden")
# (network, table, block kind): every block of the GPU file, and the negative weight the C ABI refuses
BLOCKS = [(n, t, k) for n, (_, t, _) in AA.NETS.items() for k in ("few", "sym")]
BLOCKS += [(n, t, "few") for n in ("relu1", "erf_abc") for t in AA.DEVICE_TABLES + ["neg_w"] if (n, t, "few") not in BLOCKS]
BLOCKS += [(n, t, "few") for n in ("relu1", "relu2_bias", "leaky", "erf_abc") for t in ("pair", "g16")]
BLOCKS += [("relu1", "w1", "few"), ("relu1", "base", "big"), ("relu1", "w1", "big"), ("erf_abc", "w1", "big")]


def reference_values(net, table, x1, x2, outs):
    groups, weights, w0 = table
    acts = None if net.family == "relu" else net.acts
    return {g: R.kernel_fn(x1, x2, g, net.w_std, net.b_std, acts, groups, weights, w0, exact_same=True) for g in outs}


def restatement_values(net, table, x1, x2, kind, outs):
    composite = outs == ("nngp",) and A.comp_table(net.nd - 1)[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return AA.device_additive(x1, x2, net, table, sym=kind == "sym", composite=composite)


@pytest.mark.parametrize("name,table,kind", BLOCKS)
def test_reference_and_restatement_meet_the_gate(name, table, kind):
    """If honest float64 code could not meet the gate, the gate would be wrong.  Prints worst error / gate, where, and the error
    over the scale of the summed kernel there."""
    net, _, outs = AA.NETS[name]
    x1, x2, blk = AA.block(kind, net, table, extras=(0.0, 1.0))
    want = reference_values(net, AA.TABLES[table], x1, x2, outs)
    rest, sames = restatement_values(net, AA.TABLES[table], x1, x2, kind, outs)
    groups = [t for t in blk.terms if not t[3]]
    assert len(sames) == len(groups)
    for same, (_, t, _, _) in zip(sames, groups):  # the restated device takes act_diag exactly where the referee says it does
        assert np.array_equal(same & blk.mask & (t.scale["nngp"] > 0), t.same & blk.mask & (t.scale["nngp"] > 0))
    for g in outs:
        line = "%s %s %s %s:" % (name, table, kind, g)
        for who, got, extra in (("float64 reference", want[g], 1.0), ("restatement", rest[g], 0.0)):
            ratio, at, of_scale = blk.ratio(got, g, extra)
            line += "  %s worst error / gate %.3f at %s (%.2e of scale)" % (who, ratio, at, of_scale)
            assert ratio <= 1.0, (name, table, kind, g, who, ratio, at)
        print(line)


def test_the_relu_group_map_is_the_restated_per_layer_recursion():
    """group_map's layer loop through act_diag / act_cross equals A.device_relu with diag = same, bit for bit."""
    tab, _ = A.parse_trig_tab()
    x1, x2 = AA.block_rows("few")
    for name in ("relu1", "relu2_bias", "relu3_ntk"):
        net = AA.NETS[name][0]
        for b, e in (AA.G2, AA.G16, AA.G1, (9, 18)):
            with np.errstate(invalid="ignore", divide="ignore"):
                kk, tt, same = AA.device_group(x1, x2, b, e, net, tab)
                a, c = x1[:, b:e], x2[:, b:e]
                acc, qa, qb = np.zeros((a.shape[0], c.shape[0])), np.zeros(a.shape[0]), np.zeros(c.shape[0])
                for f in range(e - b):
                    qa, qb = A.fma(a[:, f], a[:, f], qa), A.fma(c[:, f], c[:, f], qb)
                    acc = A.fma(a[:, f][:, None], c[:, f][None, :], acc)
                inv = 1.0 / (e - b)
                k, q1, q2 = acc * inv, qa * inv, qb * inv
                rk, rt, _ = A.device_relu(k, q1, q2, net, tab, diag=same)
            assert np.array_equal(kk, rk) and np.array_equal(tt, rt)


def test_existing_callers_get_bit_identical_gates():
    """entry() gained optional arguments for this module; the values and gates of a cached block of the plain angle tests are,
    bit for bit, the ones recorded before (tests/golden/angle_gate_d2_few_relu2_bias.npz, written by the unchanged module)."""
    ref = np.load(os.path.join(GOLDEN, "angle_gate_d2_few_relu2_bias.npz"))
    _, _, blk = A.block("d2", "few", A.cases()["relu2_bias"][0], extras=(0.0, 1.0))
    for g in ("nngp", "ntk"):
        assert np.array_equal(blk.gate_abs(g, 0.0), ref["gate0_" + g])
        assert np.array_equal(blk.gate_abs(g, 1.0), ref["gate1_" + g])
        assert np.array_equal(np.array([[float(v) for v in row] for row in blk.val[g]]), ref["val_" + g])


# ------------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("family,group", [("d2", AA.G2), ("d16", AA.G16)])
def test_every_seam_and_both_ends_are_reached_inside_the_group(family, group):
    """The rows' own slices, read back as (a, b) pairs, through A.coverage: every table entry, seam, interval and boundary, and
    the angles 0 and pi exactly."""
    x1, x2 = AA.block_rows("few")
    a_want, s_want = AA.anchor_ab_pairs()[family == "d16"], AA.sweep_ab_pairs()[family == "d16"]
    for x, want in ((x1, a_want), (x2, s_want)):
        assert np.array_equal(x[:, group[0]:group[1]], A.embed(family, want))
    problems, fig = A.coverage(family, a_want, s_want)
    print(family, group, fig)
    assert problems == [] and fig["entries"] == 65 and fig["intervals"] == 16 and fig["max_residual"] <= 0.03
    th = A.plane_angle(a_want, s_want)
    live = (np.abs(a_want).sum(axis=1)[:, None] > 0) & (np.abs(s_want).sum(axis=1)[None, :] > 0)
    assert (th[live] == 0.0).any() and (th[live] == np.pi).any()
    # the two groups see different angles at the same entry
    o2, o16 = A.plane_angle(*[p[0] for p in (AA.anchor_ab_pairs(), AA.sweep_ab_pairs())]), A.plane_angle(*[p[1] for p in (AA.anchor_ab_pairs(), AA.sweep_ab_pairs())])
    assert np.mean(np.abs(o2 - o16) > 0.05) > 0.9


def test_columns_outside_the_groups_differ_between_rows():
    for kind in ("few", "big", "sym"):
        x1, x2 = AA.block_rows(kind)
        x = x1 if x2 is None else np.concatenate([x1, x2])
        for c in AA.FILL:
            assert np.unique(x[:, c]).size == x.shape[0] and np.abs(x[:, c]).min() >= 2 ** 17


def test_exactly_collinear_width_1_entries_have_the_tight_gate():
    """Magnitudes <= 2^12: k k is exact, so is q q' - k^2 = 0 on the device and in the referee, and _ds(0, E) adds nothing: the
    gate is C1 scale, the arctangent's C0 and the sum term.  Magnitudes >= 2^20: k k rounds and the gate widens by itself."""
    net = AA.NETS["relu1"][0]
    _, _, blk = AA.block("few", net, "w1")
    _, _, big = AA.block("big", net, "w1")
    (w, t, _, _), = blk.terms
    live = t.scale["nngp"] > 0
    assert live.sum() > 1500 and (~t.same & live).sum() > 1000
    for g in ("nngp", "ntk"):
        c1, c0 = A.CONSTANTS["relu"][g], A.CONSTANTS["c0"]
        kt = np.abs(blk.value(g))
        assert np.all(blk.gate_abs(g)[live] <= ((c1 + c0) * t.scale[g] + AA.U * kt)[live])
    (_, tb, _, _), = big.terms
    wide = ~tb.same & (tb.scale["ntk"] > 0)
    assert np.all(big.gate_abs("ntk")[wide] > 1e-9 * tb.scale["ntk"][wide])  # sqrt(u): the square root of the rounding of k k


def test_identical_slice_entries_exist_off_the_diagonal():
    net = AA.NETS["relu1"][0]
    x1, x2, blk = AA.block("few", net, "base")
    for (w, t, (b, e), full), least in zip(blk.terms, (3, 3, 100)):
        i, j = np.nonzero(t.same)
        assert len(i) >= least, (b, e, len(i))
        for ii, jj in zip(i, j):  # the slices are the same bits, the rows are not
            assert np.array_equal(x1[ii, b:e], x2[jj, b:e]) and not np.array_equal(x1[ii], x2[jj])
    xs, _, sblk = AA.block("sym", net, "base")
    off = sblk.terms[0][1].same & ~np.eye(xs.shape[0], dtype=bool)
    assert off.any()


# ------------------------------------------------------------------------------------------------- the 1e-6 escape, closed
@pytest.mark.parametrize("table", ["w1", "pair", "base"])
def test_entries_the_older_gate_left_at_1e_6_are_held_tightly(table):
    """tests/test_gpu_additive.py holds every entry at which some term sees collinear, non-identical slices to 1e-6 max |want|
    (additive_reference.degenerate).  On exact inputs the new gate there is below 1e-13 max |want|: for the width-1 group
    (every entry of it), for the pair group's exactly antiparallel entries, and for the three groups together."""
    net = AA.NETS["relu1"][0]
    groups, weights, w0 = AA.TABLES[table]
    x1, x2, blk = AA.block("few", net, table)
    old = R.degenerate(x1, x2, groups, weights, w0, exclude_same=True)
    assert old.sum() >= (1000 if table != "pair" else 1)
    for g in ("nngp", "ntk"):
        top = np.abs(blk.value(g)).max()
        worst = (blk.gate_abs(g)[old] / top).max()
        print("%s %s: %d entries the older gate holds to 1e-6; the new gate there is at most %.2e of max |want|" % (table, g, old.sum(), worst))
        assert worst < 1e-13
