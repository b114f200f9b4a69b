"""The additive kernel build over the whole angle range on the MI355X (-m gpu): nngp_kernel_build_additive and
nngp_kernel_diag_additive through the C ABI against the mpmath referee of tests/additive_angle_reference.py, entry by entry, on
rows whose groups each carry an exact-input sweep of [0, pi] (every seam of the rotation table and both ends inside the width-2 and
the width-16 group, exactly collinear width-1 slices, identical slices on different rows; coverage asserted in
tests/test_additive_angles_host.py).  Inputs, referee and gate are described in additive_angle_reference.py; the gate is computed
from the referee alone and no device result took part in its constants.

Worst device error / gate on the MI355X (this file's printout; NNGP, NTK):
  rectangular, three groups:   relu1 0.26, 0.31; relu2_bias 0.15, 0.17; relu3_ntk 0.17, 0.21; leaky 0.35, 0.28; abs 0.41, 0.47;
                               erf 0.19, 0.16; erf_abc 0.17, 0.02; comp3 (whole-input term by the composite map) 0.12
  symmetric and its row range: relu1 0.24, 0.90 (nearly parallel width-16 slices: the rounding of k k; the restatement of the device
                               arithmetic sits at the same 0.90); relu2_bias 0.22, 0.30; relu3_ntk 0.19, 0.21; leaky 0.29, 0.37;
                               abs 0.43, 0.47; erf 0.37, 0.12; erf_abc 0.35, 0.04; comp3 0.23
  the other group tables:      relu1 <= 0.24, <= 0.36 (widths 3 and 7); erf_abc <= 0.24, <= 0.17
  identical slices, other rows: <= 0.38, <= 0.28 (relu1: the bits of the referee's value rounded)
  exactly collinear slices:    width 1 at |x| <= 2^12 0.00 (every one of the 1791 entries is the referee's value rounded); the width-2
                               group's 10 entries 0.06; width 1 at |x| >= 2^20 0.88 (k k rounds: sqrt(u) of angle, carried by the gate)
  nngp_kernel_diag_additive:   <= 0.65 (erf), the symmetric build's diagonal bit for bit
  erf_abc on slices within 1e-3 rad at raw norms (reported only): device 2.2e-16 / 2.7e-17 of scale, float64 reference 2.1e-12 / 6.0e-6.
No defect was found in kernel_build_additive.hip.
Value-only mutations of kernel_build_additive.hip, each built on a scratch copy and run once against this file and
tests/test_gpu_additive.py (failed tests here | there): same[r][c] = false 18 | 10; q2[c] (1 + 1e-12) into act_cross 23 | 13;
the second group's wg (1 + 1e-12) 37 | 0; inv_dg (1 + 1e-12) for q, q' only 46 | 14.  With same = false the relu1 and Erf cases of
test_identical_slices_... still pass: the anchors' slices have q q an exact float64 number (rr is exactly 0 either way), and
erf_cross_comp's bracket is exactly 0 at k = q = q'; the symmetric blocks and the biased / ABRelu networks see the mutation.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import additive_angle_reference as AA  # noqa: E402
import additive_reference as R  # noqa: E402
import angle_reference as A  # noqa: E402
import gpu_util as G  # noqa: E402
from nngp_src_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
BOTH = ("nngp", "ntk")


def _arch(net):
    return _lib.make_arch_act(net.w_std, net.b_std, net.acts)


def build_add(x1, x2, net, table, get=BOTH, rows=None, dtype=torch.float64, ld=None, rc=False):
    lib = _lib.load()
    groups, weights, w0 = table
    x1d = _lib.to_device_f64(x1, G.dev())
    x2d = None if x2 is None else _lib.to_device_f64(x2, G.dev())
    n1, d = x1d.shape
    n2 = n1 if x2d is None else x2d.shape[0]
    ld = n2 if ld is None else ld
    outs = {g: torch.full((n1, ld), float("nan"), dtype=dtype, device=G.dev()) for g in get}
    arch, tab = _arch(net), _lib.make_groups(tuple(groups), tuple(weights), w0)
    r0, r1 = (0, n1) if rows is None else rows
    code = lib.nngp_kernel_build_additive(_lib.ptr(x1d), n1, _lib.ptr(x2d), n2, d, ctypes.byref(arch), ctypes.byref(tab),
                                          _lib.DTYPE_F64 if dtype == torch.float64 else _lib.DTYPE_F32,
                                          _lib.ptr(outs.get("nngp")), _lib.ptr(outs.get("ntk")), ld, r0, r1, _lib.stream_ptr())
    if rc:
        return code
    _lib.check(code)
    torch.cuda.synchronize()
    return {g: t.cpu().numpy() for g, t in outs.items()}


def diag_add(x, net, table):
    lib = _lib.load()
    groups, weights, w0 = table
    xd = _lib.to_device_f64(x, G.dev())
    dn = torch.full((xd.shape[0],), float("nan"), dtype=torch.float64, device=G.dev())
    dt = torch.full_like(dn, float("nan"))
    arch, tab = _arch(net), _lib.make_groups(tuple(groups), tuple(weights), w0)
    _lib.check(lib.nngp_kernel_diag_additive(_lib.ptr(xd), xd.shape[0], xd.shape[1], ctypes.byref(arch), ctypes.byref(tab),
                                             _lib.ptr(dn), _lib.ptr(dt), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dn.cpu().numpy(), dt.cpu().numpy()


def hold(blk, got, outs, what, where=None):
    """got[g] against the gate; prints worst error / gate per output, as check_block of test_gpu_kernel_angles.py does."""
    for g in outs:
        assert np.all(np.isfinite(got[g])), (what, g)
        ratio, at, of_scale = blk.ratio(got[g], g, where=where)
        print("%s %s: worst error / gate %.3f at %s (error %.2e of scale there)" % (what, g, ratio, at, of_scale))
        assert ratio <= 1.0, (what, g, ratio, at)


def _padded(n2, odd):
    """ld > n2: odd (rows not 16-byte aligned: the scalar stores) or a multiple of 4 (the 16-byte stores)."""
    return n2 + 3 - (n2 % 2) if odd else (n2 + 7) // 4 * 4


@pytest.mark.parametrize("name", list(AA.NETS))
def test_rectangular_build_meets_the_gate(name):
    """Three anchors x the medium sweep, float64, NNGP and NTK, odd ld with NaN padding; the aligned ld and each output alone give
    the same bits."""
    net, tname, outs = AA.NETS[name]
    table = AA.TABLES[tname]
    x1, x2, blk = AA.block("few", net, tname)
    n2 = x2.shape[0]
    ld = _padded(n2, True)
    assert ld % 2 == 1
    got = build_add(x1, x2, net, table, outs, ld=ld)
    for g in outs:
        assert np.isnan(got[g][:, n2:]).all()  # the padding is not written
        got[g] = got[g][:, :n2]
    hold(blk, got, outs, "%s %s rect" % (name, tname))
    aligned = build_add(x1, x2, net, table, outs, ld=_padded(n2, False))
    for g in outs:
        np.testing.assert_array_equal(aligned[g][:, :n2], got[g])
        assert np.isnan(aligned[g][:, n2:]).all()
        np.testing.assert_array_equal(build_add(x1, x2, net, table, (g,))[g], got[g])  # alone (comp3: NNGP is all there is)


@pytest.mark.parametrize("name", list(AA.NETS))
def test_symmetric_build_and_a_row_range_meet_the_gate(name):
    """75 rows (a full and a ragged tile a side): the lower triangle against the gate, bitwise symmetry, each output alone, and the
    rows [5, 70) of the same problem built as a row range (not the symmetric build: the whole-input term's diagonal then takes
    the cross-entry form; the group terms take act_diag there all the same, so without a whole-input term the bits are equal)."""
    net, tname, outs = AA.NETS[name]
    table = AA.TABLES[tname]
    x, _, blk = AA.block("sym", net, tname)
    n = x.shape[0]
    got = build_add(x, None, net, table, outs)
    for g in outs:
        assert np.array_equal(got[g], got[g].T)
        np.testing.assert_array_equal(build_add(x, None, net, table, (g,))[g], got[g])
    hold(blk, got, outs, "%s %s sym" % (name, tname))
    part = build_add(x, x, net, table, outs, rows=(5, 70), ld=_padded(n, True))
    strict = np.tril(np.ones((n, n), dtype=bool), -1)
    strict[:5], strict[70:] = False, False
    for g in outs:
        assert np.isnan(part[g][:5]).all() and np.isnan(part[g][70:]).all() and np.isnan(part[g][:, n:]).all()
        rows, low = part[g][5:70, :n], np.tril(np.ones((n, n), dtype=bool))[5:70]
        if table[2] == 0.0:  # the same operations in the same order at and below the diagonal; above it the symmetric build
            np.testing.assert_array_equal(rows[low], got[g][5:70][low])  # mirrors, the row range computes with q, q' exchanged
            if net.family != "erf":  # (every map but erf_cross_comp's lo term is symmetric in q, q' bit for bit)
                np.testing.assert_array_equal(rows, got[g][5:70])
        cols = np.zeros((n, n), dtype=bool)
        cols[:, 5:70] = True
        above = np.tril(cols, -1)  # entry (j, i) of the row range, j in [5, 70), i > j: held as (i, j) is
        lower = np.where(strict, np.nan_to_num(part[g][:, :n]), 0.0)
        upper = np.where(above, np.nan_to_num(part[g][:, :n]).T, 0.0)
        hold(blk, {g: lower}, (g,), "%s %s rows [5, 70) below the diagonal" % (name, tname), where=strict)
        hold(blk, {g: upper}, (g,), "%s %s rows [5, 70) above the diagonal" % (name, tname), where=above)


@pytest.mark.parametrize("tname", AA.DEVICE_TABLES)
@pytest.mark.parametrize("name", ["relu1", "erf_abc"])
def test_every_group_table_meets_the_gate(name, tname):
    """Chunk boundaries (widths 8, 9, 17 from odd offsets), overlapping groups, a group equal to the whole input, widths 3 and 7, a
    weight of 0, full_weight 1 beside the groups."""
    net = AA.NETS[name][0]
    table = AA.TABLES[tname]
    x1, x2, blk = AA.block("few", net, tname)
    got = build_add(x1, x2, net, table)
    hold(blk, got, BOTH, "%s %s rect" % (name, tname))
    if tname == "zero_w":  # a group of weight 0 is left out: the bits of the table without it
        groups, weights, w0 = table
        keep = [i for i, w in enumerate(weights) if w != 0.0]
        assert len(keep) < len(weights)
        other = build_add(x1, x2, net, ([groups[i] for i in keep], [weights[i] for i in keep], w0))
        for g in BOTH:
            np.testing.assert_array_equal(other[g], got[g])


def test_a_negative_weight_is_refused():
    """The referee and the host file hold the table "neg_w"; the C ABI does not take it."""
    net = AA.NETS["relu1"][0]
    x1, x2 = AA.block_rows("few")
    assert build_add(x1, x2[:8], net, AA.TABLES["neg_w"], rc=True) == -2


@pytest.mark.parametrize("name", ["relu1", "relu2_bias", "leaky", "erf_abc"])
def test_identical_slices_on_different_rows_take_the_diagonal_form(name):
    """The `same` rule off the diagonal: entries whose width-2 (width-16) slices are bit-identical while the rows differ meet the gate
    of an exact-diagonal entry -- no angle allowance at all -- for Theta and K."""
    net = AA.NETS[name][0]
    for tname, (b, e) in (("pair", AA.G2), ("g16", AA.G16)):
        x1, x2, blk = AA.block("few", net, tname)
        t = [t for _, t, be, _ in blk.terms if be == (b, e)][0]
        where = t.same & (t.scale["ntk"] > 0)
        assert where.sum() >= 3 and all(not np.array_equal(x1[i], x2[j]) for i, j in zip(*np.nonzero(where)))
        for g in BOTH:
            assert np.all(t.carry[(g, 0.0)][where] == 0.0)
        got = build_add(x1, x2, net, AA.TABLES[tname])
        hold(blk, got, BOTH, "%s %s identical [%d, %d) slices (%d entries)" % (name, tname, b, e, where.sum()), where=where)


@pytest.mark.parametrize("kind,tname", [("few", "w1"), ("few", "pair"), ("few", "base"), ("big", "w1")])
def test_exactly_collinear_slices_meet_the_tight_gate(kind, tname):
    """The entries tests/test_gpu_additive.py holds to 1e-6 max |want| (some term sees collinear, non-identical slices): on exact
    inputs q q' - k^2 is exactly 0 on the device and in the referee, and they are held to the gate like any other.  With
    magnitudes >= 2^20 (kind "big") k k rounds and the gate widens by itself."""
    net = AA.NETS["relu1"][0]
    groups, weights, w0 = AA.TABLES[tname]
    x1, x2, blk = AA.block(kind, net, tname)
    old = R.degenerate(x1, x2, groups, weights, w0, exclude_same=True)
    assert old.sum() >= (1 if tname == "pair" else 1000)
    got = build_add(x1, x2, net, AA.TABLES[tname])
    for g in BOTH:
        top = np.abs(blk.value(g)).max()
        print("%s %s %s: the older gate would have left %d of %d entries at 1e-6 max |want|; the gate there is at most %.2e of it" % (
            kind, tname, g, old.sum(), old.size, (blk.gate_abs(g)[old] / top).max()))
    hold(blk, got, BOTH, "relu1 %s %s collinear entries" % (kind, tname), where=old)
    hold(blk, got, BOTH, "relu1 %s %s" % (kind, tname))


@pytest.mark.parametrize("name", list(AA.NETS))
def test_diagonal_entry_point(name):
    """nngp_kernel_diag_additive: the symmetric build's diagonal bit for bit, and entry by entry the referee's exact diagonal
    (the gate of an exact-diagonal entry: C1 (+ CD) of |K_t| per term and the sum's roundings), on the symmetric rows and on
    the sweep rows."""
    net, tname, outs = AA.NETS[name]
    table = AA.TABLES[tname]
    xs = AA.sym_rows()
    full = build_add(xs, None, net, table, outs)
    for x in (xs, AA.sweep_rows()):
        dn, dt = diag_add(x, net, table)
        if x is xs:
            for g, dv in zip(BOTH, (dn, dt)):
                if g in outs:
                    np.testing.assert_array_equal(np.diag(full[g]), dv)
        ref = AA.diag_referee(x, net, table)
        worst = 0.0
        for o, (g, dv) in enumerate(zip(BOTH, (dn, dt))):
            c = A.CONSTANTS[net.family][g] + AA.CD.get(net.family, {}).get(g, 0.0) + len(AA.live_terms(table)) * AA.U
            for i, r in enumerate(ref):
                err, gate = abs(A.mp.mpf(float(dv[i])) - r[o]), c * r[2 + o]
                assert err <= gate, (name, g, i, float(err), float(gate))
                worst = max(worst, float(err / gate) if gate > 0 else 0.0)
        print("%s diag (%d rows): worst error / gate %.3f" % (name, x.shape[0], worst))


@pytest.mark.parametrize("name", ["relu1", "relu2_bias", "erf_abc", "leaky", "comp3"])
def test_float32_outputs_are_the_float64_outputs_rounded_once(name):
    net, tname, outs = AA.NETS[name]
    x1, x2 = AA.block_rows("few")
    f64 = build_add(x1, x2, net, AA.TABLES[tname], outs)
    f32 = build_add(x1, x2, net, AA.TABLES[tname], outs, dtype=torch.float32, ld=_padded(x2.shape[0], True))
    for g in outs:
        assert f32[g].dtype == np.float32 and np.isnan(f32[g][:, x2.shape[0]:]).all()
        assert np.array_equal(f32[g][:, : x2.shape[0]], f64[g].astype(np.float32))


def test_erf_on_nearly_parallel_slices_beside_the_float64_reference():
    """Reported only (the forest case of tests/test_gpu_additive.py asserts the relation): erf_abc where a group's slices are
    within 1e-3 rad at raw norms -- the compensated bracket of erf_cross_comp -- the device's and the float64 reference's error
    against the referee."""
    net, tname, _ = AA.NETS["erf_abc"]
    groups, weights, w0 = AA.TABLES[tname]
    x1, x2, blk = AA.block("few", net, tname)
    (a2, a16), (s2, s16) = AA.anchor_ab_pairs(), AA.sweep_ab_pairs()
    th2, th16 = A.plane_angle(a2, s2), A.plane_angle(a16, s16)
    near = ((th2 < 1e-3) & ~blk.terms[0][1].same) | ((th16 < 1e-3) & ~blk.terms[1][1].same)
    assert near.sum() >= 10
    got = build_add(x1, x2, net, AA.TABLES[tname])
    for g in BOTH:
        want = R.kernel_fn(x1, x2, g, net.w_std, net.b_std, net.acts, groups, weights, w0, exact_same=True)
        ed, er = blk.error_abs(got[g], g), blk.error_abs(want, g)
        sc = blk.scale[g]
        print("erf_abc nearly parallel slices (%d entries) %s: device %.2e of scale, float64 reference %.2e, gate %.2e" % (
            near.sum(), g, (ed / sc)[near].max(), (er / sc)[near].max(), (blk.gate_abs(g) / sc)[near].max()))
