"""The kernel build over the whole angle range on the MI355X (-m gpu): nngp_kernel_build / nngp_kernel_build_act through the C ABI
against the mpmath referee of tests/angle_reference.py, on rows whose pair angles cover [0, pi] with every seam of the
65-entry rotation table (csrc/trig_tab.h) and every boundary of the composite ReLU map's 16 intervals approached from both
sides (coverage asserted in tests/test_angle_math_host.py).  Inputs, referee and the derivation of the per-entry gate are in the
module docstring of angle_reference.py; the gate is computed from the referee alone and no device result took part in its
constants.

How C0 and C1 were measured (CPU; float64 oracle = oracle/nngp_oracle.py::kernel_fn and tests/activation_reference.py,
restatement = the NumPy restatement of the device arithmetic in angle_reference.py; all blocks of cases()):

  first-layer angle error beyond the cancellation term |k| ds(E) / rho^2      restatement 5.2e-16 rad   oracle 3.4e-16 rad
  (plain: 2.3e-15 .. 4.7e-15 within 0.01 .. pi - 0.01, where the term is up to 5.5e-15)       C0 = 4 x 5.2e-16 = 2.1e-15

  value error over scale, plain | beyond the carried angle allowance          oracle               restatement          C1
  1 ReLU layer, NNGP                                                          2.8e-16 | 1.2e-16    3.2e-16 | 1.64e-16   6.6e-16
  1 ReLU layer, NTK (worst next to 0 and pi)                                  2.5e-11 | 1.04e-16   1.1e-9  | 3.6e-17    4.4e-16
  2 / 4 layers, w 1.4, b 0.25, NNGP                                           5.7e-16 | < 0        8.4e-16 | < 0
  2 / 4 layers, w 1.4, b 0.25, NTK                                            3.5e-11 | < 0        2.1e-9  | < 0
  3 layers, no bias, NTK                                                      3.3e-11 | 0          8.7e-12 | 0
  2 .. 12 layers, no bias, NNGP: per-layer path                               7.7e-16 | 0          1.7e-15 | 0
  2 .. 7 layers, no bias, NNGP: composite path (accepted tables)                                   4.8e-16 | 0
  LeakyRelu(0.1) / Abs, NNGP                                                  5.8e-16 | 1.69e-16                        6.8e-16
  LeakyRelu(0.1) / Abs, NTK                                                   1.9e-11 | 8.5e-17                         4.4e-16
  Erf(1, 1, 0), w 1, b 0 (exact Dense layer), NNGP / NTK                      2.2e-16 | 0 / 1.3e-16 | 5e-21             4.4e-16
  Erf(0.8, 1.7, 0.3), w 1.1, b 0.3, NNGP / NTK (nearly parallel rows at norm 2^20: ill conditioned)
                                                                              5.1e-11 | < 0 / 6.8e-5 | 4e-19
  C1 = max(4 x the larger figure beyond the allowance, 4 u); the NTK's plain error is the conditioning the gate carries, not C1.

Why the allowance is per layer and conditioned (float64 oracle against mpmath on the d = 2 blocks, worst error over scale; the
NTK's worst is always next to theta = 0): any honest float64 evaluation loses the NTK's digits at small angles, at every
depth, and a flat tolerance would either fail the oracle or hide a wrong table entry at ordinary angles.

Composite tables on the build host (port of comp_build_host): 2 .. 7 ReLU layers accepted (worst 9.9e-17 .. 2.2e-16), 8 refused
(4.7e-16), 9 .. 15 refused (1.4e-15 .. 1.7e-13); the gate does not depend on which path the library takes.

Worst device error / gate on the MI355X (this file's printout): per-layer ReLU path 0.33 (NNGP) and 0.90 (NTK; the symmetric d = 16
build, nearly parallel rows, where the allowance is the rounding of k k and the restatement of the device
arithmetic sits at the same level); composite path 0.16 (2 .. 7 layers), its per-layer fallback at 8 and 12 layers 0.08; composite against per-layer (key 5 = 63)
4.4e-16 .. 1.0e-15 of scale; Erf 0.30, LeakyRelu / Abs 0.54; the other kernel forms (keys 3 = 3, 4 and 5 = 21 .. 27) 0.76.
Value-only mutations of the device code, each run once on scratch copies: entry 48's angle pair moved by 1e-12 fails 23 tests
here (every ReLU case but 12 layers, Erf, ABRelu, the tilings) and, of the existing kernel-build and activation tests, only
test_kernel_build_composite_relu_map[2-1.0]; 1 / 7.5 for the series' 1 / 7 fails 24 here and two composite cases there; interval 1's
constant coefficient raised by 1e-12 fails the 8 composite tests here and nothing there.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import angle_reference as A  # noqa: E402
import gpu_util as G  # noqa: E402
from nngp_src_amd import _lib  # noqa: E402
from nngp_src_amd.model import GPModel  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = A.cases()


def build(net, x1, x2, get, **kw):
    if net.family == "relu":
        return G.kernel_build(x1, x2, net.w_std, net.b_std, get=get, **kw)
    assert not kw.get("knobs")
    return G.build_act(x1, x2, net.w_std, net.b_std, net.acts, get=get, **kw)


def check_block(name, family, kind, got_of, extra_note=""):
    """Hold what got_of(x1, x2, outs, ld) returns to the gate of the case's block; prints worst error / gate per output."""
    net, _, outs = CASES[name]
    x1, x2, blk = A.block(family, kind, net)
    n2 = blk.k.shape[1]
    ld = None if kind == "sym" else (n2 + 3 if kind != "few" else (n2 + 7) // 4 * 4)  # odd padding; 16-byte rows
    got = got_of(x1, x2, outs, ld)
    for g in outs:
        out = got[g]
        if ld is not None:
            assert np.isnan(out[:, n2:]).all()  # padding columns untouched
            out = out[:, :n2]
        assert np.all(np.isfinite(out))
        if kind == "sym":
            assert np.array_equal(out, out.T)
        ratio, at = blk.ratio(out, g)
        err, gate = blk.error_abs(out, g), blk.gate_abs(g)
        print("%s %s %s %s%s: error %.2e of scale, worst error / gate %.3f at %s (error %.3e, gate %.3e there)"
              % (name, family, kind, g, extra_note, blk.of_scale(err, g).max(), ratio, at, err[at], gate[at]))
        assert ratio <= 1.0, (name, family, kind, g, ratio, at, float(err[at]), float(gate[at]))
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_build_meets_the_gate(name):
    """Per-layer path: relu1 (NNGP + NTK), relu2_bias / relu4_bias, relu3_ntk (NTK requested: no composite map).  Composite path:
    comp2 .. comp12 (NNGP only; 8 and 12 fall back to the per-layer recursion where the table is refused -- same gate).  General
    activations: erf, erf_abc, leaky, abs.  Rectangular anchor blocks with a padded ld, and the symmetric build."""
    net, blocks, outs = CASES[name]
    for family, kind in blocks:
        got = check_block(name, family, kind, lambda x1, x2, o, ld: build(net, x1, x2, o, ld=ld))
        x1, x2, _ = A.block(family, kind, net)
        again = build(net, x1, x2, outs)  # determinism, and the unpadded ld
        for g in outs:
            np.testing.assert_array_equal(again[g], got[g][:, : again[g].shape[1]])
        if len(outs) == 2 and kind in ("few", "sym"):  # one output alone: the same bits, except where NNGP alone takes the composite map
            for g in outs:
                alone = build(net, x1, x2, (g,))[g]
                if not (g == "nngp" and net.family == "relu" and net.nd >= 3 and all(b == 0.0 for b in net.b2)):
                    np.testing.assert_array_equal(alone, again[g])


@pytest.mark.parametrize("name", ["comp2", "comp3", "comp4", "comp7"])
def test_composite_map_against_the_per_layer_path(name):
    """Timing-knob key 5 = 63 switches the composite map off: 2e-13 of scale between the two (the existing number), and the
    per-layer path of the same NNGP-only build meets the gate as well."""
    net, blocks, outs = CASES[name]
    family, kind = blocks[0]
    x1, x2, blk = A.block(family, kind, net)
    comp = G.kernel_build(x1, x2, net.w_std, net.b_std, get=("nngp",), knobs=True)["nngp"]
    lib = _lib.load(knobs=True)
    lib.nngp_debug_set(5, 63)
    try:
        check_block(name, family, kind, lambda a, b, o, ld: G.kernel_build(a, b, net.w_std, net.b_std, get=o, ld=ld, knobs=True),
                    " (key 5 = 63)")
        layered = G.kernel_build(x1, x2, net.w_std, net.b_std, get=("nngp",), knobs=True)["nngp"]
    finally:
        lib.nngp_debug_set(5, 0)
    np.testing.assert_array_equal(comp, G.kernel_build(x1, x2, net.w_std, net.b_std, get=("nngp",))["nngp"])  # knobs build = product
    zero = blk.scale["nngp"] == 0.0  # zero rows
    assert zero.any() and np.all(comp[zero] == 0.0) and np.all(layered[zero] == 0.0)
    diff = blk.of_scale(np.abs(comp - layered), "nngp")
    print(name, "composite vs per-layer: %.2e of scale" % diff.max())
    assert diff.max() < 2e-13
    if net.nd - 1 <= 4:  # these tables are accepted on every host (test_angle_math_host.py): two different paths ran
        assert not np.array_equal(comp, layered)


VARIANTS = [(3, 3), (3, 4)] + [(5, v) for v in (21, 22, 23, 24, 25, 27)]


@pytest.mark.parametrize("key,value", VARIANTS)
def test_the_other_kernel_forms_meet_the_same_gate(key, value):
    """The knobs build's A/B baselines (key 3 = 3: the first kernel on the matrix cores, 4: on the vector ALUs, both with libm;
    key 5 = 21 .. 27: the tilings of the current kernel): measurements are quoted from them, so they are held to the same gate."""
    lib = _lib.load(knobs=True)
    lib.nngp_debug_set(key, value)
    try:
        for name, family, kind in (("relu1", "d2", "ends"), ("relu2_bias", "d16", "few"), ("relu3_ntk", "d2", "few")):
            net = CASES[name][0]
            check_block(name, family, kind, lambda a, b, o, ld: G.kernel_build(a, b, net.w_std, net.b_std, get=o, ld=ld, knobs=True),
                        " (key %d = %d)" % (key, value))
    finally:
        lib.nngp_debug_set(key, 0)


@pytest.mark.parametrize("name", ["relu1", "relu2_bias", "relu3_ntk"])
def test_relu_spelled_as_abrelu_gives_the_relu_bits(name):
    """The C ABI maps ABRelu(0, 1) to the ReLU kernels (existing property) -- at these angles too."""
    net = CASES[name][0]
    x1, x2 = A.block_rows("d2", "few")
    arch = _lib.make_arch_act(net.w_std, net.b_std, [("relu",)] * (net.nd - 1))
    for l in range(net.nd - 1):
        arch.act[l] = _lib.ACT_ABRELU
        arch.p[l][0], arch.p[l][1] = 0.0, 1.0
    lib = _lib.load()
    x1d, x2d = _lib.to_device_f64(x1, G.dev()), _lib.to_device_f64(x2, G.dev())
    n1, n2 = x1.shape[0], x2.shape[0]
    kn = torch.full((n1, n2), float("nan"), dtype=torch.float64, device=G.dev())
    kt = torch.full_like(kn, float("nan"))
    _lib.check(lib.nngp_kernel_build_act(_lib.ptr(x1d), n1, _lib.ptr(x2d), n2, x1.shape[1], ctypes.byref(arch), _lib.DTYPE_F64,
                                         _lib.ptr(kn), _lib.ptr(kt), n2, 0, n1, _lib.stream_ptr()))
    torch.cuda.synchronize()
    want = G.kernel_build(x1, x2, net.w_std, net.b_std)
    np.testing.assert_array_equal(kn.cpu().numpy(), want["nngp"])
    np.testing.assert_array_equal(kt.cpu().numpy(), want["ntk"])


@pytest.mark.parametrize("name", ["relu1", "relu4_bias", "comp3", "erf_abc", "leaky"])
def test_float32_outputs_are_the_float64_outputs_rounded_once(name):
    net, blocks, outs = CASES[name]
    x1, x2 = A.block_rows(*blocks[0])
    f64 = build(net, x1, x2, outs)
    f32 = build(net, x1, x2, outs, dtype=torch.float32)
    for g in outs:
        assert f32[g].dtype == np.float32
        np.testing.assert_allclose(f32[g], f64[g], rtol=2e-7, atol=1e-30)
        assert np.array_equal(f32[g], f64[g].astype(np.float32))  # rounded once, to nearest


@pytest.mark.parametrize("name", ["relu1", "relu4_bias", "comp3", "erf_abc", "leaky"])
@pytest.mark.parametrize("family", ["d2", "d16"])
def test_diagonal_entry_point_is_the_symmetric_diagonal(name, family):
    """nngp_kernel_diag / nngp_kernel_diag_act equal the symmetric build's diagonal bit for bit on rows of radius 3 .. 2^25 (and a
    zero row), and the referee's diagonal to the roundings of their own operations."""
    net, _, outs = CASES[name]
    ab = np.concatenate([A.anchors_ab(family), A.end_anchors_ab(family), A.symmetric_ab(family)[:70]])
    x = A.embed(family, ab)
    radius = np.sqrt(np.sum(x * x, axis=1))
    assert radius.min() == 0.0 and np.sort(radius)[1] <= 273.0 and radius.max() >= 2.0 ** 24
    got = build(net, x, None, outs)
    dn, dt = G.kernel_diag(x, net.w_std, net.b_std) if net.family == "relu" else G.diag_act(x, net.w_std, net.b_std, net.acts)
    for g, dv in zip(("nngp", "ntk"), (dn, dt)):
        if g in outs:
            np.testing.assert_array_equal(np.diag(got[g]), dv)
    k, q, _ = A.gram(x, x)
    # per Dense layer one fma, per ReLU an exact halving (u per layer); ABRelu: the rounded (a^2 + b^2) / 2 and a product more
    # (2 u); Erf: the arctangent (C0), its rounded constants, its argument and w (6 u)
    per_layer = {"relu": A.U, "abrelu": 2 * A.U, "erf": A.CONSTANTS["c0"] + 6 * A.U}[net.family]
    for i in range(0, len(q), 3):
        kk, tt, _, _ = A.entry(q[i], q[i], q[i], net, A.CONSTANTS["c0"], exact_diag=True)
        for ref, dv in ((kk, dn), (tt, dt)):
            assert abs(A.mp.mpf(float(dv[i])) - ref) <= (2 * net.nd) * per_layer * 1.01 * ref, (i, float(dv[i]), float(ref))


@pytest.mark.parametrize("name,get", [("relu1", "nngp"), ("relu1", "ntk"), ("relu2_bias", "ntk"), ("comp3", "nngp")])
def test_fit_path_builds_the_operator_bits(name, get):
    """nngp_model_set_train + nngp_model_build_rows on the symmetric sweep rows, read through nngp_model_kernel_buffer, equals the
    stand-alone operator bit for bit (an NNGP model of a bias-free network takes the composite map there too)."""
    net = CASES[name][0]
    for family in ("d2", "d16"):
        x = A.embed(family, A.symmetric_ab(family))
        n = x.shape[0]
        model = GPModel(n, x.shape[1], net.w_std, net.b_std, get=get)
        model.set_train(x, np.linspace(-1.0, 1.0, n))
        model.build_rows(0, n)
        kbuf, _ = model.kernel_buffer()
        torch.cuda.synchronize()
        got = kbuf[:, :n].cpu().numpy()
        model.close()
        np.testing.assert_array_equal(got, G.kernel_build(x, None, net.w_std, net.b_std, get=(get,))[get])
