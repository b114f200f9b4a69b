"""The additive kernel's marginal likelihood and its gradient, term weights included, on the MI355X (include/nngp_additive_mll.h,
nngp-src_amd/additive_mll.py) against the NumPy oracle of additive_mll_reference.py (forward-mode tangents, scipy Cholesky).

Gates (those of test_gpu_nngp_mll.py): NLML 1e-9 relative; every gradient component, weights included, within
1e-8 max(|half1|, |half2|) of the oracle; tr K, tr K^(t) and tr dK 1e-12 relative; -1/2 half1 + 1/2 half2 == grad exactly."""
import contextlib
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import additive_mll_reference as AM  # noqa: E402
import additive_reference as AR  # noqa: E402
import gpu_util as G  # noqa: E402
import nngp_mll_reference as R  # noqa: E402
from nngp_src_amd import _lib, additive_mll, loo, mll, predict, stax, synth, train as train_cli  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

GROUPS7 = [(0, 2), (2, 3), (3, 7), (1, 5)]  # a width-1 group, an overlap
WEIGHTS7 = [0.5, 1.0, 0.7, 0.0, 1.3]        # group (3, 7) has weight 0


def _pairs(d):
    return list(_lib.pair_groups(d))


def _table(name):
    """(d, groups, weights): the group tables of the parity test."""
    if name == "pairs20":
        return 20, _pairs(20), [0.8] + [0.5 + 0.15 * g for g in range(10)]
    if name == "pairs20_no_full":  # w0 = 0
        return 20, _pairs(20), [0.0] + [1.0 + 0.1 * g for g in range(10)]
    if name == "d7":
        return 7, GROUPS7, WEIGHTS7
    if name == "d45_wide":  # one group wider than any staging chunk, plus pairs
        return 45, [(4, 41)] + _pairs(44), [0.6, 1.5] + [0.9] * 22
    if name == "d130_width1":  # more terms than any per-launch batch one would pick
        return 130, [(k, k + 1) for k in range(130)], [0.7] + [0.5 + 0.01 * k for k in range(130)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _rows(kind, n, d):
    if kind == "synth":
        x, y = synth.synthetic_queries(n, d + d % 2, seed=n + d)
        x, y = x[:, :d] / 1000.0, y.reshape(-1)
    else:
        g = np.load(os.path.join(GOLDEN, "forest_n1000_m200.npz"))
        assert d == 20
        x = np.concatenate([g["X_train"], g["X_test"]])[:n].astype(np.float64)
        y = np.concatenate([g["Y_train"], g["Y_test"]])[:n].reshape(-1)
        if kind != "raw":
            x = x / 1000.0
        if kind == "centred":  # obtuse angles and mixed signs
            x = x - x.mean(0)
    return x, y  # shared between the tests: none of them writes to it


def _net(n_dense, w_std, b_std, act=("relu",)):
    return tuple([w_std] * n_dense), tuple([b_std] * n_dense), tuple([act] * (n_dense - 1))


@functools.lru_cache(maxsize=None)
def _reference(kind, n, table, net, lam, absolute):
    """The oracle's result for one case, computed once and shared."""
    d, groups, weights = _table(table)
    x, y = _rows(kind, n, d)
    w, b, acts = net
    v, c = R.variances(w, b)
    return AM.Oracle(x, y, groups).full(v, c, list(acts), lam, weights, absolute)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check(m, nlml, g, gw, ref, extra=0.0, label=""):
    """The gates of the module docstring; ``extra`` widens the gradient gates (the collinear-slice test's derived bound).  Returns
    the worst distance / max half over all gradient components."""
    t, ta = m.terms(), m.additive_terms()
    size = np.maximum(np.abs(ref["quad"]), np.abs(ref["trace"]))
    size_w = np.maximum(np.abs(ref["half1_w"]), np.abs(ref["half2_w"]))
    worst = max(np.max(np.abs(g - ref["grad"]) / size), np.max(np.abs(gw - ref["grad_w"]) / size_w))
    print("%s nlml rel %.2e, worst gradient distance / max half %.2e" % (label, _rel(nlml, ref["nlml"]), worst))
    assert _rel(nlml, ref["nlml"]) <= 1e-9, (nlml, ref["nlml"])
    assert np.all(np.abs(g - ref["grad"]) <= (1e-8 + extra) * size), (g, ref["grad"], size)
    assert np.all(np.abs(gw - ref["grad_w"]) <= (1e-8 + extra) * size_w), (gw, ref["grad_w"], size_w)
    assert _rel(t["tr_k"], ref["tr_k"]) <= 1e-12
    np.testing.assert_allclose(t["tr_dk"], ref["tr_dk"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(ta["tr_k_term"], ref["tr_k_term"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(-0.5 * t["quad"] + 0.5 * t["trace"], g, rtol=0, atol=0)
    np.testing.assert_allclose(-0.5 * ta["half1"] + 0.5 * ta["half2"], gw, rtol=0, atol=0)
    return worst


LEAKY = ("abrelu", 0.1, 1.0)
CASES = [  # rows, n, table, net, absolute
    ("synth", 127, "pairs20", _net(2, 1.0, 0.0), False),           # a ragged tile
    ("synth", 130, "d7", _net(3, 1.2, 0.05), True),                # three tiles a side; width 1, overlap, zero weight
    ("synth", 192, "d45_wide", _net(2, 1.5, 0.05), False),         # exact tiles; a 37-wide group
    ("unit", 1000, "pairs20", _net(3, 1.0, 0.0), False),           # many tiles
    ("synth", 1000, "pairs20_no_full", _net(2, 1.5, 0.05), True),  # w0 = 0
    ("unit", 1000, "pairs20", _net(3, 1.2, 0.05, LEAKY), False),   # an ABRelu network
    ("synth", 127, "d7", _net(5, 1.5, 0.05), False),               # NLC = 8
    ("unit", 127, "pairs20", _net(9, 1.2, 0.05), True),            # NLC = 16
    ("synth", 127, "d130_width1", _net(2, 1.0, 0.05), False),      # 131 terms (with b_std = 0: the collinear test below)
    ("synth", 192, "d7", _net(3, 1.0, 0.0), False),                # b_std = 0 with the zero weight
    ("centred", 1000, "pairs20", _net(2, 1.0, 0.0), False),        # obtuse angles
]


@pytest.mark.parametrize("kind,n,table,net,absolute", CASES)
def test_nlml_and_gradient_against_the_oracle(kind, n, table, net, absolute):
    d, groups, weights = _table(table)
    x, y = _rows(kind, n, d)
    ref = _reference(kind, n, table, net, 1e-3, absolute)
    m = additive_mll.AdditiveMarginalLikelihood(n, d, groups).set_train(x, y)
    nlml, g, gw = m.evaluate(net, 1e-3, absolute, weights=weights)
    _check(m, nlml, g, gw, ref, label="%s n=%d %s nd=%d" % (kind, n, table, len(net[0])))
    # bit-identical repeats; the NLML alone equals the one with the gradient
    nlml2, g2, gw2 = m.evaluate(net, 1e-3, absolute, weights=weights)
    assert nlml2 == nlml and np.array_equal(g2, g) and np.array_equal(gw2, gw)
    nlml3, none, none_w = m.evaluate(net, 1e-3, absolute, with_grad=False, weights=weights)
    assert none is None and none_w is None and nlml3 == nlml
    m.close()


@pytest.mark.parametrize("net", [_net(2, 1.0, 0.0), _net(3, 1.1, 30.0)])
def test_raw_forest_rows_with_pairs(net):
    """Untouched default predicates give identical slices on different rows: the identical-slice rule, off the diagonal."""
    x, y = _rows("raw", 1000, 20)
    xs = x[:, 0:2]
    assert np.sum(np.all(xs[:, None, :] == xs[None, :, :], axis=2)) > 10 * x.shape[0]
    ref = _reference("raw", 1000, "pairs20", net, 1e-3, False)
    _, groups, weights = _table("pairs20")
    m = additive_mll.AdditiveMarginalLikelihood(1000, 20, groups).set_train(x, y)
    nlml, g, gw = m.evaluate(net, 1e-3, weights=weights)
    _check(m, nlml, g, gw, ref, label="raw forest nd=%d" % len(net[0]))
    m.close()


@pytest.mark.parametrize("n_dense", [2, 3])
def test_collinear_but_not_identical_slices(n_dense):
    """Slices that are multiples of one another (the width-1 group; slices scaled by 2 or negated): s = sqrt(q q' - k^2) is
    rounding noise of size <= sqrt(u) sqrt(q q') and reaches dK'/dk and dK'/dq at first order, (1/2pi + 2/4pi) sqrt(2^-53) =
    3.4e-9 of the entry per hidden layer at worst.  Gate: (1e-8 + 3.4e-9 (n_dense - 1)) max half.
    Measured on the MI355X: 4.6e-11 (n_dense = 2) and 2.5e-10 (n_dense = 3) of the max half."""
    x, y = _rows("synth", 192, 7)
    x = x.copy()
    x[100:140, 0:2] = 2.0 * x[0:40, 0:2]
    x[140:180, 0:2] = -x[40:80, 0:2]
    x[100:140, 3:7] = -x[20:60, 3:7]
    x[150:190, 1:5] = 2.0 * x[60:100, 1:5]
    weights = [0.5, 1.0, 0.7, 0.4, 1.3]
    net = _net(n_dense, 1.2, 0.0)
    v, c = R.variances(net[0], net[1])
    ref = AM.Oracle(x, y, GROUPS7).full(v, c, list(net[2]), 1e-3, weights)
    m = additive_mll.AdditiveMarginalLikelihood(192, 7, GROUPS7).set_train(x, y)
    nlml, g, gw = m.evaluate(net, 1e-3, weights=weights)
    _check(m, nlml, g, gw, ref, extra=3.4e-9 * (n_dense - 1), label="collinear nd=%d" % n_dense)
    m.close()


def test_only_width_1_groups_without_biases():
    """130 width-1 groups with b_std = 0: EVERY group entry has q q' - k^2 = 0 in exact arithmetic, in every layer, so nothing
    dilutes the noise of s, and d/dsigma_b,0^2 takes it through dK'/dq = s / (4 pi q) with sqrt(q'/q) as large as the rows make
    it.  Same derived gate.  Measured on the MI355X: 8.2e-9 of the max half (the sigma_b,0^2 component; every other one is below
    1e-12)."""
    net = _net(2, 1.0, 0.0)
    d, groups, weights = _table("d130_width1")
    x, y = _rows("synth", 127, d)
    ref = _reference("synth", 127, "d130_width1", net, 1e-3, False)
    m = additive_mll.AdditiveMarginalLikelihood(127, d, groups).set_train(x, y)
    nlml, g, gw = m.evaluate(net, 1e-3, weights=weights)
    _check(m, nlml, g, gw, ref, extra=3.4e-9, label="130 width-1 groups, b_std = 0")
    m.close()


def test_device_gradient_against_finite_differences_of_the_device_nlml():
    """Every weight against differences of the device's own NLML, to 1e-6 max half: five-point central differences at 1e-3 w_t,
    and at the zero weight the five-point forward difference (error h^4 f^(5) / 5) at h = 1e-3, the central step at w = 1.  (A
    group that enters an evidence without it changes the NLML over a few hundredths of its weight: at h = 1e-2 the forward
    difference itself is 2e-5 of the half away.)"""
    x, y = _rows("synth", 192, 7)
    net = _net(3, 1.2, 0.05)
    m = additive_mll.AdditiveMarginalLikelihood(192, 7, GROUPS7).set_train(x, y)
    _, _, gw = m.evaluate(net, 1e-3, weights=WEIGHTS7)
    ta = m.additive_terms()
    for t in range(5):
        def f(s, t=t):
            ww = list(WEIGHTS7)
            ww[t] = s
            return m.evaluate(net, 1e-3, with_grad=False, weights=ww)[0]

        w = WEIGHTS7[t]
        if w == 0.0:
            h = 1e-3
            fd = (-25 * f(0.0) + 48 * f(h) - 36 * f(2 * h) + 16 * f(3 * h) - 3 * f(4 * h)) / (12 * h)
        else:
            h = 1e-3 * w
            fd = (-f(w + 2 * h) + 8 * f(w + h) - 8 * f(w - h) + f(w - 2 * h)) / (12 * h)
        scale = max(abs(ta["half1"][t]), abs(ta["half2"][t]))
        print("weight %d: fd %.10e device %.10e distance / max half %.2e" % (t, fd, gw[t], abs(fd - gw[t]) / scale))
        assert abs(fd - gw[t]) <= 1e-6 * scale, (t, fd, gw[t], scale)
    m.close()


def test_bit_conditions():
    lib = _lib.load()
    x, y = _rows("unit", 130, 20)
    net = _net(3, 1.2, 0.05)
    plain = mll.NNGPMarginalLikelihood(130, 20).set_train(x, y)
    nlml_p, g_p = plain.evaluate(net, 1e-3)
    # n_groups = 0 and w0 = 1: the bits of nngp_mll_evaluate, NLML and gradient
    m0 = additive_mll.AdditiveMarginalLikelihood(130, 20, []).set_train(x, y)
    nlml0, g0, gw0 = m0.evaluate(net, 1e-3, weights=[1.0])
    assert nlml0 == nlml_p and np.array_equal(g0, g_p)
    assert np.array_equal(m0.terms()["quad"], plain.terms()["quad"]) and np.array_equal(m0.terms()["trace"], plain.terms()["trace"])
    m0.close()
    # a handle with a reserved table: nngp_mll_evaluate and nngp_mll_loo_evaluate return the bits they returned before, before
    # and after an additive evaluation; no device allocation after reserve
    _, groups, weights = _table("pairs20")
    m = additive_mll.AdditiveMarginalLikelihood(130, 20, groups).set_train(x, y)
    count = lib.nngp_alloc_count()
    for _ in range(2):
        nlml_q, g_q = mll.NNGPMarginalLikelihood.evaluate(m, net, 1e-3)
        assert nlml_q == nlml_p and np.array_equal(g_q, g_p)
        first = m.evaluate(net, 1e-3, weights=weights)
    # repeats, and the NLML alone
    again = m.evaluate(net, 1e-3, weights=weights)
    assert again[0] == first[0] and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    assert m.evaluate(net, 1e-3, with_grad=False, weights=weights)[0] == first[0]
    assert lib.nngp_alloc_count() == count
    m.close()
    lo = loo.LeaveOneOut(130, 20).set_train(x, y)
    val_p, gl_p = lo.evaluate(net, 1e-3)
    table = _lib.make_groups(groups, [1.0] * 10, 1.0)
    assert lib.nngp_mll_reserve_additive(lo._h, ctypes.byref(table)) == 0
    val_q, gl_q = lo.evaluate(net, 1e-3)
    assert val_q == val_p and np.array_equal(gl_q, gl_p)
    lo.close()
    plain.close()
    # a zero-weight group leaves the NLML's bits where they are without it (and still has a derivative)
    x7, y7 = _rows("synth", 192, 7)
    a = additive_mll.AdditiveMarginalLikelihood(192, 7, GROUPS7).set_train(x7, y7)
    b = additive_mll.AdditiveMarginalLikelihood(192, 7, GROUPS7[:2] + GROUPS7[3:]).set_train(x7, y7)
    na, ga, gwa = a.evaluate(net, 1e-3, weights=WEIGHTS7)
    nb, gb, gwb = b.evaluate(net, 1e-3, weights=WEIGHTS7[:3] + WEIGHTS7[4:])
    assert na == nb and np.array_equal(ga, gb) and np.array_equal(np.delete(gwa, 3), gwb) and gwa[3] != 0.0
    a.close()
    b.close()


def test_gauge_identity_on_device_results():
    """sum_t w_t dNLML/dw_t = v_last dNLML/dv_last + c_last dNLML/dc_last, within the sum of the gates of the components involved."""
    x, y = _rows("synth", 192, 7)
    for net in (_net(3, 1.2, 0.05), _net(2, 1.0, 0.0)):
        nd = len(net[0])
        v, c = R.variances(net[0], net[1])
        m = additive_mll.AdditiveMarginalLikelihood(192, 7, GROUPS7).set_train(x, y)
        _, g, gw = m.evaluate(net, 1e-3, weights=WEIGHTS7)
        t, ta = m.terms(), m.additive_terms()
        wt = np.asarray(WEIGHTS7)
        lhs = float(np.sum(wt * gw))
        rhs = v[-1] * g[2 * nd - 2] + c[-1] * g[2 * nd - 1]
        half = np.maximum(np.abs(t["quad"]), np.abs(t["trace"]))
        gate = 1e-8 * (np.sum(wt * np.maximum(np.abs(ta["half1"]), np.abs(ta["half2"]))) + v[-1] * half[2 * nd - 2]
                       + c[-1] * half[2 * nd - 1])
        print("gauge: |lhs - rhs| / gate = %.2e" % (abs(lhs - rhs) / gate))
        assert abs(lhs - rhs) <= gate, (lhs, rhs, gate)
        m.close()


def test_errors():
    lib = _lib.load()
    x, y = _rows("synth", 130, 7)
    net = _net(2, 1.0, 0.0)
    arch = _lib.make_arch_act(net[0], net[1], net[2])
    out = ctypes.c_double()
    five = (ctypes.c_double * 5)(*WEIGHTS7)

    def message():
        return lib.nngp_last_error().decode()

    # evaluate before reserve
    plain = mll.NNGPMarginalLikelihood(130, 7).set_train(x, y)
    assert lib.nngp_mll_evaluate_additive(plain._h, ctypes.byref(arch), five, 1e-3, 0, ctypes.byref(out), None, None,
                                          _lib.stream_ptr()) == -2
    assert "nngp_mll_reserve_additive first" in message()
    # a bad table
    for groups, text in (([(0, 9)], "outside 0 <= begin < end <= d"), ([(3, 3)], "outside 0 <= begin < end <= d")):
        table = _lib.make_groups(groups, [1.0], 1.0)
        assert lib.nngp_mll_reserve_additive(plain._h, ctypes.byref(table)) == -2
        assert text in message()
    table = _lib.make_groups([], [], 1.0)
    table.n_groups = _lib.MAX_GROUPS + 1
    assert lib.nngp_mll_reserve_additive(plain._h, ctypes.byref(table)) == -2 and "n_groups" in message()
    assert lib.nngp_mll_reserve_additive(plain._h, None) == -2 and "NULL" in message()
    plain.close()
    # weights
    m = additive_mll.AdditiveMarginalLikelihood(130, 7, GROUPS7).set_train(x, y)
    for bad, text in (([0.5, -1.0, 1.0, 1.0, 1.0], "weight 1 must be finite and >= 0"),
                      ([float("nan"), 1.0, 1.0, 1.0, 1.0], "weight 0 must be finite and >= 0"),
                      ([1.0, 1.0, float("inf"), 1.0, 1.0], "weight 2 must be finite and >= 0"),
                      ([0.0] * 5, "all weights are zero")):
        with pytest.raises(_lib.NngpError, match=text):
            m.evaluate(net, 1e-3, weights=bad)
    # an Erf layer; the handle stays usable
    erf = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])
    assert lib.nngp_mll_evaluate_additive(m._h, ctypes.byref(erf), five, 1e-3, 0, ctypes.byref(out), None, None,
                                          _lib.stream_ptr()) == -2
    assert "Erf" in message()
    with pytest.raises(_lib.NngpError, match="no evaluation with grad_w"):
        m.additive_terms()
    assert np.isfinite(m.evaluate(net, 1e-3, weights=WEIGHTS7)[0])
    # relevances together with groups, either way round
    assert lib.nngp_mll_reserve_ard(m._h) == -2 and "relevances together with groups" in message()
    m.close()
    ard = mll.NNGPMarginalLikelihood(130, 7, ard=True)
    table = _lib.make_groups(GROUPS7, [1.0] * 4, 1.0)
    assert lib.nngp_mll_reserve_additive(ard._h, ctypes.byref(table)) == -2 and "relevances together with groups" in message()
    ard.close()
    # the Python layer
    m = additive_mll.AdditiveMarginalLikelihood(130, 7, GROUPS7).set_train(x, y)
    with pytest.raises(ValueError, match="5 values"):
        m.evaluate(net, 1e-3, weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="weights are needed"):
        m.evaluate(net, 1e-3)
    _, _, other = stax.additive((stax.Dense(8), stax.Relu(), stax.Dense(1)), [(0, 3)])
    with pytest.raises(ValueError, match="not the ones reserved"):
        m.evaluate(other, 1e-3)
    m.close()
    with pytest.raises(ValueError):
        additive_mll.AdditiveMarginalLikelihood(130, 7, "pairs")  # d = 7 is odd
    _, _, kf = stax.additive((stax.Dense(8), stax.Relu(), stax.Dense(1)), GROUPS7, WEIGHTS7[1:], WEIGHTS7[0])
    with pytest.raises(ValueError, match="additive"):
        mll.marginal_likelihood(kf, x, y)
    # and the one-shot function is the handle's evaluation
    nlml, gd = additive_mll.marginal_likelihood(kf, x, y)
    ref = _reference("synth", 130, "d7", net, 1e-3, False)
    assert _rel(nlml, ref["nlml"]) <= 1e-9 and set(gd) == {"w_std2", "b_std2", "diag_reg", "full_weight", "group_weights"}
    size_w = np.maximum(np.abs(ref["half1_w"]), np.abs(ref["half2_w"]))
    assert np.all(np.abs(np.array([gd["full_weight"]] + gd["group_weights"]) - ref["grad_w"]) <= 1e-8 * size_w)
    assert additive_mll.marginal_likelihood(kf, x, y, with_grad=False) == nlml


def test_tuner_matches_the_oracle_driven_run_and_the_posterior():
    g = np.load(os.path.join(GOLDEN, "forest_n256_m64.npz"))
    x, y, xt = g["X_train"].astype(np.float64), g["Y_train"], g["X_test"].astype(np.float64)
    _, _, kf = stax.additive((stax.Dense(512), stax.Relu(), stax.Dense(1)), "pairs")
    printed = []
    kf_t, lam_t, hist = additive_mll.tune_hyperparameters(kf, x, y, steps=10, lr=0.05, report=printed.append)
    kf_o, lam_o, hist_o = additive_mll.tune_hyperparameters(kf, x, y, steps=10, lr=0.05, report=None,
                                                            evaluator=AM.Oracle(x, y, _pairs(20)))
    np.testing.assert_allclose(kf_t.w_std, kf_o.w_std, rtol=1e-8)
    np.testing.assert_allclose(kf_t.group_weights, kf_o.group_weights, rtol=1e-8)
    assert _rel(kf_t.full_weight, kf_o.full_weight) <= 1e-8 and _rel(lam_t, lam_o) <= 1e-8
    np.testing.assert_allclose(hist, hist_o, rtol=1e-9)
    assert all(b < a for a, b in zip(hist, hist[1:])) and hist[0] < 1391.58
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, v) for i, v in enumerate(hist)]
    assert kf_t.w_std[-1] == 1.0 and kf_t.groups == tuple(_pairs(20))
    # the tuned kernel through the posterior, against the reference posterior at the tuned values
    mean, _ = predict.gradient_descent_mse_ensemble(kf_t, x, y, diag_reg=lam_t)(x_test=xt, get="nngp", compute_cov="diag")
    ref = AR.Posterior(x, y, list(kf_t.w_std), list(kf_t.b_std), None, _pairs(20), list(kf_t.group_weights), kf_t.full_weight,
                       diag_reg=lam_t).predict(xt, "nngp", False)
    l2, elem = G.mean_gate(mean, ref)
    print("tuned posterior mean gate", l2, elem)
    assert l2 <= 1e-4 and elem <= 1e-4, (l2, elem)


def test_train_cli_tune_additive_on_forest_queries(tmp_path):
    g = np.load(os.path.join(GOLDEN, "forest_queries.npz"))
    g = {k: g[k] for k in g.files}
    sent = np.iinfo(np.int32).min
    names = "ABCDEFGHIJ"
    per_file = 2000
    for fi, fn in enumerate(g["files"]):
        with open(tmp_path / str(fn), "w") as fh:
            for i in range(fi * per_file, (fi + 1) * per_file):
                preds = ["%s,%d,%d" % (names[c], g["bounds"][i, c, 0], g["bounds"][i, c, 1]) for c in range(10)
                         if g["bounds"][i, c, 0] != sent]
                fh.write("#".join(preds) + "@%d\n" % g["cards"][i])
    args = train_cli.parse_args(["--kernel_type", "nngp", "--query_path", str(tmp_path), "--max_num_train", "1000",
                                 "--max_num_test", "200", "--tune_hyper", "5", "--additive", "pairs", "--tune_additive"])
    args.join_query = False
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    text = buf.getvalue()
    steps = [float(line.split(":")[-1]) for line in text.splitlines() if line.startswith("Step:")]
    assert len(steps) == 5 and all(b < a for a, b in zip(steps, steps[1:])), steps
    for needle in ("Tuned W_std", "Tuned weights: full=", "Kernel construction in", "Mean Square Error:",
                   "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    assert np.all(np.isfinite(res["pred_mean"]))
    mse = float(text.split("Mean Square Error:")[1].split()[0]) / 200.0  # the CLI prints the sum of squares
    print("NLML per step", steps, "final MSE %.4f (untuned pairs + full: 4.134)" % mse)
    print([line for line in text.splitlines() if line.startswith("Tuned")])
