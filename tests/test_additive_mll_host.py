"""The additive kernel's marginal likelihood without a GPU (include/nngp_additive_mll.h, nngp-src_amd/additive_mll.py): the NumPy
oracle against finite differences of its own NLML, the gauge identity, the oracle without groups, the raw vector of the tuner, a
tuning run driven by the oracle, the header's symbols and the command line."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import additive_mll_reference as AM  # noqa: E402
import nngp_mll_reference as R  # noqa: E402
from nngp_src_amd import _lib, additive_mll, loo, mll, stax, synth, train  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

GROUPS7 = [(0, 2), (2, 3), (3, 7), (1, 5)]     # a width-1 group, an overlap
WEIGHTS7 = [0.5, 1.0, 0.7, 0.0, 1.3]           # w0 = 0.5; group (3, 7) has weight 0
NET3 = ([1.2, 0.9, 1.1], [0.01, 0.0, 0.04], [("relu",), ("abrelu", 0.1, 1.0)])


def _synth7(n=160):
    x, y = synth.synthetic_queries(n, 8, seed=5)
    return x[:, :7] / 1000.0, y.reshape(-1)


def _forest_raw(n=160):
    g = np.load(os.path.join(GOLDEN, "forest_n1000_m200.npz"))
    return g["X_train"][:n].astype(np.float64), g["Y_train"][:n].reshape(-1)


def _pairs(d):
    return list(_lib.pair_groups(d))


def _fd(f, base, h):
    """Central difference of f at base; at base == 0 the one-sided three-point difference (the parameter is >= 0), at a tenth
    of the step: its truncation error is h^2 f''' / 3 against the central one's h^2 f''' / 6, and a bias variance at 0 sits
    where the NLML bends most (the rank-one term c 1 1^T saturates once c passes 1 / (1^T A^-1 1))."""
    if base == 0.0:
        h = 0.1 * h
        return (-3.0 * f(0.0) + 4.0 * f(h) - f(2.0 * h)) / (2.0 * h)
    return (f(base + h) - f(base - h)) / (2.0 * h)


def _check_against_finite_differences(x, y, groups, net, weights, lam, step_w, step_v):
    w, b, acts = net
    v, c = R.variances(w, b)
    o = AM.Oracle(x, y, groups)
    f = o.full(v, c, acts, lam, weights)
    assert np.all(np.isfinite(f["grad"])) and np.all(np.isfinite(f["grad_w"]))
    worst = 0.0
    for p in range(2 * len(v) + 1):
        def val(t, p=p):
            vv, cc, ll = list(v), list(c), lam
            if p == 2 * len(v):
                ll = t
            elif p % 2 == 0:
                vv[p // 2] = t
            else:
                cc[p // 2] = t
            return o.nlml_var(vv, cc, acts, ll, weights)

        base = lam if p == 2 * len(v) else (v[p // 2] if p % 2 == 0 else c[p // 2])
        h = step_v * (lam if p == 2 * len(v) else 1.0)
        fd = _fd(val, base, h)
        scale = max(abs(f["quad"][p]), abs(f["trace"][p]))
        worst = max(worst, abs(fd - f["grad"][p]) / scale)
        assert abs(fd - f["grad"][p]) <= 1e-6 * scale, ("theta", p, fd, f["grad"][p], scale)
    for t in range(len(weights)):
        def val(s, t=t):
            ww = list(weights)
            ww[t] = s
            return o.nlml_var(v, c, acts, lam, ww)

        fd = _fd(val, weights[t], step_w)
        scale = max(abs(f["half1_w"][t]), abs(f["half2_w"][t]))
        worst = max(worst, abs(fd - f["grad_w"][t]) / scale)
        assert abs(fd - f["grad_w"][t]) <= 1e-6 * scale, ("weight", t, fd, f["grad_w"][t], scale)
    return f, worst


def test_oracle_against_finite_differences_of_its_own_nlml():
    """Every component -- layer variances, lambda, every weight; one-sided at the zero weight and at b = 0 -- within
    1e-6 max(|half1|, |half2|).  Steps: 1e-5 for weights, 1e-6 for variances (lambda: 1e-6 of itself)."""
    x, y = _synth7()
    f, worst = _check_against_finite_differences(x, y, GROUPS7, NET3, WEIGHTS7, 1e-3, 1e-5, 1e-6)
    print("worst distance / max half:", worst)
    assert f["grad_w"][3] != 0.0  # the zero-weight group has its own derivative


def test_oracle_against_finite_differences_on_raw_forest_rows_with_pairs():
    """160 raw forest rows, pairs + the whole input: identical default slices off the diagonal (the identical-slice rule).
    The rows are of size 1e3, so q is of size 1e5 .. 1e6: the bias variances are stepped at that scale (1e-6 q), the others as
    above."""
    x, y = _forest_raw()
    groups = _pairs(20)
    xs = x[:, 0:2]
    assert np.sum(np.all(xs[:, None, :] == xs[None, :, :], axis=2)) > x.shape[0]  # identical slices off the diagonal
    net = ([1.1, 0.9], [30.0, 0.0], [("relu",)])
    weights = [1.0] * 11
    w, b, acts = net
    v, c = R.variances(w, b)
    o = AM.Oracle(x, y, groups)
    f = o.full(v, c, acts, 1e-3, weights)
    qbar = float(np.mean(np.sum(x * x, axis=1)) / x.shape[1])
    for p in range(5):
        def val(t, p=p):
            vv, cc, ll = list(v), list(c), 1e-3
            if p == 4:
                ll = t
            elif p % 2 == 0:
                vv[p // 2] = t
            else:
                cc[p // 2] = t
            return o.nlml_var(vv, cc, acts, ll, weights)

        base = 1e-3 if p == 4 else (v[p // 2] if p % 2 == 0 else c[p // 2])
        h = 1e-9 if p == 4 else (1e-6 if p % 2 == 0 else 1e-6 * qbar)
        fd = _fd(val, base, h)
        scale = max(abs(f["quad"][p]), abs(f["trace"][p]))
        assert abs(fd - f["grad"][p]) <= 1e-6 * scale, ("theta", p, fd, f["grad"][p], scale)
    for t in range(11):
        def val(s, t=t):
            ww = list(weights)
            ww[t] = s
            return o.nlml_var(v, c, acts, 1e-3, ww)

        fd = _fd(val, 1.0, 1e-5)
        scale = max(abs(f["half1_w"][t]), abs(f["half2_w"][t]))
        assert abs(fd - f["grad_w"][t]) <= 1e-6 * scale, ("weight", t, fd, f["grad_w"][t], scale)


def _gauge(f, v, c, weights):
    """Both sides of sum_t w_t dNLML/dw_t = v_last dNLML/dv_last + c_last dNLML/dc_last, and the size of the halves they cancel from."""
    nd = len(v)
    weights = np.asarray(weights)
    lhs = float(np.sum(weights * f["grad_w"]))
    rhs = v[-1] * f["grad"][2 * nd - 2] + c[-1] * f["grad"][2 * nd - 1]
    size = float(np.sum(weights * np.maximum(np.abs(f["half1_w"]), np.abs(f["half2_w"]))))
    return lhs, rhs, size


@pytest.mark.parametrize("absolute", [False, True])
def test_gauge_identity(absolute):
    x, y = _synth7()
    w, b, acts = NET3
    v, c = R.variances(w, b)
    f = AM.Oracle(x, y, GROUPS7).full(v, c, acts, 1e-3, WEIGHTS7, absolute)
    lhs, rhs, size = _gauge(f, v, c, WEIGHTS7)
    print("gauge:", abs(lhs - rhs) / size)
    assert abs(lhs - rhs) <= 1e-12 * size
    # the traces obey it too
    np.testing.assert_allclose(np.sum(np.asarray(WEIGHTS7) * f["tr_k_term"]), f["tr_k"], rtol=1e-13)
    np.testing.assert_allclose(v[-1] * f["tr_dk"][4] + c[-1] * f["tr_dk"][5], f["tr_k"], rtol=1e-13)


def test_without_groups_the_oracle_is_the_plain_one():
    x, y = _synth7()
    w, b, acts = NET3
    v, c = R.variances(w, b)
    plain = R.Oracle(x, y).full(v, c, acts, 1e-3)
    f = AM.Oracle(x, y, []).full(v, c, acts, 1e-3, [1.0])
    assert f["nlml"] == plain["nlml"] and np.array_equal(f["grad"], plain["grad"])
    assert np.array_equal(f["quad"], plain["quad"]) and np.array_equal(f["trace"], plain["trace"])
    # w0 = 2 is the last layer's v and c doubled
    f2 = AM.Oracle(x, y, []).full(v, c, acts, 1e-3, [2.0])
    p2 = R.Oracle(x, y).full(v[:-1] + [2.0 * v[-1]], c[:-1] + [2.0 * c[-1]], acts, 1e-3)
    assert abs(f2["nlml"] - p2["nlml"]) <= 1e-12 * abs(p2["nlml"])
    gate = 1e-12 * np.maximum(np.abs(p2["quad"]), np.abs(p2["trace"]))
    for p in (0, 1, 2, 3, 6):  # the layers before the last, and lambda
        assert abs(f2["grad"][p] - p2["grad"][p]) <= gate[p]
    for p in (4, 5):           # d/dv_last at 2 v_last is half of d/dv_last' at v_last' = 2 v_last ... times 2: chain rule
        assert abs(f2["grad"][p] - 2.0 * p2["grad"][p]) <= 2.0 * gate[p]


def test_params_packing():
    P = additive_mll._Params
    w, b = [1.2, 0.9, 1.1], [0.05, 0.0, 0.04]
    wt = [0.5, 1.0, 0.0, 2.0]
    p = P(w, b, 1e-3, wt)
    # log v_0, log v_1 (the last W_std is fixed), log c_0, log c_2, log w_0, log w_1, log w_3 (the zero weight is fixed), log lambda
    np.testing.assert_allclose(p.raw0, np.log([1.44, 0.81, 0.0025, 0.0016, 0.5, 1.0, 2.0, 1e-3]), rtol=1e-14)
    raw = p.raw0 + np.array([0.1, -0.2, 0.3, 0.0, 0.5, -0.5, 0.25, 0.2])
    ww, bb, lam, clamped = p.unpack(raw)
    np.testing.assert_allclose(ww, [1.2 * np.exp(0.05), 0.9 * np.exp(-0.1), 1.1], rtol=1e-14)
    np.testing.assert_allclose(bb, [0.05 * np.exp(0.15), 0.0, 0.04], rtol=1e-14)
    assert not clamped and abs(lam - 1e-3 * np.exp(0.2)) <= 1e-17
    np.testing.assert_allclose(p.weights(raw), [0.5 * np.exp(0.5), np.exp(-0.5), 0.0, 2.0 * np.exp(0.25)], rtol=1e-14)
    # the chain rule through exp: d/dlog t = t d/dt; the fixed ones have no entry
    g = np.arange(1.0, 8.0)
    g_w = np.array([10.0, 20.0, 30.0, 40.0])
    got = p.grad_raw(g, raw, g_w)
    wts = p.weights(raw)
    want = [g[0] * ww[0] ** 2, g[2] * ww[1] ** 2, g[1] * bb[0] ** 2, g[5] * bb[2] ** 2, 10.0 * wts[0], 20.0 * wts[1], 40.0 * wts[3],
            g[6] * lam]
    np.testing.assert_allclose(got, want, rtol=1e-14)
    # tie_groups: one multiplier for the groups, w0 apart
    t = P(w, b, 1e-3, wt, tie_groups=True)
    assert t.raw0.shape[0] == 4 + 2 + 1 and t.raw0[4] == np.log(0.5) and t.raw0[5] == 0.0
    raw = t.raw0.copy()
    raw[5] = np.log(3.0)
    np.testing.assert_allclose(t.weights(raw), [0.5, 3.0, 0.0, 6.0], rtol=1e-14)
    np.testing.assert_allclose(t.grad_raw(g, raw, g_w)[4:6], [10.0 * 0.5, 20.0 * 3.0 + 40.0 * 6.0], rtol=1e-14)
    # without tune_weights: mll's vector, every W_std free, the weights constant
    n = P(w, b, 1e-3, wt, tune_weights=False)
    np.testing.assert_array_equal(n.raw0, mll._Params(w, b, 1e-3).raw0)
    np.testing.assert_array_equal(n.weights(n.raw0 + 1.0), wt)
    with pytest.raises(ValueError):
        P(w, b, 1e-3, [0.0, 0.0])
    with pytest.raises(ValueError):
        P(w, b, 1e-3, [1.0, -1.0])


def test_oracle_driven_tuner_lowers_the_nlml_at_every_step():
    """forest_n256_m64, pairs + the whole input, one ReLU layer, b_std = 0, 40 steps at lr = 0.05: log sigma_w,0^2, the 11
    log w_t and log lambda are tuned (W_std of the last layer fixed).  Start 1391.58; the run is monotone and ends below 900."""
    g = np.load(os.path.join(GOLDEN, "forest_n256_m64.npz"))
    x, y = g["X_train"].astype(np.float64), g["Y_train"].reshape(-1)  # the rows as they are: the start below is theirs
    _, _, kf = stax.additive((stax.Dense(512), stax.Relu(), stax.Dense(1)), "pairs")
    o = AM.Oracle(x, y, _pairs(20))
    start = o.evaluate((list(kf.w_std), list(kf.b_std), list(kf.activations)), 1e-3, False, False, weights=[1.0] * 11)[0]
    assert abs(start - 1391.58) <= 0.01, start
    kf_t, lam, hist = additive_mll.tune_hyperparameters(kf, x, y, steps=40, lr=0.05, report=None, evaluator=o)
    print("start", start, "end", hist[-1])
    assert len(hist) == 40 and hist[0] < start
    assert all(b < a for a, b in zip(hist, hist[1:])), hist
    assert hist[-1] < 900.0
    assert kf_t.w_std[-1] == 1.0 and kf_t.w_std[0] != 1.0 and kf_t.b_std == (0.0, 0.0)
    assert kf_t.groups == tuple(_pairs(20)) and len(kf_t.group_weights) == 10 and kf_t.full_weight != 1.0
    # what comes back evaluates to the last NLML of the run
    back = o.evaluate((list(kf_t.w_std), list(kf_t.b_std), list(kf_t.activations)), lam, False, False,
                      weights=[kf_t.full_weight] + list(kf_t.group_weights))[0]
    assert abs(back - hist[-1]) <= 1e-9 * abs(hist[-1])


def test_symbols_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_additive_mll.h")) as f:
        declared = set(re.findall(r"\bint (nngp_mll_\w+)\(", f.read()))
    assert declared == set(_lib.ADDITIVE_MLL_ABI_SYMBOLS) and len(declared) == 3
    lib = _lib.load()
    for name in _lib.ADDITIVE_MLL_ABI_SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    # the headers whose symbol sets other tests pin are not extended
    for header, symbols in (("nngp_mll.h", _lib.MLL_ABI_SYMBOLS), ("nngp_ard.h", _lib.ARD_ABI_SYMBOLS)):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert set(re.findall(r"\bint (nngp_mll_\w+)\(", f.read())) == set(symbols)


def test_train_cli_flag(capsys):
    a = train.parse_args([])
    assert a.tune_additive is False
    a = train.parse_args(["--tune_hyper", "5", "--additive", "pairs", "--tune_additive"])
    assert (a.tune_hyper, a.additive, a.tune_additive) == (5, "pairs", True)
    for bad in (["--tune_additive"],                                                        # no --tune_hyper
                ["--tune_additive", "--tune_hyper", "5"],                                   # no --additive pairs
                ["--tune_additive", "--additive", "pairs"],
                ["--tune_additive", "--tune_hyper", "5", "--additive", "pairs", "--kernel_type", "ntk"],
                ["--tune_additive", "--tune_hyper", "5", "--additive", "pairs", "--tune_objective", "loo_nlpd"]):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
        assert "--tune_additive" in capsys.readouterr().err
    text = " ".join(train.make_parser().format_help().split())
    assert "--tune_additive" in text and "(--tune_hyper and --loo work on the plain kernel only)" not in text


def test_what_mll_and_loo_still_refuse():
    _, _, kf = stax.additive((stax.Dense(8), stax.Relu(), stax.Dense(1)), "pairs")
    with pytest.raises(ValueError, match="additive"):
        mll.check_supported(kf)
    with pytest.raises(ValueError, match="additive_mll"):
        mll.marginal_likelihood(kf, np.zeros((4, 4)), np.zeros(4))
    with pytest.raises(ValueError, match="additive"):
        loo.check_supported(kf)
    # and what this module refuses before any GPU call: no groups, relevances with groups, Erf
    _, _, plain = stax.serial(stax.Dense(8), stax.Relu(), stax.Dense(1))
    x, y = np.ones((4, 4)), np.ones(4)
    with pytest.raises(ValueError, match="groups"):
        additive_mll.marginal_likelihood(plain, x, y)
    with pytest.raises(ValueError, match="input_scale"):
        additive_mll.marginal_likelihood(kf.with_input_scale(np.ones(4)), x, y)
    _, _, erf = stax.additive((stax.Dense(8), stax.Erf(), stax.Dense(1)), "pairs")
    with pytest.raises(ValueError, match="Erf"):
        additive_mll.tune_hyperparameters(erf, x, y, steps=1)
    with pytest.raises(ValueError):
        additive_mll.marginal_likelihood(kf, x, np.ones((4, 2)))
