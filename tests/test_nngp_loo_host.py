"""CPU tests of leave-one-out cross-validation: the NumPy oracle (nngp_loo_reference.py) against brute-force refits, finite
differences and a long-double referee; loo.tune_hyperparameters driven by the oracle; what is refused without a GPU; the
CLI flags."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_loo_reference as L  # noqa: E402
import nngp_mll_reference as R  # noqa: E402
import nngp_oracle as oracle  # noqa: E402
from nngp_src_amd import _lib, loo, mll, stax, train as train_cli  # noqa: E402

RELU = ([1.0, 1.0], [0.0, 0.0], [("relu",)])
LEAKY = ([1.2, 0.9, 1.1], [0.05, 0.1, 0.0], [("abrelu", 0.1, 1.0), ("relu",)])


def _forest_rows(golden_dir, n):
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    return g["X_train"][:n] / 1000.0, g["Y_train"][:n].reshape(-1)


@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("net", [RELU, LEAKY], ids=["relu", "leaky_relu"])
@pytest.mark.parametrize("n", [200, 400])
def test_closed_form_equals_the_refit_without_each_point(golden_dir, n, net, absolute):
    """r held at its full-data value: the closed form IS the refit, at every point -- duplicated and zero rows included (a
    duplicate's partner stays in the refit, so its LOO variance is small, not singular: r > 0)."""
    x, y = _forest_rows(golden_dir, n)
    x[5] = 0.0
    x[77] = 0.0
    x[150:160] = x[20:30]
    w, b, acts = net
    lam = 1e-3 if not absolute else 1e-2
    o = L.Oracle(x, y)
    ref = o.full(*R.variances(w, b), acts, lam, absolute, with_grad=False)
    mean, var = o.brute_force(*R.variances(w, b), acts, lam, absolute)
    # both sides solve systems of condition ~1e5 in float64: 1e-9 is four orders above what they reach (1e-13 measured)
    assert np.linalg.norm(mean - ref["mean"]) <= 1e-9 * np.linalg.norm(ref["mean"])
    assert np.linalg.norm(var - ref["var"]) <= 1e-9 * np.linalg.norm(ref["var"])
    full = o.full(*R.variances(w, b), acts, lam, absolute)  # b from A^-1's diagonal instead of the rows of L^-1
    assert np.linalg.norm(full["var"] - ref["var"]) <= 1e-9 * np.linalg.norm(ref["var"])
    assert abs(full["value"] - ref["value"]) <= 1e-9 * abs(ref["value"])


@pytest.mark.parametrize("objective", L.OBJECTIVES)
@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("net", [RELU, LEAKY], ids=["relu", "leaky_relu"])
def test_oracle_gradient_against_finite_differences(golden_dir, net, absolute, objective):
    x, y = _forest_rows(golden_dir, 150)
    w, b, acts = net
    v, c = R.variances(w, b)
    lam = 1e-2
    o = L.Oracle(x, y, objective)
    ref = o.full(v, c, acts, lam, absolute)
    np.testing.assert_allclose(ref["grad"], -(ref["half1"] + ref["half2"]), rtol=0, atol=0)
    for p in range(2 * len(w) + 1):
        base = (v[p // 2] if p % 2 == 0 else c[p // 2]) if p < 2 * len(w) else lam
        if base == 0.0:
            continue  # one-sided at a zero bias
        h = 1e-3 * base

        def f(dt):
            vv, cc, ll = list(v), list(c), lam
            if p == 2 * len(w):
                ll += dt
            elif p % 2 == 0:
                vv[p // 2] += dt
            else:
                cc[p // 2] += dt
            return o.value_var(vv, cc, acts, ll, absolute)

        fd = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        scale = max(abs(ref["half1"][p]), abs(ref["half2"][p]))
        # 4-point differences of a value good to ~cond eps: 1e-6 of the halves' scale (1e-8 measured)
        assert abs(fd - ref["grad"][p]) <= 1e-6 * scale, (p, fd, ref["grad"][p], scale)


def test_closed_form_against_the_long_double_referee(golden_dir):
    """N = 400, one ReLU layer, relative diag_reg 1e-3 (cond 3e5).  Measured here: residuals 2.1e-12 (relative norm), variances
    1.4e-13, mse 3.9e-14, nlpd 4.4e-14 (the issue's own NumPy evaluation measured 1.4e-12, 1.1e-12 and 8e-14); the gates are
    the float64 floor cond * eps = 7e-11 rounded up to 1e-10."""
    x, y = _forest_rows(golden_dir, 400)
    w, b, acts = RELU
    o = L.Oracle(x, y)
    ref = o.full(*R.variances(w, b), acts, 1e-3, with_grad=False)
    ld = o.long_double(*R.variances(w, b), acts, 1e-3)
    assert 1e5 < ld["cond"] < 1e6
    e_r = np.linalg.norm(ref["resid"] - ld["resid"]) / np.linalg.norm(ld["resid"])
    e_v = np.linalg.norm(ref["var"] - ld["var"]) / np.linalg.norm(ld["var"])
    e_m, e_n = abs(ref["mse"] - ld["mse"]) / ld["mse"], abs(ref["nlpd"] - ld["nlpd"]) / abs(ld["nlpd"])
    print("residuals %.2e variances %.2e mse %.2e nlpd %.2e cond %.2e" % (e_r, e_v, e_m, e_n, ld["cond"]))
    assert max(e_r, e_v, e_m, e_n) <= 1e-10


def test_ntk_kernel_of_the_oracle(golden_dir):
    x, _ = _forest_rows(golden_dir, 120)
    w, b = (1.5, 1.2, 0.9), (0.05, 0.1, 0.02)
    t = L.ntk_kernel(x, *R.variances(w, b), [("relu",), ("relu",)])
    ref = oracle.kernel_fn(x, None, "ntk", oracle.Arch(w, b))
    off = ~np.eye(120, dtype=bool)
    np.testing.assert_allclose(t[off], ref[off], rtol=1e-12)
    _, td = oracle.diag_kernel(np.sum(x * x, axis=1) / x.shape[1], oracle.Arch(w, b))
    np.testing.assert_allclose(np.diag(t), td, rtol=1e-14)


@pytest.mark.parametrize("objective", L.OBJECTIVES)
def test_tune_hyperparameters_with_the_oracle_lowers_the_objective(golden_dir, objective):
    x, y = _forest_rows(golden_dir, 300)
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.0, b_std=0.0), stax.Relu(), stax.Dense(1, W_std=1.0, b_std=0.0))
    printed = []
    o = L.Oracle(x, y, objective)
    start = o.evaluate(([1.0, 1.0], [0.05, 0.05], [("relu",)]), 1e-3, False, False)[0]
    kf_t, lam, hist = loo.tune_hyperparameters(kf, x, y, steps=8, lr=0.05, b_std_init=0.05, report=printed.append, evaluator=o,
                                               objective=objective)
    assert len(hist) == 8 and hist[-1] < hist[0] < start
    assert printed == ["Step: %d, LOO %s: %f" % (i, objective, v) for i, v in enumerate(hist)]
    assert lam > 0 and len(kf_t.w_std) == 2 and all(v > 0 for v in kf_t.b_std)
    assert [tuple(a) for a in kf_t.activations] == [("relu",)]
    end = o.evaluate((kf_t.w_std, kf_t.b_std, kf_t.activations), lam, False, False)[0]
    assert abs(end - hist[-1]) <= 1e-9 * abs(end)  # the returned kernel_fn is the tuned point
    # the marginal-likelihood loop and its report are untouched
    printed = []
    mll.tune_hyperparameters(kf, x, y, steps=2, b_std_init=0.05, report=printed.append, evaluator=R.Oracle(x, y))
    assert all(s.startswith("Step: %d, neg marginal likelihood: " % i) for i, s in enumerate(printed)) and len(printed) == 2


def test_refusals_raise_before_any_gpu_call(golden_dir):
    x, y = _forest_rows(golden_dir, 50)
    _, _, kf = stax.serial(stax.Dense(8), stax.Relu(), stax.Dense(1))
    _, _, kf_erf = stax.serial(stax.Dense(8), stax.Erf(), stax.Dense(1))
    with pytest.raises(ValueError, match="Erf"):
        loo.loo_predict(kf_erf, x, y)
    with pytest.raises(ValueError, match="Erf"):
        loo.loo_objective(kf_erf, x, y, objective="mse")
    with pytest.raises(ValueError, match="Erf"):
        loo.tune_hyperparameters(kf_erf, x, y, evaluator=L.Oracle(x, y))
    with pytest.raises(ValueError, match="nlpd"):
        loo.loo_objective(kf, x, y, objective="nlpd", with_grad=False, get="ntk")
    with pytest.raises(ValueError, match="gradient"):
        loo.loo_objective(kf, x, y, objective="mse", with_grad=True, get="ntk")
    with pytest.raises(ValueError):
        loo.loo_objective(kf, x, y, objective="rmse")
    with pytest.raises(ValueError):
        loo.loo_predict(kf, x, y, get="gp")
    with pytest.raises(ValueError):
        loo.tune_hyperparameters(kf, x, y, objective="mll", evaluator=L.Oracle(x, y))
    with pytest.raises(ValueError):
        loo.loo_predict(kf, x, np.stack([y, y], 1))
    with pytest.raises(ValueError):
        loo.LeaveOneOut(50, x.shape[1], "nlpd", "ntk")
    assert loo.check_supported(kf, "ntk", "mse", False)[0] == [1.0, 1.0]


def test_abi_symbols_and_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nngp_loo.h")).read()
    for name in _lib.LOO_ABI_SYMBOLS:
        assert "int %s(" % name in header, name
    assert "#define NNGP_LOO_NLPD %d" % _lib.LOO_NLPD in header and "#define NNGP_LOO_MSE %d" % _lib.LOO_MSE in header
    assert loo.OBJECTIVES == {"nlpd": _lib.LOO_NLPD, "mse": _lib.LOO_MSE}
    assert loo.LeaveOneOut._prefix == mll.NNGPMarginalLikelihood._prefix == "nngp_mll_"


def test_cli_flags():
    p = train_cli.make_parser()
    a = p.parse_args([])
    assert a.loo is False and a.tune_objective == "mll" and a.tune_hyper == 0
    a = p.parse_args(["--loo", "--tune_hyper", "3", "--tune_objective", "loo_mse"])
    assert a.loo is True and a.tune_objective == "loo_mse"
    with pytest.raises(SystemExit):
        p.parse_args(["--tune_objective", "loo"])
    bad = p.parse_args(["--kernel_type", "ntk", "--tune_hyper", "2", "--tune_objective", "loo_nlpd"])
    bad.join_query = False
    with pytest.raises(ValueError):
        train_cli.main(bad)
