"""Leave-one-out cross-validation on the MI355X (include/nngp_loo.h, nngp-src_amd/loo.py) against the NumPy oracle of
nngp_loo_reference.py (closed form from scipy's Cholesky, gradient by forward-mode tangents).  The gates are those of
test_gpu_nngp_mll.py for this float64 core; the LOO means and variances take the scalar gate, 1e-9 norm-wise (the float64
floor of the closed form is 1e-12, test_nngp_loo_host.py)."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_loo_reference as L  # noqa: E402
import nngp_mll_reference as R  # noqa: E402
import nngp_oracle as oracle  # noqa: E402
from nngp_src_amd import _lib, loo, mll, predict, stax, synth, train as train_cli  # noqa: E402
from test_gpu_nngp_mll import CASES, _forest, _net, _rel, _rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OBJECTIVES = ("nlpd", "mse")


def _nrel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _check_values(m, val, ref):
    print("value rel %.3e" % _rel(val, ref["value"]))
    assert _rel(val, ref["value"]) <= 1e-9, (val, ref["value"])
    mean, var = m.predictions()
    print("mean rel %.3e  var rel %.3e" % (_nrel(mean, ref["mean"]), _nrel(var, ref["var"])))
    assert _nrel(mean, ref["mean"]) <= 1e-9
    assert _nrel(var, ref["var"]) <= 1e-9


def _check(m, val, g, ref):
    _check_values(m, val, ref)
    scale = np.maximum(np.abs(ref["half1"]), np.abs(ref["half2"]))
    print("gradient error / halves' scale", np.abs(g - ref["grad"]) / scale)
    assert np.all(np.abs(g - ref["grad"]) <= 1e-8 * scale), (g, ref["grad"], scale)
    t = m.terms()
    assert _rel(t["tr_k"], ref["tr_k"]) <= 1e-12
    np.testing.assert_allclose(t["tr_dk"], ref["tr_dk"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(-(t["half1"] + t["half2"]), g, rtol=0, atol=0)


def _both_objectives(x, y, w, b, acts, lam, absolute=False, block=512):
    """Both objectives at one point on one handle, each against the oracle; returns the handle."""
    o = L.Oracle(x, y, block=block)
    m = loo.LeaveOneOut(x.shape[0], x.shape[1]).set_train(x, y)
    for obj in OBJECTIVES:
        ref = o.full(*R.variances(w, b), acts, lam, absolute, objective=obj)
        val, g = m.evaluate((w, b, acts), lam, absolute, objective=obj)
        assert np.all(np.isfinite(g))
        _check(m, val, g, ref)
    return m


@pytest.mark.parametrize("n,n_dense,w_std,b_std,absolute,rows", CASES)
def test_objectives_gradient_and_predictions_against_the_oracle(golden_dir, n, n_dense, w_std, b_std, absolute, rows):
    x, y = _rows(golden_dir, rows, n)
    w, b, acts = _net(n_dense, w_std, b_std)
    lam = 1e-3 if not absolute else (1e-3 if rows == "unit" or rows == "synthetic" else 1.0)
    m = _both_objectives(x, y, w, b, acts, lam, absolute)
    # bit-identical repeats; the value alone (no A^-1 product) equals the one returned with the gradient, predictions included
    val, g = m.evaluate((w, b, acts), lam, absolute, objective="mse")
    mean, var = m.predictions()
    val2, g2 = m.evaluate((w, b, acts), lam, absolute, objective="mse")
    assert val2 == val and np.array_equal(g2, g)
    val3, none = m.evaluate((w, b, acts), lam, absolute, with_grad=False, objective="mse")
    assert none is None and val3 == val
    mean3, var3 = m.predictions()
    assert np.array_equal(mean3, mean) and np.array_equal(var3, var)
    m.close()


@pytest.mark.parametrize("act", [("abrelu", 0.1, 1.0), ("abrelu", -1.0, 1.0)])
@pytest.mark.parametrize("b_std", [0.0, 0.05])
def test_leaky_relu_and_abs_networks(golden_dir, act, b_std):
    x, y = _rows(golden_dir, "unit", 1000)
    w, b, acts = _net(3, 1.2, b_std, act)
    _both_objectives(x, y, w, b, acts, 1e-3).close()


def test_zero_and_duplicated_rows(golden_dir):
    x, y = _rows(golden_dir, "unit", 600)
    x[5] = 0.0
    x[77] = 0.0
    x[300:310] = x[100:110]
    w, b, acts = [1.0, 1.3, 1.1], [0.0, 0.05, 0.0], [("relu",), ("abrelu", 0.1, 1.0)]
    _both_objectives(x, y, w, b, acts, 1e-3).close()


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_device_gradient_against_finite_differences_of_the_device_value(golden_dir, objective):
    x, y = _rows(golden_dir, "unit", 1000)
    w, b, acts = [1.2, 0.9, 1.1], [0.05, 0.1, 0.02], [("relu",), ("relu",)]
    m = loo.LeaveOneOut(1000, x.shape[1], objective).set_train(x, y)
    lam = 1e-3
    _, g = m.evaluate((w, b, acts), lam)
    t = m.terms()
    v, c = R.variances(w, b)
    for p in range(2 * len(w) + 1):
        base = (v[p // 2] if p % 2 == 0 else c[p // 2]) if p < 2 * len(w) else lam
        h = 1e-3 * base

        def f(dt):
            vv, cc, ll = list(v), list(c), lam
            if p == 2 * len(w):
                ll += dt
            elif p % 2 == 0:
                vv[p // 2] += dt
            else:
                cc[p // 2] += dt
            return m.evaluate(([np.sqrt(e) for e in vv], [np.sqrt(e) for e in cc], acts), ll, with_grad=False)[0]

        fd = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        scale = max(abs(t["half1"][p]), abs(t["half2"][p]))
        print(p, fd, g[p], abs(fd - g[p]) / scale)
        assert abs(fd - g[p]) <= 1e-6 * scale, (p, fd, g[p], scale)
    m.close()


def test_one_handle_serves_both_and_the_marginal_likelihood_is_unchanged(golden_dir):
    """MLL -> LOO -> MLL on one handle: the identical NLML and gradient; the factor is refused after a LOO gradient (C lies over
    it) and back after an evaluation that keeps it."""
    x, y = _rows(golden_dir, "unit", 1000)
    w, b, acts = _net(3, 1.2, 0.05)
    m = mll.NNGPMarginalLikelihood(1000, x.shape[1]).set_train(x, y)
    nlml, g = m.evaluate((w, b, acts), 1e-3)
    lo = loo.LeaveOneOut.__new__(loo.LeaveOneOut)  # the same device handle through the LOO interface
    lo.__dict__.update(m.__dict__)
    lo.objective, lo.get = "nlpd", "nngp"
    ref = L.Oracle(x, y).full(*R.variances(w, b), acts, 1e-3)
    val, gl = lo.evaluate((w, b, acts), 1e-3)
    _check(lo, val, gl, ref)
    with pytest.raises(_lib.NngpError, match="factor"):
        m.factor()
    nlml2, g2 = m.evaluate((w, b, acts), 1e-3)
    assert nlml2 == nlml and np.array_equal(g2, g)
    assert m.factor().shape[0] == 1024
    lo.evaluate((w, b, acts), 1e-3, with_grad=False)
    assert lo.factor().shape[0] == 1024
    lo._h = None  # one owner
    m.close()


@pytest.mark.parametrize("n_dense,b_std", [(2, 0.0), (3, 0.05)])
def test_ntk_value_and_means_against_the_oracle(golden_dir, n_dense, b_std):
    x, y = _rows(golden_dir, "unit", 1000)
    w, b, acts = _net(n_dense, 1.2, b_std)
    ref = L.Oracle(x, y, "mse", get="ntk").full(*R.variances(w, b), acts, 1e-3, with_grad=False)
    m = loo.LeaveOneOut(1000, x.shape[1], "mse", "ntk").set_train(x, y)
    val, none = m.evaluate((w, b, acts), 1e-3, with_grad=False)
    assert none is None and _rel(val, ref["mse"]) <= 1e-9, (val, ref["mse"])
    mean, var = m.predictions()
    assert var is None and _nrel(mean, ref["mean"]) <= 1e-9
    mean2, var2 = loo.loo_predict(stax.serial(*_layers(w, b))[2], x, y, get="ntk")
    assert var2 is None and np.array_equal(mean2, mean)
    m.close()


def _layers(w, b):
    out = []
    for l in range(len(w)):
        out.append(stax.Dense(1 if l == len(w) - 1 else 512, W_std=w[l], b_std=b[l]))
        if l < len(w) - 1:
            out.append(stax.Relu())
    return out


def test_public_functions(golden_dir):
    x, y = _rows(golden_dir, "unit", 600)
    w, b, acts = _net(2, 1.0, 0.05)
    kf = stax.serial(*_layers(w, b))[2]
    ref = L.Oracle(x, y, "nlpd").full(*R.variances(w, b), acts, 1e-3)
    mean, var = loo.loo_predict(kf, x, y)
    assert _nrel(mean, ref["mean"]) <= 1e-9 and _nrel(var, ref["var"]) <= 1e-9
    val, g = loo.loo_objective(kf, x, y, objective="nlpd")
    assert _rel(val, ref["nlpd"]) <= 1e-9
    assert set(g) == {"w_std2", "b_std2", "diag_reg"} and len(g["w_std2"]) == 2
    assert abs(g["diag_reg"] - ref["grad"][4]) <= 1e-8 * max(abs(ref["half1"][4]), abs(ref["half2"][4]))
    assert _rel(loo.loo_objective(kf, x, y, objective="mse", with_grad=False), ref["mse"]) <= 1e-9


def test_errors(golden_dir):
    lib = _lib.load()
    x, y = _rows(golden_dir, "unit", 300)
    m = loo.LeaveOneOut(300, x.shape[1], "mse")
    # a pivot that is not positive: absolute lambda = 0 with duplicated rows -- names a column; the handle stays usable
    xd = x.copy()
    xd[200:220] = xd[10:30]
    m.set_train(xd, y)
    w, b, acts = _net(2, 1.0, 0.0)
    with pytest.raises(_lib.NngpError, match="column"):
        m.evaluate((w, b, acts), 0.0, absolute=True)
    ref = L.Oracle(xd, y, "mse").full(*R.variances(w, b), acts, 1e-3)
    val, g = m.evaluate((w, b, acts), 1e-3)
    _check(m, val, g, ref)
    out = ctypes.c_double()
    grad = (ctypes.c_double * 5)()

    def rc(arch, get=_lib.GET_NNGP, lam=1e-3, objective=_lib.LOO_MSE, g=None):
        return lib.nngp_mll_loo_evaluate(m._h, ctypes.byref(arch), get, lam, 0, objective, ctypes.byref(out), g, _lib.stream_ptr())

    relu = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("relu",)])
    assert rc(_lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])) == -2
    assert rc(relu, lam=-1e-3) == -2
    assert rc(relu, lam=float("nan")) == -2
    assert rc(relu, get=7) == -2
    assert rc(relu, objective=5) == -2
    assert rc(relu, get=_lib.GET_NTK, g=grad) == -2
    assert rc(relu, get=_lib.GET_NTK, objective=_lib.LOO_NLPD) == -2
    assert b"NTK" in lib.nngp_last_error()
    assert rc(relu, get=_lib.GET_NTK) == 0
    mean = torch.empty(300, dtype=torch.float64, device=DEV)
    assert lib.nngp_mll_loo_predictions(m._h, _lib.ptr(mean), _lib.ptr(mean), _lib.stream_ptr()) == -2  # var after the NTK
    assert lib.nngp_mll_loo_predictions(m._h, _lib.ptr(mean), None, _lib.stream_ptr()) == 0
    assert lib.nngp_mll_loo_terms(m._h, grad, 1) == -2
    m.close()


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_tune_hyperparameters_matches_the_oracle_driven_run_and_the_posterior(golden_dir, objective):
    f = _forest(golden_dir)
    x, y, xt = f["X_train"] / 1000.0, f["Y_train"], f["X_test"] / 1000.0
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.0, b_std=0.05), stax.Relu(), stax.Dense(1, W_std=1.0, b_std=0.05))
    printed = []
    kf_t, lam_t, hist = loo.tune_hyperparameters(kf, x, y, steps=10, lr=0.05, report=printed.append, objective=objective)
    kf_o, lam_o, hist_o = loo.tune_hyperparameters(kf, x, y, steps=10, lr=0.05, report=None, objective=objective,
                                                   evaluator=L.Oracle(x, y, objective))
    np.testing.assert_allclose(kf_t.w_std, kf_o.w_std, rtol=1e-8)
    np.testing.assert_allclose(kf_t.b_std, kf_o.b_std, rtol=1e-8)
    assert _rel(lam_t, lam_o) <= 1e-8
    np.testing.assert_allclose(hist, hist_o, rtol=1e-9)
    assert hist[-1] < hist[0]
    assert printed == ["Step: %d, LOO %s: %f" % (i, objective, v) for i, v in enumerate(hist)]
    # the tuned network through the posterior, against oracle.Posterior at the tuned values
    mean, var = predict.gradient_descent_mse_ensemble(kf_t, x, y, diag_reg=lam_t)(x_test=xt, get="nngp", compute_cov="diag")
    arch = oracle.Arch(tuple(kf_t.w_std), tuple(kf_t.b_std))
    ref_mean, ref_cov = oracle.Posterior(x, y, arch, diag_reg=lam_t).predict(xt, "nngp", True)
    assert np.linalg.norm(mean - ref_mean) / np.linalg.norm(ref_mean) <= 1e-6
    np.testing.assert_allclose(var, np.diag(ref_cov), rtol=1e-5)


def _write_queries(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "forest_queries.npz"))
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


def _run_cli(argv):
    args = train_cli.make_parser().parse_args(argv)
    args.join_query = False
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    return res, buf.getvalue()


@pytest.mark.parametrize("kernel_type", ["nngp", "ntk"])
def test_train_cli_loo_on_forest_queries(golden_dir, tmp_path, kernel_type):
    _write_queries(golden_dir, tmp_path)
    res, text = _run_cli(["--kernel_type", kernel_type, "--query_path", str(tmp_path), "--max_num_train", "1000",
                          "--max_num_test", "200", "--loo"])
    for needle in ("Kernel construction in", "Mean Square Error:", "Predict Result Profile of 200 Queries:",
                   "LOO Mean Square Error:", "Predict Result Profile of 1000 Queries:"):
        assert needle in text, needle
    assert text.index("LOO Mean Square Error:") > text.index("Predict Result Profile of 200 Queries:")
    assert res["loo_errors"].shape == (1000,) and np.all(np.isfinite(res["loo_errors"]))
    assert (res["loo_var"] is None) == (kernel_type == "ntk")


def test_train_cli_tune_objective_on_forest_queries(golden_dir, tmp_path):
    _write_queries(golden_dir, tmp_path)
    res, text = _run_cli(["--kernel_type", "nngp", "--query_path", str(tmp_path), "--max_num_train", "1000", "--max_num_test",
                          "200", "--tune_hyper", "5", "--tune_objective", "loo_nlpd", "--b_std_init", "0.05"])
    for i in range(5):
        assert "Step: %d, LOO nlpd:" % i in text
    assert "neg marginal likelihood" not in text
    for needle in ("Tuned W_std", "Kernel construction in", "Mean Square Error:", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    assert np.all(np.isfinite(res["pred_mean"]))
    with pytest.raises(ValueError):
        _run_cli(["--kernel_type", "ntk", "--query_path", str(tmp_path), "--tune_hyper", "2", "--tune_objective", "loo_mse"])


def test_reference_size():
    """N = 10800, d = 20 (the reference's forest run), one ReLU layer: both objectives, gradient and predictions."""
    x, y = synth.synthetic_queries(10800, 20, seed=7)
    x = x / 1000.0
    y = y.reshape(-1)
    w, b, acts = _net(2, 1.0, 0.0)
    _both_objectives(x, y, w, b, acts, 1e-3, block=1024).close()
