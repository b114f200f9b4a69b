"""NNGP marginal likelihood and its gradient on the MI355X (include/nngp_mll.h, nngp-src_amd/mll.py) against the NumPy
oracle of nngp_mll_reference.py (forward-mode tangents, scipy Cholesky)."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_mll_reference as R  # noqa: E402
import nngp_oracle as oracle  # noqa: E402
from nngp_src_amd import _lib, mll, predict, stax, synth, train as train_cli  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _forest(golden_dir, name="forest_n1000_m200.npz"):
    g = np.load(os.path.join(golden_dir, name))
    return {k: g[k] for k in g.files}


def _rows(golden_dir, kind, n):
    if kind == "synthetic":
        x, y = synth.synthetic_queries(n, 20, seed=n)
        return x / 1000.0, y.reshape(-1)
    f = _forest(golden_dir)
    x = np.concatenate([f["X_train"], f["X_test"]] * 5)[:n]
    y = np.concatenate([f["Y_train"], f["Y_test"]] * 5)[:n].reshape(-1)
    if kind == "centred":  # obtuse angles and mixed signs: the other half of the arctangent's table, in the adjoint pass too
        x = x / 1000.0
        return x - x.mean(0), y
    return (x / 1000.0 if kind == "unit" else x), y


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check(m, o, got_nlml, got_g, ref):
    assert _rel(got_nlml, ref["nlml"]) <= 1e-9, (got_nlml, ref["nlml"])
    gate = 1e-8 * np.maximum(np.abs(ref["quad"]), np.abs(ref["trace"]))
    assert np.all(np.abs(got_g - ref["grad"]) <= gate), (got_g, ref["grad"], gate)
    t = m.terms()
    assert _rel(t["tr_k"], ref["tr_k"]) <= 1e-12
    np.testing.assert_allclose(t["tr_dk"], ref["tr_dk"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(-0.5 * t["quad"] + 0.5 * t["trace"], got_g, rtol=0, atol=0)


def _net(n_dense, w_std, b_std, act=("relu",)):
    return [w_std] * n_dense, [b_std] * n_dense, [act] * (n_dense - 1)


CASES = [  # n, n_dense, W_std, b_std, absolute, rows
    (127, 2, 1.0, 0.0, False, "raw"),
    (127, 4, 1.5, 0.05, True, "unit"),
    (127, 2, 1.5, 0.05, False, "synthetic"),
    (1000, 2, 1.0, 0.0, False, "unit"),
    (1000, 4, 1.0, 0.05, False, "raw"),
    (1000, 4, 1.5, 0.0, True, "synthetic"),
    (1000, 2, 1.5, 0.05, True, "unit"),
    (4097, 2, 1.0, 0.05, False, "unit"),
    (4097, 4, 1.5, 0.0, False, "raw"),
    (4097, 4, 1.0, 0.05, True, "synthetic"),
    (1000, 2, 1.0, 0.0, False, "centred"),
    (1000, 4, 1.5, 0.05, False, "centred"),
    (127, 5, 1.5, 0.05, False, "centred"),   # 5 .. 8 Dense layers: the NLC = 8 instantiation of the adjoint pass
    (127, 9, 1.2, 0.05, True, "unit"),       # 9 .. 16 Dense layers: NLC = 16
]


@pytest.mark.parametrize("n,n_dense,w_std,b_std,absolute,rows", CASES)
def test_nlml_and_gradient_against_the_oracle(golden_dir, n, n_dense, w_std, b_std, absolute, rows):
    x, y = _rows(golden_dir, rows, n)
    w, b, acts = _net(n_dense, w_std, b_std)
    lam = 1e-3 if not absolute else (1e-3 if rows == "unit" or rows == "synthetic" else 1.0)
    ref = R.Oracle(x, y).full(*R.variances(w, b), acts, lam, absolute)
    m = mll.NNGPMarginalLikelihood(n, x.shape[1]).set_train(x, y)
    nlml, g = m.evaluate((w, b, acts), lam, absolute)
    _check(m, None, nlml, g, ref)
    # bit-identical repeats; the NLML alone equals the one with the gradient
    nlml2, g2 = m.evaluate((w, b, acts), lam, absolute)
    assert nlml2 == nlml and np.array_equal(g2, g)
    nlml3, none = m.evaluate((w, b, acts), lam, absolute, with_grad=False)
    assert none is None and nlml3 == nlml
    m.close()


@pytest.mark.parametrize("act", [("abrelu", 0.1, 1.0), ("abrelu", -1.0, 1.0)])
@pytest.mark.parametrize("b_std", [0.0, 0.05])
def test_leaky_relu_and_abs_networks(golden_dir, act, b_std):
    x, y = _rows(golden_dir, "unit", 1000)
    w, b, acts = _net(3, 1.2, b_std, act)
    ref = R.Oracle(x, y).full(*R.variances(w, b), acts, 1e-3)
    m = mll.NNGPMarginalLikelihood(1000, x.shape[1]).set_train(x, y)
    nlml, g = m.evaluate((w, b, acts), 1e-3)
    _check(m, None, nlml, g, ref)
    m.close()


def test_zero_and_duplicated_rows(golden_dir):
    """b_0 = 0 with zero rows (q = 0) and duplicated rows (s = 0 off the diagonal): a finite gradient, equal to the oracle's."""
    x, y = _rows(golden_dir, "unit", 600)
    x[5] = 0.0
    x[77] = 0.0
    x[300:310] = x[100:110]
    w, b, acts = [1.0, 1.3, 1.1], [0.0, 0.05, 0.0], [("relu",), ("abrelu", 0.1, 1.0)]
    ref = R.Oracle(x, y).full(*R.variances(w, b), acts, 1e-3)
    m = mll.NNGPMarginalLikelihood(600, x.shape[1]).set_train(x, y)
    nlml, g = m.evaluate((w, b, acts), 1e-3)
    assert np.all(np.isfinite(g))
    _check(m, None, nlml, g, ref)
    m.close()


def test_device_gradient_against_finite_differences_of_the_device_nlml(golden_dir):
    x, y = _rows(golden_dir, "unit", 1000)
    w, b, acts = [1.2, 0.9, 1.1], [0.05, 0.1, 0.02], [("relu",), ("relu",)]
    m = mll.NNGPMarginalLikelihood(1000, x.shape[1]).set_train(x, y)
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
        scale = max(abs(t["quad"][p]), abs(t["trace"][p]))
        assert abs(fd - g[p]) <= 1e-6 * scale, (p, fd, g[p], scale)
    m.close()


def test_errors(golden_dir):
    lib = _lib.load()
    x, y = _rows(golden_dir, "unit", 300)
    m = mll.NNGPMarginalLikelihood(300, x.shape[1]).set_train(x, y)
    # a pivot that is not positive: absolute lambda = 0 with duplicated rows -- names a column; the handle stays usable
    xd = x.copy()
    xd[200:220] = xd[10:30]
    m.set_train(xd, y)
    w, b, acts = _net(2, 1.0, 0.0)
    with pytest.raises(_lib.NngpError, match="column"):
        m.evaluate((w, b, acts), 0.0, absolute=True)
    ref = R.Oracle(xd, y).full(*R.variances(w, b), acts, 1e-3)
    nlml, g = m.evaluate((w, b, acts), 1e-3)
    _check(m, None, nlml, g, ref)
    # Erf returns -2; ny = 2 returns -2; a negative or non-finite parameter returns -2
    arch = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])
    out = ctypes.c_double()
    assert lib.nngp_mll_evaluate(m._h, ctypes.byref(arch), 1e-3, 0, ctypes.byref(out), None, _lib.stream_ptr()) == -2
    arch = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("relu",)])
    assert lib.nngp_mll_evaluate(m._h, ctypes.byref(arch), -1e-3, 0, ctypes.byref(out), None, _lib.stream_ptr()) == -2
    assert lib.nngp_mll_evaluate(m._h, ctypes.byref(arch), float("nan"), 0, ctypes.byref(out), None, _lib.stream_ptr()) == -2
    y2 = torch.zeros(300, 2, dtype=torch.float64, device=DEV)
    xt = _lib.to_device_f64(x, DEV)
    assert lib.nngp_mll_set_train(m._h, _lib.ptr(xt), _lib.ptr(y2), 300, 2, _lib.stream_ptr()) == -2
    # the Python layer refuses Erf, the NTK and two output columns before any GPU call
    _, _, kf_erf = stax.serial(stax.Dense(8), stax.Erf(), stax.Dense(1))
    _, _, kf = stax.serial(stax.Dense(8), stax.Relu(), stax.Dense(1))
    with pytest.raises(ValueError):
        mll.marginal_likelihood(kf_erf, x, y)
    with pytest.raises(ValueError):
        mll.check_supported(kf, get="ntk")
    with pytest.raises(ValueError):
        mll.marginal_likelihood(kf, x, np.stack([y, y], 1))
    m.close()


def test_tune_hyperparameters_matches_the_oracle_driven_run_and_the_posterior(golden_dir):
    f = _forest(golden_dir)
    x, y, xt = f["X_train"] / 1000.0, f["Y_train"], f["X_test"] / 1000.0
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.0, b_std=0.05), stax.Relu(), stax.Dense(1, W_std=1.0, b_std=0.05))
    printed = []
    kf_t, lam_t, hist = mll.tune_hyperparameters(kf, x, y, steps=10, lr=0.05, report=printed.append)
    kf_o, lam_o, hist_o = mll.tune_hyperparameters(kf, x, y, steps=10, lr=0.05, report=None, evaluator=R.Oracle(x, y))
    np.testing.assert_allclose(kf_t.w_std, kf_o.w_std, rtol=1e-8)
    np.testing.assert_allclose(kf_t.b_std, kf_o.b_std, rtol=1e-8)
    assert _rel(lam_t, lam_o) <= 1e-8
    np.testing.assert_allclose(hist, hist_o, rtol=1e-9)
    assert hist[-1] < hist[0]
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, v) for i, v in enumerate(hist)]
    # the tuned network through the posterior, against oracle.Posterior at the tuned values
    mean, var = predict.gradient_descent_mse_ensemble(kf_t, x, y, diag_reg=lam_t)(x_test=xt, get="nngp", compute_cov="diag")
    arch = oracle.Arch(tuple(kf_t.w_std), tuple(kf_t.b_std))
    ref_mean, ref_cov = oracle.Posterior(x, y, arch, diag_reg=lam_t).predict(xt, "nngp", True)
    assert np.linalg.norm(mean - ref_mean) / np.linalg.norm(ref_mean) <= 1e-6
    np.testing.assert_allclose(var, np.diag(ref_cov), rtol=1e-5)


def test_train_cli_tune_hyper_on_forest_queries(golden_dir, tmp_path):
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
    args = train_cli.make_parser().parse_args(["--kernel_type", "nngp", "--query_path", str(tmp_path), "--max_num_train", "1000",
                                               "--max_num_test", "200", "--tune_hyper", "5", "--b_std_init", "0.05"])
    args.join_query = False
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    text = buf.getvalue()
    for i in range(5):
        assert "Step: %d, neg marginal likelihood:" % i in text
    for needle in ("Tuned W_std", "Kernel construction in", "Mean Square Error:", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    assert np.all(np.isfinite(res["pred_mean"]))
    bad = train_cli.make_parser().parse_args(["--kernel_type", "ntk", "--query_path", str(tmp_path), "--tune_hyper", "2"])
    bad.join_query = False
    with pytest.raises(ValueError):
        train_cli.main(bad)


def test_reference_size():
    """N = 10800, d = 20 (the reference's forest run), one ReLU layer: NLML and gradient against the oracle."""
    x, y = synth.synthetic_queries(10800, 20, seed=7)
    x = x / 1000.0
    y = y.reshape(-1)
    w, b, acts = _net(2, 1.0, 0.0)
    ref = R.Oracle(x, y, block=1024).full(*R.variances(w, b), acts, 1e-3)
    m = mll.NNGPMarginalLikelihood(10800, 20).set_train(x, y)
    nlml, g = m.evaluate((w, b, acts), 1e-3)
    _check(m, None, nlml, g, ref)
    m.close()
