"""--kernel_type gp on the MI355X (float64 RBF GP, reference train.py:60-150) against the NumPy oracle of gp_reference.py."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_reference as R  # noqa: E402
from nngp_src_amd import _lib, gp, train as train_cli  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _forest(golden_dir, name="forest_n1000_m200.npz"):
    g = np.load(os.path.join(golden_dir, name))
    return {k: g[k] for k in g.files}


def _rel(a, b):
    return abs(a - b) / abs(b)


def _grad_gate(g, terms):
    return 1e-9 * (np.abs(terms["quad_half"]) + np.abs(terms["trace_half"])) + 1e-12


@pytest.mark.parametrize("ls", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("n", [127, 1000, 4097])
@pytest.mark.parametrize("unit", [False, True])
def test_kernel_entries(golden_dir, ls, n, unit):
    f = _forest(golden_dir)
    x = np.concatenate([f["X_train"], f["X_test"]] * 4)[:n]
    if unit:
        x = x / 1000.0
    xt = f["X_test"][:77] / (1000.0 if unit else 1.0)
    np.testing.assert_allclose(gp.kernel(x, None, ls), R.rbf(x, x, ls), rtol=0, atol=1e-12)
    np.testing.assert_allclose(gp.kernel(xt, x, ls), R.rbf(xt, x, ls), rtol=0, atol=1e-12)


def test_potrf_f64_factor_and_not_positive_definite():
    lib = _lib.load()
    rng = np.random.default_rng(0)
    n = 4096
    x = rng.uniform(0.0, 1.0, size=(n, 8))
    a = 0.7 * R.rbf(x, x, 0.5) + 1e-3 * np.eye(n)
    ad = torch.from_numpy(a).to(DEV)
    _lib.check(lib.nngp_potrf_f64(_lib.ptr(ad), n, n, _lib.stream_ptr()), lib)
    l = np.tril(ad.cpu().numpy())
    assert np.linalg.norm(a - l @ l.T) / np.linalg.norm(a) <= 1e-13
    ref = 0.5 * np.linalg.slogdet(a)[1]
    assert _rel(np.sum(np.log(np.diag(l))), ref) <= 1e-12
    # not positive definite: a negative direction appears at column 300; rc < 0 naming it, no NaN pivot
    m = 384
    b = np.eye(m) * 2.0
    b[300, 300] = -1.0
    bd = torch.from_numpy(b).to(DEV)
    rc = lib.nngp_potrf_f64(_lib.ptr(bd), m, m, _lib.stream_ptr())
    assert rc < 0 and b"column 300" in lib.nngp_last_error()
    assert lib.nngp_potrf_f64(_lib.ptr(bd), 100, 100, _lib.stream_ptr()) < 0  # not a multiple of 128


def _unit_fixture(golden_dir):
    f = _forest(golden_dir)
    return f["X_train"] / 1000.0, f["Y_train"], f["X_test"] / 1000.0, f


@pytest.mark.parametrize("raw", [(0.0, -5.0, 0.0), (0.4, -3.0, -0.6)])
@pytest.mark.parametrize("n", [127, 1000])
def test_nlml_gradient_and_factor(golden_dir, raw, n):
    x, y, _, _ = _unit_fixture(golden_dir)
    x, y = x[:n], y[:n]
    o = R.Oracle(x, y)
    nlml_ref, g_ref, terms = o.evaluate(raw)
    m = gp.RBFGP(n, x.shape[1]).set_train(x, y)
    nlml, g = m.evaluate(raw)
    assert _rel(nlml, nlml_ref) <= 1e-10
    assert np.all(np.abs(g - g_ref) <= _grad_gate(g, terms)), (g, g_ref)
    t = m.terms()
    assert _rel(t["logdet_half"], terms["logdet_half"]) <= 1e-12
    for k in ("a_k_a", "tr_ainv_k", "a_a", "tr_ainv"):
        assert _rel(t[k], terms[k]) <= 1e-9, k
    amp, noise, ls, _, _, a, _ = o.factor(raw)
    l = np.tril(m.factor().cpu().numpy())[:n, :n]
    assert np.linalg.norm(a - l @ l.T) / np.linalg.norm(a) <= 1e-13
    # two evaluations at the same point are bit-identical; the NLML alone equals the one with the gradient
    nlml2, g2 = m.evaluate(raw)
    assert nlml2 == nlml and np.array_equal(g2, g)
    nlml3, none = m.evaluate(raw, False)
    assert none is None and nlml3 == nlml
    m.close()


def test_trajectory_and_posterior_on_the_forest_fixture(golden_dir):
    x, y, xt, f = _unit_fixture(golden_dir)
    o = R.Oracle(x, y)
    traj, nlmls = R.train(o)
    m = gp.RBFGP(x.shape[0], x.shape[1], xt.shape[0]).set_train(x, y)
    seen = []

    def evaluate(raw, with_grad):
        out = m.evaluate(raw, with_grad)
        seen.append(np.array(raw))
        return out

    printed = []
    raw, hist = gp.train_hyperparameters(evaluate, report=printed.append)
    assert len(seen) == 11
    for step in range(10):
        np.testing.assert_allclose(seen[step + 1], traj[step], rtol=0, atol=1e-9)
        assert _rel(hist[step], nlmls[step]) <= 1e-10
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, v) for i, v in enumerate(nlmls)]
    mean_ref, var_ref = o.predict(raw, xt)
    mean, var = m.predict(xt, "diag")
    np.testing.assert_allclose(mean, mean_ref, rtol=1e-8)
    np.testing.assert_allclose(var, var_ref, rtol=1e-8)
    mean_n, none = m.predict(xt, None)
    assert none is None and np.array_equal(mean_n, mean)
    _, cov_ref = o.predict(raw, xt[:16], full=True)
    mean16, cov = m.predict(xt[:16], "full")
    np.testing.assert_allclose(mean16, mean_ref[:16], rtol=1e-8)
    np.testing.assert_allclose(cov, cov_ref, rtol=1e-8, atol=1e-8 * np.abs(np.diag(cov_ref)).max())
    m.close()


def test_train_cli_gp_on_forest_queries(golden_dir, tmp_path):
    """train.py --kernel_type gp on the reference's forest queries, raw encodings (K is the identity except for duplicates)."""
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
    args = train_cli.make_parser().parse_args(["--kernel_type", "gp", "--query_path", str(tmp_path),
                                               "--max_num_train", "1000", "--max_num_test", "200"])
    args.join_query = False
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    text = buf.getvalue()
    assert text.count("neg marginal likelihood:") == 10
    for needle in ("number of query: 18000", "(1000, 20) (200, 20)", "Step: 9, neg marginal likelihood:", "Kernel construction in",
                   "GP Inference in", "Predict Result Profile of", "Query attributes:num_predicates="):
        assert needle in text, needle
    import re
    assert sum(int(v) for v in re.findall(r"# Queries = (\d+)", text)) == 200  # the partitions cover the test set
    f = _forest(golden_dir)
    o = R.Oracle(f["X_train"], f["Y_train"])
    traj, nlmls = R.train(o)
    np.testing.assert_allclose(res["raw"], traj[-1], rtol=0, atol=1e-9)
    for i, v in enumerate(nlmls):
        assert "Step: %d, neg marginal likelihood: %f" % (i, v) in text
    mean_ref, var_ref = o.predict(traj[-1], f["X_test"])
    np.testing.assert_allclose(res["pred_mean"], mean_ref.ravel(), rtol=1e-8)
    np.testing.assert_allclose(res["pred_var"], var_ref, rtol=1e-8)


@pytest.mark.parametrize("unit", [False, True])
def test_reference_size(unit):
    """N = 10800 / M = 3600 (the reference's forest run), one gradient evaluation and one diagonal posterior."""
    from nngp_src_amd import synth
    x, y = synth.synthetic_queries(10800, 20, seed=7)
    xt, _ = synth.synthetic_queries(3600, 20, seed=8)
    scale = 1.0 / 1000.0 if unit else 1.0
    x, xt = x * scale, xt * scale  # synthetic encodings span [0, 1000] like the forest's
    raw = (0.2, -4.0, -0.3)
    o = R.Oracle(x, y)
    nlml_ref, g_ref, terms = o.evaluate(raw)
    m = gp.RBFGP(x.shape[0], x.shape[1], xt.shape[0]).set_train(x, y)
    nlml, g = m.evaluate(raw)
    assert _rel(nlml, nlml_ref) <= 1e-10
    assert np.all(np.abs(g - g_ref) <= _grad_gate(g, terms)), (g, g_ref)
    mean_ref, var_ref = o.predict(raw, xt)
    mean, var = m.predict(xt, "diag")
    np.testing.assert_allclose(mean, mean_ref, rtol=1e-8)
    np.testing.assert_allclose(var, var_ref, rtol=1e-8)
    m.close()


def test_errors_leave_the_handle_usable(golden_dir):
    lib = _lib.load()
    x, y, xt, _ = _unit_fixture(golden_dir)
    x, y = x[:300], y[:300]
    m = gp.RBFGP(300, x.shape[1], 8).set_train(x, y)
    nlml0, g0 = m.evaluate((0.0, -5.0, 0.0))
    xd = torch.from_numpy(x).to(DEV)
    y2 = torch.from_numpy(np.concatenate([y, y], axis=1)).to(DEV)
    assert lib.nngp_rbf_gp_set_train(m._h, _lib.ptr(xd), _lib.ptr(y2), 300, 2, _lib.stream_ptr()) < 0
    assert b"one output column" in lib.nngp_last_error()
    big = torch.zeros(301, x.shape[1], dtype=torch.float64, device=DEV)
    assert lib.nngp_rbf_gp_set_train(m._h, _lib.ptr(big), _lib.ptr(big), 301, 1, _lib.stream_ptr()) < 0
    assert b"n_cap" in lib.nngp_last_error()
    for bad in ((float("nan"), -5.0, 0.0), (0.0, float("inf"), 0.0)):
        with pytest.raises(_lib.NngpError, match="non-finite"):
            m.evaluate(bad)
    # a matrix that is not positive definite, through the stand-alone operator, between two uses of the handle
    b = torch.eye(256, dtype=torch.float64, device=DEV)
    b[200, 200] = -1.0
    assert lib.nngp_potrf_f64(_lib.ptr(b), 256, 256, _lib.stream_ptr()) < 0 and b"column 200" in lib.nngp_last_error()
    m.set_train(x, y)
    nlml1, g1 = m.evaluate((0.0, -5.0, 0.0))
    assert nlml1 == nlml0 and np.array_equal(g1, g0)
    mean, var = m.predict(xt[:8])
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    m.close()

