"""--kernel_type gp on the host: the NumPy oracle's analytic gradient against torch autograd and finite differences, the
update rule of gp.py against a hand-written trajectory, and the CLI flag.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_reference as R  # noqa: E402
from nngp_src_amd import gp, train as train_cli  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=40, d=5, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, scale, size=(n, d))
    y = np.sin(x.sum(axis=1, keepdims=True)) + 0.1 * rng.standard_normal((n, 1))
    return x, y


def _torch_nlml(x, y, raw):
    """The reference's computation in torch float64: Cholesky and triangular solves, differentiated by autograd."""
    p = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    sp = torch.logaddexp(p, torch.zeros((), dtype=torch.float64))
    amp, noise, ls = sp[0], sp[1], sp[2]
    xt = torch.tensor(x, dtype=torch.float64) / ls
    yt = torch.tensor(y, dtype=torch.float64).reshape(-1, 1)
    yt = yt - yt.mean()
    n = xt.shape[0]
    d2 = ((xt[:, None, :] - xt[None, :, :]) ** 2).sum(-1)
    a = amp * torch.exp(-d2) + torch.eye(n, dtype=torch.float64) * (noise + 1e-6)
    l = torch.linalg.cholesky(a)
    w = torch.linalg.solve_triangular(l, yt, upper=False)
    kinvy = torch.linalg.solve_triangular(l.T, w, upper=True)
    c = float(np.log(2. * 3.1415))
    ml = -0.5 * (yt.T @ kinvy).sum() - torch.log(torch.diagonal(l)).sum() - (n / 2.) * c
    ml = ml - (-0.5 * c - torch.log(amp) ** 2)
    nlml = -ml
    nlml.backward()
    return nlml.item(), p.grad.numpy().copy()


@pytest.mark.parametrize("raw", [(0.0, -5.0, 0.0), (0.3, -2.0, -0.4), (-0.7, -4.0, 0.9)])
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_oracle_gradient_matches_autograd(raw, scale):
    x, y = _data(scale=scale)
    o = R.Oracle(x, y)
    nlml, g, terms = o.evaluate(raw)
    t_nlml, t_g = _torch_nlml(x, y, raw)
    assert abs(nlml - t_nlml) <= 1e-12 * abs(t_nlml)
    np.testing.assert_allclose(g, t_g, rtol=1e-10, atol=1e-10 * np.abs(terms["quad_half"] + terms["trace_half"]).max())


@pytest.mark.parametrize("raw", [(0.0, -5.0, 0.0), (0.3, -2.0, -0.4)])
def test_oracle_gradient_matches_central_differences(raw):
    x, y = _data(n=30, d=3, seed=1)
    o = R.Oracle(x, y)
    _, g, terms = o.evaluate(raw)
    h = 1e-3
    fd = np.zeros(3)
    for i in range(3):
        def f(t):
            r = np.array(raw, dtype=np.float64)
            r[i] += t
            return o.evaluate(r, False)[0]
        # fourth-order central difference: truncation ~h^4, rounding ~eps |f| / h
        fd[i] = (8.0 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12.0 * h)
    scale = np.abs(terms["quad_half"]) + np.abs(terms["trace_half"])
    assert np.all(np.abs(fd - g) <= 1e-10 * np.maximum(scale, np.abs(g)) + 1e-10), (fd, g)


def test_oracle_terms_are_consistent():
    x, y = _data()
    o = R.Oracle(x, y)
    nlml, g, t = o.evaluate((0.2, -3.0, 0.1))
    nlml2, none, t2 = o.evaluate((0.2, -3.0, 0.1), False)
    assert none is None and nlml == nlml2
    _, noise, _ = R.softplus(np.array([0.2, -3.0, 0.1]))
    assert t["tr_ainv"] > 0 and t["a_a"] > 0 and np.isfinite(t["tr_ainv_kd"])


def test_update_rule_reproduces_a_hand_written_trajectory():
    """gp.train_hyperparameters driven by the NumPy evaluator, against three steps written out scalar by scalar."""
    x, y = _data(n=25, d=4, seed=3)
    o = R.Oracle(x, y)
    calls = []

    def evaluate(raw, with_grad):
        calls.append((np.array(raw), with_grad))
        nlml, g, _ = o.evaluate(raw, with_grad)
        return nlml, g

    printed = []
    raw, hist = gp.train_hyperparameters(evaluate, steps=3, report=printed.append)
    assert [c[1] for c in calls] == [True, True, True, False]  # 4 evaluations for 3 steps; the last needs no gradient

    p = [0.0, -5.0, 0.0]
    mom = [0.0, 0.0, 0.0]
    sc = [1.0, 1.0, 1.0]
    g = list(o.evaluate(p)[1])
    expect_p, expect_nlml = [], []
    for step in range(3):
        for k in range(3):
            mom[k] = 0.9 * mom[k] + 0.1 * g[k]
            sc[k] = 0.9 * sc[k] + 0.1 * g[k] ** 2
            p[k] = p[k] - 0.01 * mom[k] / np.sqrt(sc[k] + 1e-5)
        nlml, gg, _ = o.evaluate(p)
        g = list(gg)
        expect_p.append(list(p))
        expect_nlml.append(nlml)
    for step in range(3):
        np.testing.assert_array_equal(calls[step + 1][0], expect_p[step])
    np.testing.assert_array_equal(raw, expect_p[-1])
    assert hist == expect_nlml
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, v) for i, v in enumerate(expect_nlml)]
    # the first step moves every parameter against its gradient by about lr (|m| / sqrt(s) ~ 0.1 / sqrt(0.9) for |g| >> 1)
    g0 = o.evaluate((0.0, -5.0, 0.0))[1]
    assert np.all(np.sign(expect_p[0] - np.array([0.0, -5.0, 0.0])) == -np.sign(g0))


def test_oracle_trajectory_matches_the_update_rule():
    x, y = _data(n=20, d=3, seed=4)
    o = R.Oracle(x, y)
    traj, nlmls = R.train(o, steps=4)
    raw, hist = gp.train_hyperparameters(lambda r, w: o.evaluate(r, w)[:2], steps=4, report=None)
    np.testing.assert_array_equal(raw, traj[-1])
    assert hist == nlmls


def test_oracle_predict_matches_dense_formula():
    x, y = _data(n=30, d=3, seed=5)
    xt, _ = _data(n=7, d=3, seed=6)
    o = R.Oracle(x, y)
    raw = (0.1, -2.0, 0.2)
    amp, noise, ls = R.softplus(np.array(raw))
    mean, cov = o.predict(raw, xt, full=True)
    a = amp * R.rbf(x, x, ls) + (noise + 1e-6) * np.eye(30)
    kx = amp * R.rbf(xt, x, ls)
    np.testing.assert_allclose(mean.ravel(), kx @ np.linalg.solve(a, o.y) + o.ymean, rtol=1e-10)
    np.testing.assert_allclose(cov, amp * R.rbf(xt, xt, ls) - kx @ np.linalg.solve(a, kx.T), rtol=1e-8, atol=1e-12)
    _, var = o.predict(raw, xt)
    np.testing.assert_allclose(var, np.diag(cov), rtol=1e-12)


def test_parser_accepts_gp():
    args = train_cli.make_parser().parse_args(["--kernel_type", "gp"])
    assert args.kernel_type == "gp"
    assert "gp" in train_cli.make_parser()._option_string_actions["--kernel_type"].help


def test_gp_abi_is_bound_and_declared():
    from nngp_src_amd import _lib
    import re
    header = open(os.path.join(ROOT, "include", "nngp_rbf_gp.h")).read()
    declared = set(re.findall(r"\b(nngp_[a-z0-9_]+)\s*\(", header)) - {"nngp_last_error"}  # (named in a comment)
    assert declared == set(_lib.GP_ABI_SYMBOLS)
    lib = _lib.load()
    for name in _lib.GP_ABI_SYMBOLS:
        assert hasattr(lib, name), name
    # argument checks answer before any device work
    h = __import__("ctypes").c_void_p()
    assert lib.nngp_rbf_gp_create(__import__("ctypes").byref(h), 0, 0, 4) < 0
    assert b"rbf_gp_create" in lib.nngp_last_error()
    assert lib.nngp_potrf_f64(None, 100, 100, None) < 0 and b"multiple of 128" in lib.nngp_last_error()
