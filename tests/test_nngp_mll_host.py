"""CPU tests of the NNGP marginal likelihood: the NumPy oracle (nngp_mll_reference.py) against torch float64 autograd and
finite differences, the parameter mapping and kernel_fn rebuild of mll.tune_hyperparameters, the generalised update rule, and
what is refused without a GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activation_reference as AR  # noqa: E402
import nngp_mll_reference as R  # noqa: E402
import nngp_oracle as oracle  # noqa: E402
from nngp_src_amd import _lib, gp, mll, stax  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=90, d=6, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)), rng.standard_normal(n)


def torch_nlml(x, y, v, c, acts, lam, absolute):
    """The NLML restated in torch (exact diagonal, safe-where sqrt) for autograd."""
    x = torch.as_tensor(x, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64)
    n, d = x.shape
    eye = torch.eye(n, dtype=torch.bool)
    q = (x * x).sum(1) / d
    k = torch.where(eye, q[:, None].expand(n, n), x @ x.T / d)
    q1, q2 = q[:, None], q[None, :]
    for l in range(len(v)):
        k = v[l] * k + c[l]
        q1 = v[l] * q1 + c[l]
        q2 = v[l] * q2 + c[l]
        if l == len(v) - 1:
            break
        spec = R._spec(acts[l])
        h = R._h(spec)
        r = torch.where(eye, torch.ones_like(k), q1 * q2 - k * k)
        s = torch.where(eye, torch.zeros_like(k), torch.sqrt(torch.clamp(r, min=0.0)))
        th = torch.atan2(s, k)
        kr = s / (2 * math.pi) + (math.pi - th) / (2 * math.pi) * k
        if spec[0] == "abrelu":
            a, b = spec[1], spec[2]
            kr = a * b * k + (b - a) ** 2 * kr
        k = torch.where(eye, h * k, kr)
        q1, q2 = h * q1, h * q2
    reg = lam if absolute else lam * torch.trace(k) / n
    a_mat = k + reg * torch.eye(n, dtype=torch.float64)
    ell = torch.linalg.cholesky(a_mat)
    alpha = torch.cholesky_solve(y[:, None], ell)[:, 0]
    return 0.5 * y @ alpha + torch.log(torch.diagonal(ell)).sum() + 0.5 * n * math.log(2 * math.pi)


NETS = [
    ([1.0, 1.0], [0.0, 0.0], [("relu",)]),
    ([1.5, 1.2, 0.9], [0.05, 0.1, 0.02], [("relu",), ("relu",)]),
    ([1.1, 1.3, 1.0], [0.0, 0.05, 0.0], [("abrelu", 0.1, 1.0), ("abrelu", -1.0, 1.0)]),
    ([1.2, 0.8], [0.05, 0.05], [("abrelu", -1.0, 1.0)]),
]


@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_oracle_gradient_against_torch_autograd(net, absolute):
    w, b, acts = NETS[net]
    x, y = _data()
    v, c = R.variances(w, b)
    lam = 1e-3 if not absolute else 0.05
    ref = R.Oracle(x, y, block=32).full(v, c, acts, lam, absolute)
    vt = [torch.tensor(e, dtype=torch.float64, requires_grad=True) for e in v]
    ct = [torch.tensor(e, dtype=torch.float64, requires_grad=True) for e in c]
    lt = torch.tensor(lam, dtype=torch.float64, requires_grad=True)
    f = torch_nlml(x, y, vt, ct, acts, lt, absolute)
    f.backward()
    auto = [t.grad.item() for pair in zip(vt, ct) for t in pair] + [lt.grad.item()]
    assert abs(f.item() - ref["nlml"]) <= 1e-11 * abs(ref["nlml"])
    gate = 1e-10 * np.maximum(np.abs(ref["quad"]), np.abs(ref["trace"])) + 1e-13
    assert np.all(np.abs(np.array(auto) - ref["grad"]) <= gate), (auto, ref["grad"])
    np.testing.assert_allclose(ref["grad"], -0.5 * ref["quad"] + 0.5 * ref["trace"], rtol=0, atol=0)


@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("net", range(len(NETS)))
def test_oracle_gradient_against_central_differences(net, absolute):
    x, y = _data(seed=1)
    _central_differences(x, y, net, absolute)


def test_oracle_gradient_against_central_differences_on_centred_forest_rows(golden_dir):
    """The rows of the GPU file's "centred" cases (unit forest rows minus their mean: obtuse angles, mixed signs), so that the
    oracle is itself checked at the angles it is about to referee."""
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    x = g["X_train"][:90] / 1000.0
    x = x - x.mean(0)
    y = g["Y_train"][:90].reshape(-1)
    cos = (x @ x.T) / np.sqrt(np.outer((x * x).sum(1), (x * x).sum(1)))
    assert cos.min() < -0.5 and (cos < 0).mean() > 0.3
    _central_differences(x, y, 1, False)


def _central_differences(x, y, net, absolute):
    w, b, acts = NETS[net]
    v, c = R.variances(w, b)
    lam = 1e-3 if not absolute else 0.05
    o = R.Oracle(x, y, block=40)
    ref = o.full(v, c, acts, lam, absolute)
    nd = len(v)
    for p in range(2 * nd + 1):
        base = lam if p == 2 * nd else (v[p // 2] if p % 2 == 0 else c[p // 2])
        h = 1e-3 * (base if base > 0.0 else 1e-2)

        def f(t):
            vv, cc, ll = list(v), list(c), lam
            if p == 2 * nd:
                ll += t
            elif p % 2 == 0:
                vv[p // 2] += t
            else:
                cc[p // 2] += t
            return o.nlml_var(vv, cc, acts, ll, absolute)

        fd = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        scale = max(abs(ref["quad"][p]), abs(ref["trace"][p]))
        assert abs(fd - ref["grad"][p]) <= 1e-6 * scale, (p, fd, ref["grad"][p])


def test_oracle_kernel_matches_the_kernel_references():
    x, _ = _data(70, 5, seed=3)
    for w, b, acts in NETS:
        v, c = R.variances(w, b)
        k = R.Oracle(x, np.zeros(70), block=16).kernel(v, c, acts)
        np.testing.assert_allclose(k, AR.kernel_fn(x, None, "nngp", w, b, acts), rtol=1e-14, atol=1e-15)
        if all(a == ("relu",) for a in acts):  # oracle/nngp_oracle.py: the same off the diagonal
            ko = oracle.kernel_fn(x, None, "nngp", oracle.Arch(tuple(w), tuple(b)))
            off = ~np.eye(70, dtype=bool)
            np.testing.assert_allclose(k[off], ko[off], rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(np.diag(k), oracle.diag_kernel(np.sum(x * x, 1) / 5, oracle.Arch(tuple(w), tuple(b)))[0],
                                       rtol=1e-15)


def test_zero_row_gradient_follows_the_q_rule():
    """A zero row with b_0 = 0: the q = 0 rule keeps the tangents finite; the sigma_w^2 components and the sigma_b^2
    components from the first positive bias on still match finite differences."""
    x, y = _data(60, 4, seed=4)
    x[7] = 0.0
    w, b, acts = [1.0, 1.2, 0.9], [0.0, 0.1, 0.05], [("relu",), ("relu",)]
    v, c = R.variances(w, b)
    o = R.Oracle(x, y, block=32)
    ref = o.full(v, c, acts, 1e-3)
    assert np.all(np.isfinite(ref["grad"]))
    for p in (0, 2, 3, 4, 5, 6):
        base = 1e-3 if p == 6 else (v[p // 2] if p % 2 == 0 else c[p // 2])
        h = 1e-3 * base

        def f(t):
            vv, cc, ll = list(v), list(c), 1e-3
            if p == 6:
                ll += t
            elif p % 2 == 0:
                vv[p // 2] += t
            else:
                cc[p // 2] += t
            return o.nlml_var(vv, cc, acts, ll)

        fd = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        assert abs(fd - ref["grad"][p]) <= 1e-6 * max(abs(ref["quad"][p]), abs(ref["trace"][p])), p


def test_parameter_mapping_and_rebuild():
    p = mll._Params([1.5, 0.5], [0.0, 0.2], 1e-3)
    assert p.free_b == [1]
    np.testing.assert_allclose(p.raw0, [math.log(2.25), math.log(0.25), math.log(0.04), math.log(1e-3)])
    w, b, lam, clamped = p.unpack(p.raw0)
    np.testing.assert_allclose(w, [1.5, 0.5])
    np.testing.assert_allclose(b, [0.0, 0.2])
    assert abs(lam - 1e-3) < 1e-18 and not clamped
    g = np.array([1.0, 2.0, 3.0, 4.0, 5.0])  # d/dv0, d/dc0, d/dv1, d/dc1, d/dlambda
    np.testing.assert_allclose(p.grad_raw(g, p.raw0), [1.0 * 2.25, 3.0 * 0.25, 4.0 * 0.04, 5.0 * 1e-3])
    # lambda below min_diag_reg is held there, and its raw gradient vanishes
    raw = p.raw0.copy()
    raw[-1] = math.log(1e-9)
    _, _, lam, clamped = p.unpack(raw)
    assert lam == 1e-6 and clamped and p.grad_raw(g, raw)[-1] == 0.0
    # b_std_init frees the layers whose b_std is 0, and keeps the others' own start
    q = mll._Params([1.0, 1.0, 1.0], [0.0, 0.3, 0.0], 1e-2, b_std_init=0.05)
    assert q.free_b == [0, 1, 2]
    np.testing.assert_allclose(q.unpack(q.raw0)[1], [0.05, 0.3, 0.05])
    with pytest.raises(ValueError):
        mll._Params([1.0, 1.0], [0.0, 0.0], 1e-3, b_std_init=[0.1])
    kf = mll.rebuild_kernel_fn([1.2, 0.7, 1.1], [0.0, 0.05, 0.1], [("relu",), ("abrelu", 0.1, 1.0)])
    assert kf.w_std == (1.2, 0.7, 1.1) and kf.b_std == (0.0, 0.05, 0.1)
    assert kf.activations == (("relu",), ("abrelu", 0.1, 1.0))


def _old_rule(evaluate, raw0, steps, lr):
    """The update rule as it stood for the RBF GP (three parameters), written out by hand."""
    raw = np.array(raw0, dtype=np.float64)
    m, s = np.zeros(3), np.ones(3)
    _, g = evaluate(raw, True)
    traj = []
    for i in range(steps):
        m = 0.9 * m + 0.1 * g
        s = 0.9 * s + 0.1 * g ** 2
        raw = raw - lr * m / np.sqrt(s + 1e-5)
        _, g = evaluate(raw, i + 1 < steps)
        traj.append(raw.copy())
    return raw, traj


def test_generalised_update_rule():
    def quad(raw, with_grad):
        t = np.arange(1.0, raw.size + 1.0)
        return float(np.sum(t * raw ** 2)), (2.0 * t * raw if with_grad else None)

    # three parameters: identical to the rule as it was
    seen = []

    def ev3(raw, with_grad):
        seen.append(np.array(raw))
        return quad(raw, with_grad)

    raw, hist = gp.train_hyperparameters(ev3, (0.3, -0.2, 0.5), steps=6, lr=0.05, report=None)
    old_raw, old_traj = _old_rule(quad, (0.3, -0.2, 0.5), 6, 0.05)
    assert np.array_equal(raw, old_raw)
    for a, b_ in zip(seen[1:], old_traj):
        assert np.array_equal(a, b_)
    # five parameters: the same rule per parameter, by hand
    r = np.array([0.4, -0.1, 0.2, 0.7, -0.3])
    m, s = np.zeros(5), np.ones(5)
    g = quad(r, True)[1]
    expect = []
    for i in range(4):
        m = 0.9 * m + 0.1 * g
        s = 0.9 * s + 0.1 * g ** 2
        r = r - 0.05 * m / np.sqrt(s + 1e-5)
        expect.append(quad(r, False)[0])
        g = quad(r, True)[1]
    printed = []
    raw5, hist5 = gp.train_hyperparameters(quad, (0.4, -0.1, 0.2, 0.7, -0.3), steps=4, lr=0.05, report=printed.append)
    np.testing.assert_allclose(raw5, r, rtol=0, atol=0)
    np.testing.assert_allclose(hist5, expect, rtol=0, atol=0)
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, v) for i, v in enumerate(expect)]


def test_tune_with_the_oracle_evaluator_lowers_the_nlml():
    x, y = _data(80, 5, seed=5)
    _, _, kf = stax.serial(stax.Dense(16), stax.LeakyRelu(0.1), stax.Dense(1))
    kf_t, lam, hist = mll.tune_hyperparameters(kf, x, y, steps=8, lr=0.05, b_std_init=0.05, report=None,
                                               evaluator=R.Oracle(x, y, block=40))
    assert len(hist) == 8 and hist[-1] < hist[0]
    assert kf_t.activations == (("abrelu", 0.1, 1.0),) and all(bv > 0.0 for bv in kf_t.b_std) and lam > 0.0


def test_refused_without_a_gpu():
    x, y = _data(20, 3)
    _, _, kf_erf = stax.serial(stax.Dense(8), stax.Erf(), stax.Dense(1))
    _, _, kf = stax.serial(stax.Dense(8), stax.Relu(), stax.Dense(1))
    with pytest.raises(ValueError, match="Erf"):
        mll.marginal_likelihood(kf_erf, x, y)
    with pytest.raises(ValueError, match="Erf"):
        mll.tune_hyperparameters(kf_erf, x, y, steps=1, report=None)
    with pytest.raises(ValueError, match="NTK"):
        mll.check_supported(kf, get="ntk")
    with pytest.raises(ValueError, match="one output column"):
        mll.marginal_likelihood(kf, x, np.stack([y, y], 1))


def test_train_cli_flags():
    from nngp_src_amd import train
    a = train.make_parser().parse_args([])
    assert a.tune_hyper == 0 and a.b_std_init is None
    a = train.make_parser().parse_args(["--tune_hyper", "5", "--tune_lr", "0.1", "--b_std_init", "0.05"])
    assert (a.tune_hyper, a.tune_lr, a.b_std_init) == (5, 0.1, 0.05)
    bad = train.make_parser().parse_args(["--kernel_type", "ntk", "--tune_hyper", "2"])
    bad.join_query = False
    with pytest.raises(ValueError, match="nngp"):
        train.main(bad)


def test_mll_symbols_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_mll.h")) as f:
        declared = set(re.findall(r"\bint (nngp_mll_\w+)\(", f.read()))
    assert declared == set(_lib.MLL_ABI_SYMBOLS)
