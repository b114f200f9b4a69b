"""Host checks (no GPU) of the Erf / ABRelu / LeakyRelu / Abs activations: the NumPy restatement (activation_reference.py)
against independent pins -- 2-D Gauss-Hermite quadrature, the ABRelu = linear + ReLU decomposition on the oracle's Cho-Saul
function, finite-width Monte Carlo through stax's apply_fn and a torch-autograd empirical NTK -- plus the stax front end and
the ctypes layout of nngp_arch_act."""
import ctypes
import fractions
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.special

import activation_reference as R
import nngp_oracle as o
from nngp_src_amd import _lib, stax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_GH_X, _GH_W = np.polynomial.hermite.hermgauss(200)


def _gauss2(q1, q2, k, f, g):
    """E[f(u) g(v)] for (u, v) ~ N(0, [[q1, k], [k, q2]]) by a 200 x 200 Gauss-Hermite rule on the Cholesky transform."""
    l11 = math.sqrt(q1)
    l21 = k / l11
    l22 = math.sqrt(max(q2 - l21 * l21, 0.0))
    z = math.sqrt(2.0) * _GH_X
    u = l11 * z[:, None]
    v = l21 * z[:, None] + l22 * z[None, :]
    w = np.outer(_GH_W, _GH_W) / math.pi
    return float(np.sum(w * f(u) * g(v)))


_GL_X, _GL_W = np.polynomial.legendre.leggauss(3000)


def _cond_erf(q1, q2, k, a, b, c, deriv):
    """The same expectation as a 1-D integral over u of f(u) E[g(v) | u], with the inner expectation in closed form
    (v | u ~ N(k u / q1, q2 - k^2 / q1)) and a 3000-node Gauss-Legendre rule on |u| <= 12 sqrt(q1): it resolves erf(b u)'s
    step at large b^2 q, where the 2-D Gauss-Hermite rule stops converging."""
    s2 = max(q2 - k * k / q1, 0.0)
    sd = math.sqrt(q1)
    u = 12.0 * sd * _GL_X
    dens = np.exp(-u * u / (2 * q1)) / math.sqrt(2 * math.pi * q1) * 12.0 * sd * _GL_W
    mu = k / q1 * u
    g = 1.0 + 2.0 * b * b * s2
    if deriv:
        f = a * b * (2.0 / math.sqrt(math.pi)) * np.exp(-b * b * u * u)
        inner = a * b * (2.0 / math.sqrt(math.pi)) * np.exp(-b * b * mu * mu / g) / math.sqrt(g)
    else:
        f = a * scipy.special.erf(b * u) + c
        inner = a * scipy.special.erf(b * mu / math.sqrt(g)) + c
    return float(np.sum(dens * f * inner))


@pytest.mark.parametrize("abc", [(1.0, 1.0, 0.0), (0.7, 1.6, 0.3), (1.3, 0.4, -0.5)])
@pytest.mark.parametrize("rho", [-0.8, 0.0, 0.3, 0.9, 0.999, 0.9999])
@pytest.mark.parametrize("bq", [0.05, 1.0, 10.0])
def test_erf_closed_form_against_quadrature(abc, rho, bq):
    a, b, c = abc
    q1 = bq / (b * b)
    q2 = 0.6 * q1
    k = rho * math.sqrt(q1 * q2)
    phi = lambda x: a * scipy.special.erf(b * x) + c
    dphi = lambda x: a * b * (2.0 / math.sqrt(math.pi)) * np.exp(-b * b * x * x)
    spec = ("erf", a, b, c)
    kn, kd = R.act_cross(spec, np.float64(k), np.float64(q1), np.float64(q2))
    qn, qkd = R.act_diag(spec, np.float64(q1))
    if bq <= 1.0:  # the 2-D Gauss-Hermite rule converges here
        assert abs(float(kn) - _gauss2(q1, q2, k, phi, phi)) < 1e-12
        assert abs(float(kd) - _gauss2(q1, q2, k, dphi, dphi)) < 1e-12
        assert abs(float(qn) - _gauss2(q1, q1, q1, phi, phi)) < 1e-12
        assert abs(float(qkd) - _gauss2(q1, q1, q1, dphi, dphi)) < 1e-12
    assert abs(float(kn) - _cond_erf(q1, q2, k, a, b, c, False)) < 1e-12
    assert abs(float(kd) - _cond_erf(q1, q2, k, a, b, c, True)) < 1e-12
    assert abs(float(qn) - _cond_erf(q1, q1, q1, a, b, c, False)) < 1e-12
    assert abs(float(qkd) - _cond_erf(q1, q1, q1, a, b, c, True)) < 1e-12


@pytest.mark.parametrize("ab", [(0.1, 1.0), (-1.0, 1.0), (-0.3, 2.0), (0.5, -1.5)])
def test_abrelu_against_the_cho_saul_decomposition(ab):
    """phi = a x + (b - a) relu(x):  K' = a^2 K + a (b - a) K + (b - a)^2 relu(K) (E[u relu(v)] = K / 2 twice)."""
    a, b = ab
    rng = np.random.default_rng(3)
    x = rng.standard_normal((9, 6)) * np.array([0.1, 1, 3, 1, 1, 2])
    x[4] = x[2]
    x[5] = -x[1]
    d = x.shape[1]
    k = x @ x.T / d
    relu_k = 0.5 * o.cho_saul_arccos1(x / math.sqrt(d), x / math.sqrt(d))
    want = a * a * k + a * (b - a) * k + (b - a) ** 2 * relu_k
    got = R.kernel_fn(x, x + 0.0, "nngp", [1.0, 1.0], [0.0, 0.0], [("abrelu", a, b)])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13 * np.abs(want).max())
    # the symmetric form (exact diagonal) agrees with it too
    np.testing.assert_allclose(R.kernel_fn(x, None, "nngp", [1.0, 1.0], [0.0, 0.0], [("abrelu", a, b)]), want, rtol=0,
                               atol=1e-13 * np.abs(want).max())


def test_relu_restatement_is_the_oracle():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((20, 7))
    xt = rng.standard_normal((5, 7))
    w, b = [1.2, 0.9, 1.1], [0.1, 0.2, 0.0]
    for get in ("nngp", "ntk"):
        want = o.kernel_fn(xt, x, get, o.Arch(tuple(w), tuple(b)))
        for acts in ([("relu",), ("relu",)], [("abrelu", 0.0, 1.0), ("relu",)]):
            np.testing.assert_allclose(R.kernel_fn(xt, x, get, w, b, acts), want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("act", [stax.Erf(), stax.Erf(0.8, 1.7, 0.2), stax.LeakyRelu(0.1), stax.Abs(), stax.ABRelu(-0.3, 2.0)])
def test_nngp_against_finite_width_monte_carlo(act):
    """apply_fn at width 2e5: the readout's NNGP given the hidden features is w^2 phi phi^T / width + b^2."""
    width = 200000
    init_fn, apply_fn, kernel_fn = stax.serial(stax.Dense(width, W_std=1.3, b_std=0.2), act, stax.Dense(1, W_std=0.9, b_std=0.1))
    rng = np.random.default_rng(5)
    x = rng.standard_normal((5, 8)) * 1.5
    _, params = init_fn(7, x.shape)
    feats = apply_fn(params, x, readout=False)
    emp = 0.81 * feats @ feats.T / width + 0.01
    want = R.kernel_fn(x, None, "nngp", kernel_fn.w_std, kernel_fn.b_std, kernel_fn.activations)
    assert np.abs(emp - want).max() < 1.5e-2 * np.abs(want).max()
    assert apply_fn(params, x).shape == (5, 1)


@pytest.mark.parametrize("acts", [[("erf", 1.0, 1.0, 0.0)], [("abrelu", -0.3, 2.0)], [("erf", 0.9, 1.4, 0.1), ("relu",)],
                                  [("abrelu", 0.1, 1.0), ("erf", 1.0, 0.7, 0.0)]])
def test_ntk_against_the_empirical_ntk(acts):
    """Width-4096 empirical NTK (torch autograd, NTK parameterisation, averaged over 4 draws) against the restated Theta."""
    import torch
    width, seeds = 4096, 4
    w_std = [1.2] + [1.0] * len(acts)
    b_std = [0.3] * (len(acts) + 1)
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((4, 5)))

    def phi(spec, h):
        if spec[0] == "relu":
            return torch.relu(h)
        if spec[0] == "abrelu":
            return torch.where(h < 0, spec[1] * h, spec[2] * h)
        return spec[1] * torch.erf(spec[2] * h) + spec[3]

    emp = np.zeros((4, 4))
    for seed in range(seeds):
        g = torch.Generator().manual_seed(seed)
        dims = [x.shape[1]] + [width] * len(acts) + [1]
        params = []
        for i in range(len(dims) - 1):
            params.append(torch.randn(dims[i], dims[i + 1], generator=g, dtype=torch.float64).requires_grad_())
            params.append(torch.randn(dims[i + 1], generator=g, dtype=torch.float64).requires_grad_())
        jac = []
        for r in range(4):
            h = x[r:r + 1]
            for i in range(len(dims) - 1):
                h = w_std[i] / math.sqrt(dims[i]) * (h @ params[2 * i]) + b_std[i] * params[2 * i + 1]
                if i < len(acts):
                    h = phi(acts[i], h)
            grads = torch.autograd.grad(h.sum(), params)
            jac.append(torch.cat([gr.reshape(-1) for gr in grads]))
        jm = torch.stack(jac)
        emp += (jm @ jm.T).detach().numpy() / seeds
    want = R.kernel_fn(x.numpy(), None, "ntk", w_std, b_std, acts)
    assert np.abs(emp - want).max() < 5e-2 * np.abs(want).max()


def test_stable_r_against_the_naive_form():
    """Near-duplicate rows at raw forest norms: the fused form keeps r to a few ulps, the product form loses digits."""
    rng = np.random.default_rng(8)
    x1 = rng.uniform(0.0, 3000.0, 8)
    x2 = x1 + rng.standard_normal(8) * 1e-3
    d = 8
    q1, q2, k = float(x1 @ x1 / d), float(x2 @ x2 / d), float(x1 @ x2 / d)
    assert q1 > 1e6
    F = fractions.Fraction
    exact = 1 + 2 * (F(q1) + F(q2)) + 4 * (F(q1) * F(q2) - F(k) * F(k))
    stable = float(R.stable_r(np.float64(k), np.float64(q1), np.float64(q2), 1.0))
    naive = float(R.naive_r(np.float64(k), np.float64(q1), np.float64(q2), 1.0))
    err_s = abs(F(stable) - exact) / exact
    err_n = abs(F(naive) - exact) / exact
    assert err_s < 1e-14, float(err_s)
    assert err_n > 1e-11, float(err_n)


def test_serial_accepts_the_new_topologies_and_rejects_bad_ones():
    for acts in ([stax.Erf()], [stax.Erf(), stax.Relu()], [stax.LeakyRelu(0.2), stax.Abs(), stax.ABRelu(-0.5, 1.5)]):
        layers = [stax.Dense(64)]
        for a in acts:
            layers += [a, stax.Dense(64)]
        _, _, kf = stax.serial(*layers)
        assert len(kf.activations) == len(acts) and not kf.all_relu
        assert isinstance(kf._arch(), _lib.NngpArchAct)
    _, _, kf = stax.serial(stax.Dense(8), stax.Erf(0.5, 2.0, 0.1), stax.Dense(8), stax.Relu(do_stabilize=True), stax.Dense(1))
    assert kf.activations == (("erf", 0.5, 2.0, 0.1), ("relu",))
    for bad in ([stax.Dense(8), stax.Erf()], [stax.Erf(), stax.Dense(8)], [stax.Dense(8), stax.Erf(), stax.Relu(), stax.Dense(1)],
                [stax.Dense(8), stax.Dense(8)]):
        with pytest.raises(NotImplementedError):
            stax.serial(*bad)
    with pytest.raises(ValueError):
        stax.Erf(float("nan"))
    with pytest.raises(ValueError):
        stax.LeakyRelu(float("inf"))


def test_relu_archs_keep_the_old_struct():
    for act in (stax.Relu(), stax.ABRelu(0, 1), stax.LeakyRelu(0.0), stax.Relu(do_stabilize=True)):
        _, _, kf = stax.serial(stax.Dense(8, W_std=1.1, b_std=0.2), act, stax.Dense(1))
        assert kf.all_relu and kf.activations == (("relu",),)
        arch = kf._arch()
        assert type(arch) is _lib.NngpArch
        assert arch.n_dense == 2 and arch.w_std[0] == 1.1 and arch.b_std[0] == 0.2


def test_arch_act_ctypes_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nngp_activations.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(nngp_arch_act), offsetof(nngp_arch_act, base),'
                   ' offsetof(nngp_arch_act, act), offsetof(nngp_arch_act, p), sizeof(((nngp_arch_act*)0)->p[0]),'
                   ' sizeof(nngp_arch)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.NngpArchAct
    want = [ctypes.sizeof(A), A.base.offset, A.act.offset, A.p.offset, 3 * ctypes.sizeof(ctypes.c_double),
            ctypes.sizeof(_lib.NngpArch)]
    assert got == want
    arch = _lib.make_arch_act([1.0, 2.0, 3.0], [0.0, 0.5, 0.0], [("erf", 0.5, 2.0, 0.1), ("abrelu", -1.0, 1.0)])
    assert list(arch.act)[:2] == [_lib.ACT_ERF, _lib.ACT_ABRELU] and arch.base.n_dense == 3
    assert list(arch.p[0]) == [0.5, 2.0, 0.1] and list(arch.p[1])[:2] == [-1.0, 1.0]
    with pytest.raises(ValueError):
        _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [])


def test_train_cli_knows_the_activations():
    from nngp_src_amd import train, active_train
    args = train.make_parser().parse_args(["--activation", "leaky_relu", "--leaky_alpha", "0.2", "--n_relu", "2"])
    _, _, kf = train.kernel_fn_from_args(args)
    assert kf.activations == (("abrelu", 0.2, 1.0),) * 2
    args = active_train.parse_args(["--activation", "erf"])
    assert train.kernel_fn_from_args(args)[2].activations == (("erf", 1.0, 1.0, 0.0),)
    assert train.kernel_fn_from_args(train.make_parser().parse_args([]))[2].all_relu
