"""Per-feature input relevances without a GPU: the NumPy oracle against finite differences of its own value and against the
oracle without relevances, the raw vector of the tuning loop with groups, KernelFn.with_input_scale, and a tuning run driven by
the oracle."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_ard_reference as A  # noqa: E402
import nngp_loo_reference as L  # noqa: E402
import nngp_mll_reference as R  # noqa: E402
from nngp_src_amd import _lib, dist2d, loo, mll, shard32, stax, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n, d, seed=0):
    x, y = synth.synthetic_queries(n, d, seed=seed)
    return x / 1000.0, y.reshape(-1)


NETS = [
    ([1.0, 1.0], [0.0, 0.0], [("relu",)]),
    ([1.2, 0.9, 1.1], [0.05, 0.1, 0.02], [("relu",), ("abrelu", 0.1, 1.0)]),
    ([1.3, 0.8, 1.1, 1.0], [0.0, 0.05, 0.0, 0.1], [("abrelu", -1.0, 1.0), ("relu",), ("relu",)]),
]


@pytest.mark.parametrize("objective", [None, "nlpd", "mse"])
@pytest.mark.parametrize("absolute", [False, True])
def test_oracle_gradient_against_finite_differences(objective, absolute):
    x, y = _data(90, 8, seed=3)
    s = np.exp(np.random.default_rng(1).normal(size=8))
    s[2] = 0.0
    for w, b, acts in NETS:
        v, c = R.variances(w, b)
        o = A.Oracle(x, y, objective)
        f = o.full(v, c, acts, 1e-3, s, absolute)
        assert np.all(np.isfinite(f["grad_s"]))
        for k in range(8):
            if s[k] == 0.0:
                continue  # a central difference would need s_k < 0
            h = 1e-3 * s[k]

            def val(dt):
                r = s.copy()
                r[k] += dt
                return o.value(v, c, acts, 1e-3, r, absolute)

            fd = (-val(2 * h) + 8 * val(h) - 8 * val(-h) + val(-2 * h)) / (12 * h)
            scale = max(abs(f["half1_s"][k]), abs(f["half2_s"][k]))
            assert abs(fd - f["grad_s"][k]) <= 1e-6 * scale, (k, fd, f["grad_s"][k], scale)
        # a common factor on s is sigma_w,0^2
        halves = (f["quad"], f["trace"]) if objective is None else (f["half1"], f["half2"])
        assert abs(np.sum(s * f["grad_s"]) - v[0] * f["grad"][0]) <= 1e-8 * max(abs(halves[0][0]), abs(halves[1][0]))
        np.testing.assert_allclose(np.sum(s * f["tr_dk_s"]), v[0] * f["tr_dk"][0], rtol=1e-12)


def test_zero_relevance_against_a_one_sided_difference():
    x, y = _data(60, 6, seed=4)
    s = np.array([1.0, 0.0, 2.0, 0.5, 1.5, 0.7])
    w, b, acts = NETS[1]
    v, c = R.variances(w, b)
    o = A.Oracle(x, y)
    f = o.full(v, c, acts, 1e-3, s)

    def val(t):
        r = s.copy()
        r[1] = t
        return o.value(v, c, acts, 1e-3, r)

    h = 2e-5
    fd = (-25 * val(0.0) + 48 * val(h) - 36 * val(2 * h) + 16 * val(3 * h) - 3 * val(4 * h)) / (12 * h)  # five points, from the right
    assert abs(fd - f["grad_s"][1]) <= 1e-6 * max(abs(f["half1_s"][1]), abs(f["half2_s"][1]))


def test_unit_relevances_equal_the_oracles_without_them():
    x, y = _data(70, 6, seed=2)
    w, b, acts = NETS[1]
    v, c = R.variances(w, b)
    f1 = A.Oracle(x, y).full(v, c, acts, 1e-3, np.ones(6))
    f0 = R.Oracle(x, y).full(v, c, acts, 1e-3)
    assert f1["nlml"] == f0["nlml"] and np.array_equal(f1["grad"], f0["grad"])
    for obj in ("nlpd", "mse"):
        g1 = A.Oracle(x, y, obj).full(v, c, acts, 1e-3, np.ones(6))
        g0 = L.Oracle(x, y, obj).full(v, c, acts, 1e-3)
        assert g1["value"] == g0["value"] and np.array_equal(g1["grad"], g0["grad"])


def test_raw_vector_with_groups_and_fixed_first_layer():
    index, ng = mll.relevance_groups("pairs", 6)
    assert list(index) == [0, 0, 1, 1, 2, 2] and ng == 3
    assert list(mll.relevance_groups(None, 3)[0]) == [0, 1, 2]
    assert list(mll.relevance_groups([7, 3, 7, 3], 4)[0]) == [0, 1, 0, 1]
    with pytest.raises(ValueError):
        mll.relevance_groups([0, 1], 3)
    with pytest.raises(ValueError):
        mll.relevance_groups("triples", 3)
    p = mll._Params([1.1, 0.9], [0.05, 0.0], 1e-3, ard_index=index, relevance_init=[2.0, 2.0, 1.0, 1.0, 0.5, 0.5])
    # log sigma_w^2 of layer 1 only, the free bias of layer 0, three groups, log lambda
    np.testing.assert_allclose(p.raw0, [np.log(0.81), np.log(0.0025), np.log(2.0), 0.0, np.log(0.5), np.log(1e-3)])
    raw = p.raw0 + np.array([0.3, -0.2, 0.1, 0.2, -0.4, 0.5])
    w, b, lam, clamped = p.unpack(raw)
    assert w[0] == 1.1 and b[1] == 0.0 and not clamped  # W_std of Dense layer 0 is held fixed
    np.testing.assert_allclose([w[1], b[0], lam], [np.exp(0.5 * raw[0]), np.exp(0.5 * raw[1]), np.exp(raw[5])])
    s = p.relevance(raw)
    np.testing.assert_allclose(s, np.exp(raw[2:5])[[0, 0, 1, 1, 2, 2]])
    g = np.array([10.0, 20.0, 30.0, 40.0, 50.0])
    gs = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    np.testing.assert_allclose(p.grad_raw(g, raw, gs), [30.0 * w[1] ** 2, 20.0 * b[0] ** 2, (1.0 + 2.0) * s[0], (3.0 + 4.0) * s[2],
                                                        (5.0 + 6.0) * s[4], 50.0 * lam])
    with pytest.raises(ValueError):
        mll._Params([1.0, 1.0], [0.0, 0.0], 1e-3, ard_index=index, relevance_init=[1.0, 2.0, 1.0, 1.0, 1.0, 1.0])
    # without relevances the vector is what it was
    p0 = mll._Params([1.1, 0.9], [0.05, 0.0], 1e-3)
    np.testing.assert_allclose(p0.raw0, [np.log(1.21), np.log(0.81), np.log(0.0025), np.log(1e-3)], rtol=0, atol=1e-15)
    assert p0.relevance(p0.raw0) is None


def test_with_input_scale_validation():
    _, _, kf = stax.serial(stax.Dense(8, W_std=1.2, b_std=0.1), stax.Abs(), stax.Dense(1))
    assert kf.input_scale is None
    ks = kf.with_input_scale([1.0, 0.0, 2.5])
    assert ks is not kf and kf.input_scale is None and np.array_equal(ks.input_scale, [1.0, 0.0, 2.5])
    assert (ks.w_std, ks.b_std, ks.activations) == (kf.w_std, kf.b_std, kf.activations)
    assert ks.with_input_scale(None).input_scale is None
    for bad in ([1.0, -0.1], [1.0, float("nan")], [float("inf")], [[1.0, 2.0]], []):
        with pytest.raises(ValueError):
            kf.with_input_scale(bad)
    from nngp_src_amd import batch
    assert np.array_equal(batch(ks, batch_size=4, device_count=0).input_scale, ks.input_scale)
    assert batch(kf, batch_size=4, device_count=0).input_scale is None
    with pytest.raises(NotImplementedError, match="input_scale"):
        dist2d.HipOps(kf.w_std, kf.b_std, input_scale=ks.input_scale)
    with pytest.raises(NotImplementedError, match="input_scale"):
        shard32.HipRowOps(10, 3, kf.w_std, kf.b_std, input_scale=ks.input_scale)


@pytest.mark.parametrize("module,objective,groups", [(mll, None, None), (mll, None, "pairs"), (loo, "nlpd", None)])
def test_tune_with_the_oracle_evaluator_lowers_the_objective(module, objective, groups):
    x, y = _data(80, 6, seed=5)
    _, _, kf = stax.serial(stax.Dense(16, W_std=1.1), stax.LeakyRelu(0.1), stax.Dense(1))
    kw = {} if objective is None else {"objective": objective}
    kf_t, lam, hist = module.tune_hyperparameters(kf, x, y, steps=8, lr=0.05, b_std_init=0.05, report=None, ard=True,
                                                  ard_groups=groups, evaluator=A.Oracle(x, y, objective, block=40), **kw)
    assert len(hist) == 8 and hist[-1] < hist[0]
    assert kf_t.w_std[0] == 1.1 and kf_t.w_std[1] != 1.0 and lam > 0.0
    assert kf_t.activations == (("abrelu", 0.1, 1.0),)
    assert kf_t.input_scale.shape == (6,) and np.all(kf_t.input_scale > 0.0) and len(set(kf_t.input_scale)) > 1
    if groups == "pairs":
        assert np.array_equal(kf_t.input_scale[0::2], kf_t.input_scale[1::2])
    # without ard the call and its result are what they were: no input_scale, every W_std free
    kf_p, _, hist_p = module.tune_hyperparameters(kf, x, y, steps=2, lr=0.05, b_std_init=0.05, report=None,
                                                  evaluator=A.Oracle(x, y, objective, block=40), **kw)
    assert kf_p.input_scale is None and kf_p.w_std[0] != 1.1 and len(hist_p) == 2


def test_train_cli_flags():
    from nngp_src_amd import train
    a = train.make_parser().parse_args([])
    assert a.tune_ard is False and a.ard_groups == "none"
    a = train.make_parser().parse_args(["--tune_hyper", "5", "--tune_ard", "--ard_groups", "pairs"])
    assert (a.tune_hyper, a.tune_ard, a.ard_groups) == (5, True, "pairs")


def test_ard_symbols_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_ard.h")) as f:
        declared = set(re.findall(r"\bint (nngp_mll_\w+)\(", f.read()))
    assert declared == set(_lib.ARD_ABI_SYMBOLS)
    lib = _lib.load()
    for name in _lib.ARD_ABI_SYMBOLS:
        assert hasattr(lib, name), name


class _StubHandle:
    """The evaluator interface of mll.NNGPMarginalLikelihood / loo.LeaveOneOut on the NumPy oracle: what the one-shot functions
    and the tuning loop do with a kernel_fn's input_scale can then be checked without a GPU."""

    def __init__(self, n_cap, d, objective=None, get="nngp", ard=False):
        self.objective, self.reserved, self.d = objective, bool(ard), d

    def reserve_ard(self):
        self.reserved = True
        return self

    def set_train(self, x, y):
        self.oracle = A.Oracle(x, y, self.objective, block=64)
        return self

    def evaluate(self, kernel_fn_or_params, diag_reg=1e-3, absolute=False, with_grad=True, relevance=None, **kw):
        assert relevance is None or self.reserved
        return self.oracle.evaluate(mll._arch_of(kernel_fn_or_params), diag_reg, absolute, with_grad, relevance=relevance)

    def close(self):
        self.closed = True


def test_one_shot_functions_and_tuning_take_the_input_scale(monkeypatch):
    monkeypatch.setattr(mll, "NNGPMarginalLikelihood", _StubHandle)
    monkeypatch.setattr(loo, "LeaveOneOut", lambda n, d, objective="nlpd", get="nngp", ard=False: _StubHandle(n, d, objective, get, ard))
    x, y = _data(60, 6, seed=7)
    c = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 0.7])
    _, _, kf = stax.serial(stax.Dense(16, W_std=1.1, b_std=0.05), stax.Relu(), stax.Dense(1))
    kfs = kf.with_input_scale(c)
    nlml, g = mll.marginal_likelihood(kfs, x, y)
    nlml0, g0 = mll.marginal_likelihood(kf, x * c, y)
    assert nlml == nlml0 and g["w_std2"] == g0["w_std2"] and g["diag_reg"] == g0["diag_reg"]
    assert len(g["relevance"]) == 6 and "relevance" not in g0 and set(g0) == {"w_std2", "b_std2", "diag_reg"}
    assert mll.marginal_likelihood(kfs, x, y, with_grad=False) == nlml0
    val, gl = loo.loo_objective(kfs, x, y, objective="mse")
    val0, gl0 = loo.loo_objective(kf, x * c, y, objective="mse")
    assert val == val0 and gl["w_std2"] == gl0["w_std2"] and len(gl["relevance"]) == 6
    # (the oracle's value-only path takes b from the rows of L^-1 instead of A^-1: the same number to rounding)
    assert abs(loo.loo_objective(kfs, x, y, objective="mse", with_grad=False) - val0) <= 1e-12 * abs(val0)
    with pytest.raises(ValueError):
        mll.marginal_likelihood(kf.with_input_scale(c[:5]), x, y)
    # tuning without ard keeps the scale as it is; with ard it is the start of the relevances
    kf_t, lam_t, hist = mll.tune_hyperparameters(kfs, x, y, steps=3, report=None)
    kf_0, lam_0, hist_0 = mll.tune_hyperparameters(kf, x * c, y, steps=3, report=None)
    assert np.array_equal(kf_t.input_scale, c) and kf_0.input_scale is None
    assert hist == hist_0 and kf_t.w_std == kf_0.w_std and lam_t == lam_0
    c1 = np.where(c > 0.0, c, 1.0)  # tuning log s needs s > 0
    for module, kw in ((mll, {}), (loo, {"objective": "mse"})):
        _, _, hist_a = module.tune_hyperparameters(kf.with_input_scale(c1), x, y, steps=2, report=None, ard=True, **kw)
        _, _, hist_b = module.tune_hyperparameters(kf, x, y, steps=2, report=None, ard=True, relevance_init=c1 * c1, **kw)
        assert hist_a == hist_b
