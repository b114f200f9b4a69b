"""Per-feature input relevances on the MI355X (include/nngp_ard.h; mll.py, loo.py, stax.py, model.py) against the NumPy oracle
of nngp_ard_reference.py (forward-mode tangents seeded at the input, scipy Cholesky).  The gates are those of
test_gpu_nngp_mll.py / test_gpu_nngp_loo.py: value 1e-9 relative, every gradient component within 1e-8 of the larger of its two
cancelling halves, tr dK/ds_k 1e-12 relative."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nngp_ard_reference as A  # noqa: E402
import nngp_mll_reference as R  # noqa: E402
from nngp_src_amd import _lib, loo, mll, stax, synth, train as train_cli  # noqa: E402
from nngp_src_amd.model import GPModel  # noqa: E402
from test_gpu_nngp_mll import _forest, _rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _rows(golden_dir, n, d=20):
    if d != 20:
        x, y = synth.synthetic_queries(n, d, seed=n)
        return x / 1000.0, y.reshape(-1)
    f = _forest(golden_dir)
    x = np.concatenate([f["X_train"], f["X_test"]])[:n] / 1000.0
    y = np.concatenate([f["Y_train"], f["Y_test"]])[:n].reshape(-1)
    return x, y


def _relevances(d, seed, zero=True):
    """Log-normal relevances, one of them exactly 0.  With d = 3 only features 0 and 1 carry data (synth.synthetic_queries: one
    range pair, the third column is empty): a zero on either would leave one-dimensional inputs, every pair of rows at angle 0
    exactly, where q q' - k^2 is rounding noise under a square root in the oracle as on the device.  There the zero goes on the
    empty feature."""
    s = np.exp(np.random.default_rng(seed).normal(size=d))
    if zero:
        s[d // 2 if d > 3 else d - 1] = 0.0
    return s


def _check_s(m, got_gs, ref, loo_form=False):
    gate = 1e-8 * np.maximum(np.abs(ref["half1_s"]), np.abs(ref["half2_s"]))
    print("grad_s error / halves' scale", np.abs(got_gs - ref["grad_s"]) / np.where(gate > 0, gate * 1e8, 1.0))  # gate 1e-8
    assert np.all(np.isfinite(got_gs))
    assert np.all(np.abs(got_gs - ref["grad_s"]) <= gate), (got_gs, ref["grad_s"], gate)
    t = m.ard_terms()
    np.testing.assert_allclose(t["tr_dk"], ref["tr_dk_s"], rtol=1e-12, atol=0)
    combined = -(t["half1"] + t["half2"]) if loo_form else -0.5 * t["half1"] + 0.5 * t["half2"]
    np.testing.assert_allclose(combined, got_gs, rtol=0, atol=0)


def _check_mll(m, nlml, g, gs, ref):
    print("nlml rel %.3e" % _rel(nlml, ref["nlml"]))
    assert _rel(nlml, ref["nlml"]) <= 1e-9, (nlml, ref["nlml"])
    gate = 1e-8 * np.maximum(np.abs(ref["quad"]), np.abs(ref["trace"]))
    assert np.all(np.abs(g - ref["grad"]) <= gate), (g, ref["grad"], gate)
    t = m.terms()
    assert _rel(t["tr_k"], ref["tr_k"]) <= 1e-12
    np.testing.assert_allclose(t["tr_dk"], ref["tr_dk"], rtol=1e-12, atol=0)
    _check_s(m, gs, ref)


CASES = [  # n, d, n_dense, W_std, b_std, activation, absolute
    (127, 20, 2, 1.0, 0.0, ("relu",), False),      # two tile rows, ragged
    (193, 33, 3, 1.5, 0.05, ("relu",), True),      # ten tiles: the XCD deal has a remainder; one feature past the 32-wide chunk
    (600, 70, 5, 1.2, 0.05, ("relu",), False),     # the NLC = 8 instantiation, three chunks
    (300, 3, 9, 1.3, 0.0, ("relu",), True),        # the NLC = 16 instantiation
    (1000, 20, 4, 1.0, 0.05, ("abrelu", 0.1, 1.0), False),
]


@pytest.mark.parametrize("n,d,n_dense,w_std,b_std,act,absolute", CASES)
def test_nlml_and_relevance_gradient_against_the_oracle(golden_dir, n, d, n_dense, w_std, b_std, act, absolute):
    x, y = _rows(golden_dir, n, d)
    w, b, acts = [w_std] * n_dense, [b_std] * n_dense, [act] * (n_dense - 1)
    s = _relevances(d, n)
    ref = A.Oracle(x, y).full(*R.variances(w, b), acts, 1e-3, s, absolute)
    m = mll.NNGPMarginalLikelihood(n, d, ard=True).set_train(x, y)
    nlml, g, gs = m.evaluate((w, b, acts), 1e-3, absolute, relevance=s)
    _check_mll(m, nlml, g, gs, ref)
    # bit-identical repeats; the value alone equals the value with the gradients
    nlml2, g2, gs2 = m.evaluate((w, b, acts), 1e-3, absolute, relevance=s)
    assert nlml2 == nlml and np.array_equal(g2, g) and np.array_equal(gs2, gs)
    nlml3, none, none_s = m.evaluate((w, b, acts), 1e-3, absolute, with_grad=False, relevance=s)
    assert none is None and none_s is None and nlml3 == nlml
    m.close()


def test_unit_relevances_give_the_bits_of_the_existing_entry_point(golden_dir):
    x, y = _rows(golden_dir, 600)
    w, b, acts = [1.2, 0.9, 1.1], [0.05, 0.1, 0.02], [("relu",), ("abrelu", 0.1, 1.0)]
    plain = mll.NNGPMarginalLikelihood(600, 20).set_train(x, y)
    nlml0, g0 = plain.evaluate((w, b, acts), 1e-3)
    m = mll.NNGPMarginalLikelihood(600, 20, ard=True).set_train(x, y)
    nlml, g, gs = m.evaluate((w, b, acts), 1e-3, relevance=np.ones(20))
    assert nlml == nlml0 and np.array_equal(g, g0)
    # the handle with relevances reserved still serves the entry point without them, before and after
    nlml1, g1 = m.evaluate((w, b, acts), 1e-3)
    assert nlml1 == nlml0 and np.array_equal(g1, g0)
    lo0 = loo.LeaveOneOut(600, 20).set_train(x, y)
    lo = loo.LeaveOneOut(600, 20, ard=True).set_train(x, y)
    for obj in ("nlpd", "mse"):
        v0, gl0 = lo0.evaluate((w, b, acts), 1e-3, objective=obj)
        v, gl, _ = lo.evaluate((w, b, acts), 1e-3, objective=obj, relevance=np.ones(20))
        assert v == v0 and np.array_equal(gl, gl0)
    for h in (plain, m, lo0, lo):
        h.close()


def test_zero_and_duplicated_rows(golden_dir):
    """b_0 = 0 with zero rows (q = 0) and duplicated rows (s = 0 off the diagonal): a finite grad_s, equal to the oracle's."""
    x, y = _rows(golden_dir, 600)
    x[5] = 0.0
    x[77] = 0.0
    x[300:310] = x[100:110]
    w, b, acts = [1.0, 1.3, 1.1], [0.0, 0.05, 0.0], [("relu",), ("abrelu", 0.1, 1.0)]
    s = _relevances(20, 3)
    ref = A.Oracle(x, y).full(*R.variances(w, b), acts, 1e-3, s)
    m = mll.NNGPMarginalLikelihood(600, 20, ard=True).set_train(x, y)
    nlml, g, gs = m.evaluate((w, b, acts), 1e-3, relevance=s)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(gs))
    _check_mll(m, nlml, g, gs, ref)
    m.close()


def test_device_gradient_against_finite_differences_of_the_device_nlml(golden_dir):
    x, y = _rows(golden_dir, 1000)
    w, b, acts = [1.2, 0.9, 1.1], [0.05, 0.1, 0.02], [("relu",), ("relu",)]
    s = _relevances(20, 11, zero=False)
    m = mll.NNGPMarginalLikelihood(1000, 20, ard=True).set_train(x, y)
    _, g, gs = m.evaluate((w, b, acts), 1e-3, relevance=s)
    t, ts = m.terms(), m.ard_terms()
    for k in range(20):
        h = 1e-3 * s[k]

        def f(dt):
            r = s.copy()
            r[k] += dt
            return m.evaluate((w, b, acts), 1e-3, with_grad=False, relevance=r)[0]

        fd = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        scale = max(abs(ts["half1"][k]), abs(ts["half2"][k]))
        print(k, abs(fd - gs[k]) / scale)
        assert abs(fd - gs[k]) <= 1e-6 * scale, (k, fd, gs[k], scale)
    # a common factor on s is sigma_w,0^2: sum_k s_k g_k = v_0 g_v0
    scale = max(abs(t["quad"][0]), abs(t["trace"][0]))
    print("identity", abs(np.sum(s * gs) - w[0] ** 2 * g[0]) / scale)
    assert abs(np.sum(s * gs) - w[0] ** 2 * g[0]) <= 1e-8 * scale
    m.close()


@pytest.mark.parametrize("n,d,absolute", [(193, 33, True), (600, 20, False)])
def test_leave_one_out_objectives_against_the_oracle(golden_dir, n, d, absolute):
    x, y = _rows(golden_dir, n, d)
    w, b, acts = [1.2, 0.9, 1.1], [0.05, 0.1, 0.02], [("relu",), ("abrelu", 0.1, 1.0)]
    s = _relevances(d, n)
    m = loo.LeaveOneOut(n, d, ard=True).set_train(x, y)
    for obj in ("nlpd", "mse"):
        ref = A.Oracle(x, y, obj).full(*R.variances(w, b), acts, 1e-3, s, absolute)
        val, g, gs = m.evaluate((w, b, acts), 1e-3, absolute, objective=obj, relevance=s)
        print(obj, "value rel %.3e" % _rel(val, ref["value"]))
        assert _rel(val, ref["value"]) <= 1e-9, (val, ref["value"])
        scale = np.maximum(np.abs(ref["half1"]), np.abs(ref["half2"]))
        assert np.all(np.abs(g - ref["grad"]) <= 1e-8 * scale), (g, ref["grad"], scale)
        _check_s(m, gs, ref, loo_form=True)
        val2, g2, gs2 = m.evaluate((w, b, acts), 1e-3, absolute, objective=obj, relevance=s)
        assert val2 == val and np.array_equal(g2, g) and np.array_equal(gs2, gs)
        val3, _, _ = m.evaluate((w, b, acts), 1e-3, absolute, objective=obj, relevance=s, with_grad=False)
        assert _rel(val3, ref["value"]) <= 1e-9  # the value alone skips A^-1 (b from the rows of L^-T), as without relevances
    # the NTK: the value with relevances, no gradient
    with pytest.raises(ValueError):
        m.evaluate((w, b, acts), 1e-3, objective="mse", get="ntk", relevance=s)
    arch = _lib.make_arch_act(w, b, acts)
    sv = (ctypes.c_double * d)(*s)
    out, gbuf = ctypes.c_double(), (ctypes.c_double * d)()
    lib = _lib.load()
    assert lib.nngp_mll_loo_evaluate_ard(m._h, ctypes.byref(arch), _lib.GET_NTK, sv, 1e-3, 0, _lib.LOO_MSE, ctypes.byref(out), None,
                                         gbuf, _lib.stream_ptr()) == -2
    val, none, none_s = m.evaluate((w, b, acts), 1e-3, objective="mse", get="ntk", relevance=s, with_grad=False)
    plain = loo.LeaveOneOut(n, d, "mse", "ntk").set_train(A.scaled(x, s), y)
    assert none is None and none_s is None and _rel(val, plain.evaluate((w, b, acts), 1e-3, with_grad=False)[0]) <= 1e-12
    plain.close()
    m.close()


def test_errors(golden_dir):
    lib = _lib.load()
    x, y = _rows(golden_dir, 300)
    w, b, acts = [1.0, 1.0], [0.0, 0.0], [("relu",)]
    arch = _lib.make_arch_act(w, b, acts)
    out, gs = ctypes.c_double(), (ctypes.c_double * 20)()

    def call(h, s, a=arch):
        return lib.nngp_mll_evaluate_ard(h._h, ctypes.byref(a), (ctypes.c_double * 20)(*s), 1e-3, 0, ctypes.byref(out), None, gs,
                                         _lib.stream_ptr())

    one = np.ones(20)
    m = mll.NNGPMarginalLikelihood(300, 20).set_train(x, y)
    assert call(m, one) == -2  # no nngp_mll_reserve_ard yet
    with pytest.raises(_lib.NngpError, match="reserve_ard"):
        m.evaluate((w, b, acts), 1e-3, relevance=one)
    ref = A.Oracle(x, y).full(*R.variances(w, b), acts, 1e-3, _relevances(20, 5))
    m.reserve_ard()
    count = lib.nngp_alloc_count()

    def usable():
        nlml, g, got = m.evaluate((w, b, acts), 1e-3, relevance=_relevances(20, 5))
        _check_mll(m, nlml, g, got, ref)

    usable()
    for bad in (-1.0, float("nan"), float("inf")):
        s = one.copy()
        s[7] = bad
        assert call(m, s) == -2
        usable()
    with pytest.raises(ValueError):  # a wrong length never reaches the library
        m.evaluate((w, b, acts), 1e-3, relevance=np.ones(19))
    erf = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])
    assert call(m, one, erf) == -2
    usable()
    assert lib.nngp_alloc_count() == count  # nothing is allocated after reserve_ard
    m.close()


@pytest.mark.parametrize("module,groups", [("mll", None), ("mll", "pairs"), ("loo", None)])
def test_tuning_matches_the_oracle_driven_run(golden_dir, module, groups):
    x, y = _rows(golden_dir, 300)
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.1, b_std=0.05), stax.Relu(), stax.Dense(1, W_std=1.0, b_std=0.05))
    tune = mll.tune_hyperparameters if module == "mll" else loo.tune_hyperparameters
    ev = A.Oracle(x, y, None if module == "mll" else "nlpd")
    kf_t, lam_t, hist = tune(kf, x, y, steps=10, lr=0.05, report=None, ard=True, ard_groups=groups)
    kf_o, lam_o, hist_o = tune(kf, x, y, steps=10, lr=0.05, report=None, ard=True, ard_groups=groups, evaluator=ev)
    np.testing.assert_allclose(kf_t.w_std, kf_o.w_std, rtol=1e-8)
    np.testing.assert_allclose(kf_t.b_std, kf_o.b_std, rtol=1e-8)
    np.testing.assert_allclose(kf_t.input_scale, kf_o.input_scale, rtol=1e-8)
    assert _rel(lam_t, lam_o) <= 1e-8
    np.testing.assert_allclose(hist, hist_o, rtol=1e-9)
    assert hist[-1] < hist[0]
    assert kf_t.w_std[0] == 1.1  # held fixed: a common factor on the relevances stands for it
    assert kf_t.input_scale.shape == (20,) and len(set(kf_t.input_scale)) > 1
    if groups == "pairs":
        assert np.array_equal(kf_t.input_scale[0::2], kf_t.input_scale[1::2])
        assert len(set(kf_t.input_scale[0::2])) > 1


def _scaled_kernel_fn():
    c = np.sqrt(_relevances(20, 2))
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.2, b_std=0.05), stax.Relu(), stax.Dense(1))
    xt = synth.synthetic_queries(64, 20, seed=1)[0] / 1000.0
    return kf, c, xt


def test_kernel_fn_with_an_input_scale(golden_dir):
    x, _ = _rows(golden_dir, 300)
    kf, c, xt = _scaled_kernel_fn()
    kfs = kf.with_input_scale(c)
    assert kf.input_scale is None and np.array_equal(kfs.input_scale, c)
    for get in ("nngp", "ntk"):
        assert np.array_equal(kfs(xt, x, get), kf(xt * c, x * c, get))
    assert np.array_equal(kfs(xt, None, "nngp"), kf(xt * c, None, "nngp"))
    with pytest.raises(ValueError):
        kfs(xt[:, :19], None, "nngp")


def test_model_with_an_input_scale_fit_predict_save_load(golden_dir, tmp_path):
    """The scaling is the same IEEE multiply on the device as on the host, so a model with input_scale equals a model fitted on
    the scaled rows bit for bit.  Save and load keep the scale; a checkpoint without one is written and read as before."""
    x, y = _rows(golden_dir, 400)
    kf, c, xt = _scaled_kernel_fn()
    ms = GPModel(400, 20, kf.w_std, kf.b_std, input_scale=c).fit(x, y)
    mp = GPModel(400, 20, kf.w_std, kf.b_std).fit(x * c, y)
    mean_s, var_s = ms.predict(xt, cov="diag")
    mean_p, var_p = mp.predict(xt * c, cov="diag")
    np.testing.assert_allclose(mean_s, mean_p, rtol=1e-12, atol=0)
    np.testing.assert_allclose(var_s, var_p, rtol=1e-12, atol=0)
    assert np.array_equal(mean_s, mean_p) and np.array_equal(var_s, var_p)
    assert np.array_equal(ms.select_pool(xt, 8), mp.select_pool(xt * c, 8))
    with pytest.raises(ValueError):
        GPModel(400, 20, kf.w_std, kf.b_std, input_scale=c[:19])
    ms.save(str(tmp_path / "scaled.npz"))
    back = GPModel.load(str(tmp_path / "scaled.npz"))
    assert np.array_equal(back.input_scale, c)
    assert np.array_equal(back.predict(xt, cov=False), ms.predict(xt, cov=False))
    plain = GPModel(400, 20, kf.w_std, kf.b_std).fit(x, y)
    plain.save(str(tmp_path / "plain.npz"))
    z = np.load(str(tmp_path / "plain.npz"))
    assert "input_scale" not in z.files and str(z["format"]) == "nngp-src_amd GPModel v1"
    again = GPModel.load(str(tmp_path / "plain.npz"))
    assert again.input_scale is None
    again.save(str(tmp_path / "plain2.npz"))
    # the same fields with the same bytes (the zip container around them carries the time of writing, so the files as a whole
    # are not compared)
    z2 = np.load(str(tmp_path / "plain2.npz"))
    assert z.files == z2.files
    for k in z.files:
        assert z[k].dtype == z2[k].dtype and z[k].shape == z2[k].shape and z[k].tobytes() == z2[k].tobytes(), k
    for h in (ms, mp, back, plain, again):
        h.close()


def test_model_with_an_input_scale_fit_append_predict(golden_dir):
    """fit -> append -> predict against a model fitted and extended on the scaled rows: equal bit for bit.  1050 + 150 rows, the
    size range test_gpu_api.py appends in."""
    x, y = _rows(golden_dir, 1200)
    kf, c, xt = _scaled_kernel_fn()
    ms = GPModel(1200, 20, kf.w_std, kf.b_std, input_scale=c).fit(x[:1050], y[:1050])
    mp = GPModel(1200, 20, kf.w_std, kf.b_std).fit(x[:1050] * c, y[:1050])
    ms.append(x[1050:], y[1050:])
    mp.append(x[1050:] * c, y[1050:])
    mean_s, var_s = ms.predict(xt, cov="diag")
    mean_p, var_p = mp.predict(xt * c, cov="diag")
    np.testing.assert_allclose(mean_s, mean_p, rtol=1e-12, atol=0)
    np.testing.assert_allclose(var_s, var_p, rtol=1e-12, atol=0)
    assert np.array_equal(mean_s, mean_p) and np.array_equal(var_s, var_p)
    ms.close()
    mp.close()


def test_train_cli_tune_ard_on_forest_queries(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "forest_queries.npz"))
    g = {k: g[k] for k in g.files}
    sent = np.iinfo(np.int32).min
    names = "ABCDEFGHIJ"
    per_file = 300
    for fi, fn in enumerate(g["files"]):
        with open(tmp_path / str(fn), "w") as fh:
            for i in range(fi * per_file, (fi + 1) * per_file):
                preds = ["%s,%d,%d" % (names[c], g["bounds"][i, c, 0], g["bounds"][i, c, 1]) for c in range(10)
                         if g["bounds"][i, c, 0] != sent]
                fh.write("#".join(preds) + "@%d\n" % g["cards"][i])
    args = train_cli.make_parser().parse_args(["--kernel_type", "nngp", "--query_path", str(tmp_path), "--max_num_train", "256",
                                               "--max_num_test", "100", "--tune_hyper", "3", "--tune_ard", "--ard_groups", "pairs"])
    args.join_query = False
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    text = buf.getvalue()
    for i in range(3):
        assert "Step: %d, neg marginal likelihood:" % i in text
    for needle in ("Tuned W_std", "Tuned relevances=[", "Kernel construction in", "Mean Square Error:", "Predict Result Profile of"):
        assert needle in text, needle
    assert np.all(np.isfinite(res["pred_mean"]))
