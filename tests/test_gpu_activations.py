"""Erf / ABRelu / LeakyRelu / Abs networks on the MI355X (-m gpu): the kernel build through nngp_kernel_build_act against the
float64 restatement (activation_reference.py), the diagonal entry point, the fit / predict / serving / append stack of a model
created by nngp_model_create_act, checkpoints, and the rule that no path computes ReLU for a network that asked otherwise."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import activation_reference as R
import gpu_util as G
from nngp_src_amd import _lib, stax, synth, predict
from nngp_src_amd.model import GPModel

pytestmark = pytest.mark.gpu

ACTS = {
    "erf": ("erf", 1.0, 1.0, 0.0),
    "erf_abc": ("erf", 0.8, 1.7, 0.3),
    "leaky": ("abrelu", 0.1, 1.0),
    "abs": ("abrelu", -1.0, 1.0),
    "abrelu": ("abrelu", -0.3, 2.0),
}


def _arch(acts, w=1.1, b=0.0):
    nd = len(acts) + 1
    return [w] * nd, [b] * nd, list(acts)


build_act, diag_act = G.build_act, G.diag_act  # (shared with test_gpu_kernel_angles.py)


def _close(got, want, tol=1e-11, x1=None, x2=None):
    """max |got - want| <= tol max |want|.  With x1 / x2: entries whose two rows are the same vector but are not the exact
    diagonal of a symmetric build (duplicates, the diagonal of a row shard) are held to 1e-6 instead: there q q' - k^2 is
    pure rounding noise of the Gram product, which the arc-cosine maps (through sqrt) and Erf's kdot (through w, at raw
    forest norms) turn into first-order differences between any two float64 evaluations."""
    scale = np.abs(want).max()
    err = np.abs(got - want)
    if x1 is not None:
        same = np.all(x1[:, None, :] == x2[None, :, :], axis=2)
        assert err[same].max(initial=0.0) <= 1e-6 * scale, (err[same].max(), scale)
        err = np.where(same, 0.0, err)
    assert err.max() <= tol * scale, (err.max(), scale)


STACKS = [[ACTS["erf"]], [ACTS["erf_abc"]] * 2, [ACTS["leaky"]], [ACTS["abs"]] * 3, [ACTS["abrelu"]],
          [ACTS["erf"], ("relu",), ACTS["erf_abc"]], [("relu",), ACTS["abrelu"]]]


@pytest.mark.parametrize("acts", STACKS, ids=lambda a: "-".join(s[0] + ",".join("%g" % v for v in s[1:]) for s in a))
@pytest.mark.parametrize("b", [0.0, 0.3])
def test_kernel_build_matches_the_restatement(acts, b):
    w_std, b_std, acts = _arch(acts, 1.1, b)
    rng = np.random.default_rng(len(acts) + int(10 * b))
    x = rng.standard_normal((150, 17)) * 1.3
    x2 = rng.standard_normal((97, 17))
    want = R.kernel_fn(x, None, ("nngp", "ntk"), w_std, b_std, acts)
    got = build_act(x, None, w_std, b_std, acts)
    _close(got["nngp"], want[0]); _close(got["ntk"], want[1])
    for get in (("nngp",), ("ntk",)):  # one output only (an NNGP-only build never takes the composite ReLU map)
        g = build_act(x, None, w_std, b_std, acts, get=get)
        np.testing.assert_array_equal(g[get[0]], got[get[0]])
    # rectangular, padded ld
    want = R.kernel_fn(x2, x, ("nngp", "ntk"), w_std, b_std, acts)
    got = build_act(x2, x, w_std, b_std, acts, ld=163)
    _close(got["nngp"][:, :150], want[0]); _close(got["ntk"][:, :150], want[1])
    # row shard of the symmetric kernel
    full = R.kernel_fn(x, None, ("nngp", "ntk"), w_std, b_std, acts)
    got = build_act(x, x, w_std, b_std, acts, rows=(36, 101))
    for i, g in enumerate(("nngp", "ntk")):  # (a row shard is not the symmetric build: its diagonal takes the cross-entry form)
        _close(got[g][36:101], full[i][36:101], x1=x[36:101], x2=x)
    # float32 output
    got = build_act(x, None, w_std, b_std, acts, dtype=torch.float32)
    assert np.abs(got["nngp"] - full[0]).max() <= 1e-6 * np.abs(full[0]).max()
    assert np.abs(got["ntk"] - full[1]).max() <= 1e-6 * np.abs(full[1]).max()


@pytest.mark.parametrize("acts", [[ACTS["erf"]], [ACTS["erf_abc"]] * 2, [ACTS["leaky"]], [ACTS["abrelu"], ACTS["erf"]]])
def test_edge_rows_and_the_diagonal_entry_point(acts, golden_dir):
    """Zero rows, exact duplicates and raw forest rows (|x|^2 ~ 2e7); the symmetric build's diagonal is nngp_kernel_diag_act's
    bit for bit."""
    w_std, b_std, acts = _arch(acts, 1.0, 0.1)
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    rng = np.random.default_rng(2)
    raw = np.abs(rng.standard_normal((60, 20))) * 1000.0
    assert np.median(np.sum(raw * raw, axis=1)) > 1e7
    x = np.concatenate([g["X_train"][:70], np.zeros((3, 20)), raw, raw[:5], g["X_train"][:4]])
    want = R.kernel_fn(x, None, ("nngp", "ntk"), w_std, b_std, acts)
    got = build_act(x, None, w_std, b_std, acts)
    off = ~np.eye(x.shape[0], dtype=bool)  # the exact diagonal is held to 1e-11 below
    for i, g in enumerate(("nngp", "ntk")):
        _close(np.where(off, got[g], 0.0), np.where(off, want[i], 0.0), x1=x, x2=x)
        _close(np.diag(got[g]), np.diag(want[i]))
    assert np.all(np.isfinite(got["nngp"])) and np.all(np.isfinite(got["ntk"]))
    dn, dt = diag_act(x, w_std, b_std, acts)
    np.testing.assert_array_equal(np.diag(got["nngp"]), dn)
    np.testing.assert_array_equal(np.diag(got["ntk"]), dt)
    rn, rt = R.diag_kernel(x, w_std, b_std, acts)
    _close(dn, rn); _close(dt, rt)
    # repeated builds are bit-identical
    again = build_act(x, None, w_std, b_std, acts)
    np.testing.assert_array_equal(again["nngp"], got["nngp"]); np.testing.assert_array_equal(again["ntk"], got["ntk"])


@pytest.mark.parametrize("get", ["nngp", "ntk"])
@pytest.mark.parametrize("n", [1000, 4097, 16384])
def test_fit_predict_against_the_float64_posterior(get, n):
    acts = [ACTS["erf"], ACTS["leaky"]] if n != 4097 else [ACTS["erf_abc"]]
    w_std, b_std, acts = _arch(acts, 1.0, 0.1)
    d = 24
    x, y = synth.synthetic_queries(n, d, seed=n)
    xt, _ = synth.synthetic_queries(16, d, seed=n + 1)
    model = GPModel(n, d, w_std, b_std, get=get, diag_reg=1e-3, activations=acts).fit(x, y)
    mean, cov = model.predict(xt, cov="full")
    mean_d, var = model.predict(xt, cov="diag")
    if n <= 4097:
        ref_mean, ref_cov = R.Posterior(x, y, w_std, b_std, acts, diag_reg=1e-3).predict(xt, get, True)
    else:  # the reference posterior from the float64 kernels, in float64 on the device (the kernels are pinned above)
        _, _, kf = stax.serial(*_layers(w_std, b_std, acts))
        kdd = kf(x, None, get, as_numpy=False)
        ktd = kf(xt, x, get, as_numpy=False)
        a = kdd + 1e-3 * (torch.trace(kdd) / n) * torch.eye(n, dtype=torch.float64, device=G.dev())
        l = torch.linalg.cholesky(a)
        yd = torch.from_numpy(np.asarray(y, np.float64).reshape(n, -1)).to(G.dev())
        ref_mean = (ktd @ torch.cholesky_solve(yd, l)).cpu().numpy()
        z = torch.cholesky_solve(ktd.T.contiguous(), l)
        ntt = kf(xt, None, "nngp", as_numpy=False)
        if get == "nngp":
            ref_cov = (ntt - ktd @ z).cpu().numpy()
        else:
            ndd = kf(x, None, "nngp", as_numpy=False)
            ntd = kf(xt, x, "nngp", as_numpy=False)
            c = ntd @ z
            ref_cov = (ntt + z.T @ ndd @ z - (c + c.T)).cpu().numpy()
        del kdd, a, l
    assert G.mean_gate(mean, ref_mean)[0] < 1e-6
    assert G.mean_gate(mean_d, ref_mean)[0] < 1e-6
    rv = np.diag(ref_cov)
    np.testing.assert_allclose(var, rv, rtol=1e-5, atol=1e-9 * np.abs(rv).max())
    assert np.abs(cov - ref_cov).max() <= 1e-5 * np.abs(rv).max()
    # a second fit of the same model is bit-identical
    model.fit(x, y)
    mean2, var2 = model.predict(xt, cov="diag")
    np.testing.assert_array_equal(mean2, mean_d); np.testing.assert_array_equal(var2, var)
    model.close()


def _layers(w_std, b_std, acts):
    out = [stax.Dense(64, W_std=w_std[0], b_std=b_std[0])]
    for l, a in enumerate(acts):
        act = stax.Relu() if a[0] == "relu" else (stax.ABRelu(a[1], a[2]) if a[0] == "abrelu" else stax.Erf(*a[1:]))
        out += [act, stax.Dense(64, W_std=w_std[l + 1], b_std=b_std[l + 1])]
    return out


@pytest.mark.parametrize("act", [stax.Erf(), stax.LeakyRelu(0.1)])
def test_forest_fixture(act, golden_dir):
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    X, Y, Xt = g["X_train"], g["Y_train"], g["X_test"]
    _, _, kf = stax.serial(stax.Dense(512), act, stax.Dense(1))
    pf = predict.gradient_descent_mse_ensemble(kf, X, Y, diag_reg=1e-3)
    mean, cov = pf(x_test=Xt, get="nngp", compute_cov=True)
    ref_mean, ref_cov = R.Posterior(X, Y, kf.w_std, kf.b_std, kf.activations, diag_reg=1e-3).predict(Xt, "nngp", True)
    assert G.mean_gate(mean, ref_mean)[0] < 1e-6
    np.testing.assert_allclose(np.diag(cov), np.diag(ref_cov), rtol=1e-5, atol=1e-9 * np.abs(np.diag(ref_cov)).max())
    assert pf.model_for("nngp").activations == kf.activations


def test_serving_and_append_for_erf():
    w_std, b_std, acts = _arch([ACTS["erf"]], 1.0, 0.1)
    n, d = 2500, 20
    x, y = synth.synthetic_queries(n + 40, d, seed=6)
    xt, _ = synth.synthetic_queries(150, d, seed=106)
    model = GPModel(n + 40, d, w_std, b_std, get="nngp", diag_reg=1e-3, activations=acts).fit(x[:n], y[:n])
    model.set_refine(3)
    mean0, var0 = model.predict(xt, cov="diag")
    model.prepare_serving()
    model.set_refine(2)
    mean1, var1 = model.predict(xt, cov="diag")
    np.testing.assert_allclose(mean1, mean0, rtol=1e-6, atol=1e-6 * np.abs(mean0).max())
    np.testing.assert_allclose(var1, var0, rtol=2e-6)
    model.append(x[n:], y[n:])
    ref = GPModel(n + 40, d, w_std, b_std, get="nngp", diag_reg=1e-3, activations=acts).fit(x, y)
    m2, v2 = model.predict(xt, cov="diag")
    m3, v3 = ref.predict(xt, cov="diag")
    np.testing.assert_allclose(m2, m3, rtol=1e-6, atol=1e-6 * np.abs(m3).max())
    np.testing.assert_allclose(v2, v3, rtol=1e-5, atol=1e-9 * np.abs(v3).max())
    ref_mean, ref_cov = R.Posterior(x, y, w_std, b_std, acts, diag_reg=1e-3).predict(xt, "nngp", True)
    assert G.mean_gate(m2, ref_mean)[0] < 1e-6
    model.close(); ref.close()


def test_checkpoints(tmp_path):
    x, y = synth.synthetic_queries(300, 12, seed=3)
    xt, _ = synth.synthetic_queries(20, 12, seed=4)
    acts = [ACTS["erf_abc"], ACTS["abs"]]
    m = GPModel(300, 12, [1.0, 1.2, 0.9], [0.1, 0.0, 0.2], get="ntk", activations=acts).fit(x, y)
    m.save(str(tmp_path / "act"))
    z = np.load(str(tmp_path / "act.npz"))
    assert str(z["format"]).endswith("v2") and z["activations"].shape == (2, 4)
    m2 = GPModel.load(str(tmp_path / "act"))
    assert m2.activations == m.activations and not m2.all_relu
    np.testing.assert_array_equal(m2.predict(xt, cov="diag")[0], m.predict(xt, cov="diag")[0])
    r = GPModel(300, 12, [1.0, 1.0], [0.0, 0.0]).fit(x, y)
    r.save(str(tmp_path / "relu"))
    assert str(np.load(str(tmp_path / "relu.npz"))["format"]).endswith("v1")
    r2 = GPModel.load(str(tmp_path / "relu"))
    assert r2.all_relu
    np.testing.assert_array_equal(r2.predict(xt, cov="diag")[0], r.predict(xt, cov="diag")[0])
    for mm in (m, m2, r, r2):
        mm.close()


@pytest.mark.parametrize("act", [stax.ABRelu(0, 1), stax.LeakyRelu(0.0)])
def test_relu_spelled_as_abrelu_gives_the_relu_bits(act):
    x, y = synth.synthetic_queries(700, 16, seed=9)
    xt, _ = synth.synthetic_queries(40, 16, seed=10)
    outs = []
    for a in (stax.Relu(), act):
        _, _, kf = stax.serial(stax.Dense(64, b_std=0.1), a, stax.Dense(64), stax.Relu(), stax.Dense(1))
        k = kf(x, None)
        kx = kf(xt, x, "nngp")
        pf = predict.gradient_descent_mse_ensemble(kf, x, y, diag_reg=1e-3)
        mean, cov = pf(x_test=xt, get="ntk", compute_cov=True)
        outs.append((k.nngp, k.ntk, kx, mean, cov))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    # the C ABI maps ABRelu(0, 1) to the ReLU kernels too
    arch = _lib.make_arch_act([1.0, 1.0], [0.1, 0.0], [("relu",)])
    arch.act[0] = _lib.ACT_ABRELU
    arch.p[0][0], arch.p[0][1] = 0.0, 1.0
    lib = _lib.load()
    xd = _lib.to_device_f64(x, G.dev())
    out = torch.empty((700, 700), dtype=torch.float64, device=G.dev())
    _lib.check(lib.nngp_kernel_build_act(_lib.ptr(xd), 700, None, 700, 16, ctypes.byref(arch), _lib.DTYPE_F64, _lib.ptr(out), None,
                                         700, 0, 700, _lib.stream_ptr()))
    np.testing.assert_array_equal(out.cpu().numpy(), G.kernel_build(x, None, [1.0, 1.0], [0.1, 0.0], get=("nngp",))["nngp"])


def test_error_paths():
    lib = _lib.load()
    x = _lib.to_device_f64(np.ones((8, 4)), G.dev())
    out = torch.empty((8, 8), dtype=torch.float64, device=G.dev())
    arch = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])
    arch.act[0] = 7
    assert lib.nngp_kernel_build_act(_lib.ptr(x), 8, None, 8, 4, ctypes.byref(arch), _lib.DTYPE_F64, _lib.ptr(out), None, 8, 0, 8,
                                     _lib.stream_ptr()) == -2
    assert b"unknown activation" in lib.nngp_last_error()
    arch = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])
    arch.p[0][1] = float("nan")
    assert lib.nngp_kernel_diag_act(_lib.ptr(x), 8, 4, ctypes.byref(arch), _lib.ptr(out), None, _lib.stream_ptr()) == -2
    assert b"not finite" in lib.nngp_last_error()
    h = ctypes.c_void_p()
    assert lib.nngp_model_create_act(ctypes.byref(h), 8, 0, 4, 1, ctypes.byref(arch), _lib.GET_NNGP, 1e-3, 0) == -2
    assert not h
    from nngp_src_amd import dist2d, shard32
    with pytest.raises(NotImplementedError):
        shard32.HipRowOps(256, 4, [1.0, 1.0], [0.0, 0.0], activations=[("erf", 1.0, 1.0, 0.0)])
    with pytest.raises(NotImplementedError):
        dist2d.HipOps([1.0, 1.0], [0.0, 0.0], activations=[("abrelu", -1.0, 1.0)])
    # a different activation is a different kernel (nothing silently computes ReLU)
    xs = np.random.default_rng(0).standard_normal((30, 5))
    _, _, kr = stax.serial(stax.Dense(8), stax.Relu(), stax.Dense(1))
    _, _, ke = stax.serial(stax.Dense(8), stax.Erf(), stax.Dense(1))
    assert np.abs(kr(xs, None, "nngp") - ke(xs, None, "nngp")).max() > 1e-2


def test_train_cli_with_erf(golden_dir, tmp_path):
    from nngp_src_amd import train as train_cli
    g = np.load(os.path.join(golden_dir, "forest_queries.npz"))
    g = {k: g[k] for k in g.files}
    sent = np.iinfo(np.int32).min
    names = "ABCDEFGHIJ"
    per_file = 2000
    for fi, fn in enumerate(g["files"]):
        with open(tmp_path / str(fn), "w") as f:
            for i in range(fi * per_file, (fi + 1) * per_file):
                preds = ["%s,%d,%d" % (names[c], g["bounds"][i, c, 0], g["bounds"][i, c, 1]) for c in range(10)
                         if g["bounds"][i, c, 0] != sent]
                f.write("#".join(preds) + "@%d\n" % g["cards"][i])
    args = train_cli.make_parser().parse_args(["--kernel_type", "nngp", "--query_path", str(tmp_path), "--activation", "erf",
                                               "--max_num_train", "1000", "--max_num_test", "200"])
    args.join_query = False
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    text = buf.getvalue()
    for needle in ("number of query: 18000", "(1000, 20) (200, 20)", "Mean Square Error:", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    assert np.all(np.isfinite(res["pred_mean"])) and np.all(res["pred_std"] > 0)
