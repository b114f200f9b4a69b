"""The matrix-free exact NNGP posterior on the MI355X (include/nngp_matfree.h, csrc/kmv_f64.hip, csrc/matfree.hip).

1. The fused operator entry by entry: V = identity columns, so OUT is K + diag_add I itself; held to the per-entry gate of
   tests/angle_reference.py on the symmetric seam / boundary rows (d = 2 and d = 16).  This pins the operand-layout claim of
   kmv_f64.hip (register `reg` of a finished block is the B operand of the second MFMA) and would localise a transposition.
2. The operator against the stored build: K from nngp_kernel_build times V in NumPy.  Gate per output entry:
   3e-14 sum_j |K_ij V_j| (the build's stated entry error) + 1e-13 sqrt(n) max|K| max|V| (the form of the
   Gram kernel's gate: float64 accumulation of n products).
3. The solver against numpy.linalg.solve on the built K: within 10 x the NumPy reference's own distance on the same case.
4. The model against oracle.Posterior on the forest golden: within 10 x the reference's own distance to the oracle.
5. Failures are reported, 6. no allocation after create, 7. Estimator and train.py.
Every figure is printed before it is asserted; DESIGN.md section 23 records them.
"""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import angle_reference as A
import gpu_util as G
import matfree_reference as M
import nngp_oracle as o
import sparse_reference as S
from nngp_src_amd import _lib
from nngp_src_amd import train as train_cli
from nngp_src_amd.matfree import MatrixFreeGPModel

pytestmark = pytest.mark.gpu
TOL = 1e-10


def dev():
    return torch.device("cuda", 0)


def kmv(x, v, w_std, b_std, acts=None, diag_add=0.0, pad=0, sentinel=7.25, r=None):
    """nngp_kmv_f64 on x [n, d] and the first r rows of v [rows, n]: (out [rows, n + pad] with the sentinel wherever nothing was
    written, rc).  V's padding columns and its rows beyond r hold NaN: they are never read."""
    lib = _lib.load()
    n, d = x.shape
    r = v.shape[0] if r is None else r
    ld = n + pad
    vd = torch.full((v.shape[0], ld), float("nan"), dtype=torch.float64, device=dev())
    vd[:r, :n] = torch.from_numpy(np.ascontiguousarray(v[:r], dtype=np.float64)).to(dev())
    out = torch.full((v.shape[0], ld), sentinel, dtype=torch.float64, device=dev())
    arch = _lib.make_arch_act(w_std, b_std, acts or [("relu",)] * (len(w_std) - 1))
    xd = _lib.to_device_f64(x, dev())
    rc = lib.nngp_kmv_f64(_lib.ptr(out), ld, _lib.ptr(vd), ld, r, _lib.ptr(xd), n, d, ctypes.byref(arch), diag_add, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), rc


# ---- 1. the operator, entry by entry ----

@pytest.mark.parametrize("name", ["relu1", "comp3", "relu2_bias", "erf_abc"])
@pytest.mark.parametrize("family", ["d2", "d16"])
def test_operator_on_identity_columns_meets_the_angle_gate(name, family):
    """ReLU nets with 1 and 3 hidden layers, one with biases, one Erf net: OUT = K entry for entry, both triangles."""
    net = A.cases()[name][0]
    x, _, blk = A.block(family, "sym", net)
    n = x.shape[0]
    out, rc = kmv(x, np.eye(n), net.w_std, net.b_std, net.acts)
    assert rc == 0 and np.all(np.isfinite(out))
    for tag, k in (("lower", out), ("upper", out.T)):
        ratio, at = blk.ratio(k, "nngp")
        err, gate = blk.error_abs(k, "nngp"), blk.gate_abs("nngp")
        print("%s %s %s triangle: error %.2e of scale, worst error / gate %.3f at %s (error %.3e, gate %.3e there)"
              % (name, family, tag, blk.of_scale(err, "nngp").max(), ratio, at, err[at], gate[at]))
        assert ratio <= 1.0, (name, family, tag, ratio, at)
    # the diagonal term: exactly one rounding on top of the diagonal, nothing anywhere else
    shifted, rc = kmv(x, np.eye(n), net.w_std, net.b_std, net.acts, diag_add=0.375)
    assert rc == 0
    np.testing.assert_array_equal(shifted, out + 0.375 * np.eye(n))


@pytest.mark.parametrize("name", ["relu1", "relu2_bias", "erf_abc"])
@pytest.mark.parametrize("family", ["d2", "d16"])
def test_operator_and_build_run_one_map(name, family):
    """OUT of the identity (diag_add = 0) has the stored build's bits on the lower triangle (row >= column).  Those entries come
    from the same tile with the same operand roles in both kernels, through the one Gram loop and layer map of kernel_tile.h, and
    a one-hot vector makes the second MFMA, the wave sum and the split reduction exact (each is k * 1 + 0).  None of these nets
    takes the composite map in the build."""
    net = A.cases()[name][0]
    x, _, _ = A.block(family, "sym", net)
    n = x.shape[0]
    if net.family == "relu":
        k = G.kernel_build(x, None, net.w_std, net.b_std, get=("nngp",))["nngp"]
    else:
        k = G.build_act(x, None, net.w_std, net.b_std, net.acts, get=("nngp",))["nngp"]
    out, rc = kmv(x, np.eye(n), net.w_std, net.b_std, net.acts)
    assert rc == 0 and out.shape == k.shape
    low = np.tril_indices(n)
    differ = out[low] != k[low]
    print("%s %s: n %d, %d of %d lower entries differ from the build" % (name, family, n, int(differ.sum()), differ.size))
    assert np.array_equal(out[low], k[low])


# ---- 2. the operator against the stored build ----

NETS = {"relu1": ([1.0, 1.0], [0.0, 0.0], None), "relu3": ([1.3] * 4, [0.0] * 4, None), "bias2": ([1.4] * 3, [0.25] * 3, None),
        "erf": ([1.1, 1.1], [0.3, 0.3], [("erf", 0.8, 1.7, 0.3)])}


@pytest.mark.parametrize("n,d,r,net", [(1, 3, 1, "relu1"), (63, 20, 7, "bias2"), (64, 20, 16, "relu1"), (65, 33, 17, "relu3"),
                                       (129, 130, 33, "erf"), (200, 20, 40, "relu1")])
def test_operator_against_the_stored_build(n, d, r, net):
    """Tile tails (63, 65, 129, 200), the k-chunk tail (d = 3, 20, 33, 130), d > 128, the r tail (7, 17, 33, 40: a wide pass and
    a narrow one), ld = n + 6 with NaN in V's padding and beyond r, a sentinel in OUT's padding."""
    w_std, b_std, acts = NETS[net]
    rng = np.random.default_rng(n * 1000 + r)
    x = rng.standard_normal((n, d))
    v = rng.standard_normal((r + 2, n))  # two rows beyond r: NaN on the device, sentinel rows in OUT
    if acts is None:
        k = G.kernel_build(x, None, w_std, b_std, get=("nngp",))["nngp"]
    else:
        k = G.build_act(x, None, w_std, b_std, acts, get=("nngp",))["nngp"]
    diag_add = 0.0123
    out, rc = kmv(x, v, w_std, b_std, acts, diag_add=diag_add, pad=6, r=r)
    assert rc == 0
    assert np.all(out[:, n:] == 7.25) and np.all(out[r:] == 7.25)  # the padding and the rows beyond r survive
    want = v[:r] @ k + diag_add * v[:r]
    gate = 3e-14 * (np.abs(v[:r]) @ np.abs(k) + diag_add * np.abs(v[:r])) + 1e-13 * np.sqrt(n) * np.abs(k).max() * np.abs(v[:r]).max()
    ratio = float(np.max(np.abs(out[:r, :n] - want) / gate))
    print("kmv n %d d %d r %d %s: worst error %.2e, worst error / gate %.4f" % (n, d, r, net, np.abs(out[:r, :n] - want).max(), ratio))
    assert np.all(np.isfinite(out[:r, :n])) and ratio <= 1.0
    again, _ = kmv(x, v, w_std, b_std, acts, diag_add=diag_add, pad=6, r=r)
    assert again.tobytes() == out.tobytes()  # two identical calls: identical bytes
    alone, _ = kmv(x, v[r - 1:r], w_std, b_std, acts, diag_add=diag_add, pad=6)
    assert alone[0, :n].tobytes() == out[r - 1, :n].tobytes()  # a vector's result does not depend on r or on its place in the block


# ---- 3. the solver ----

def model_for(n_cap, m, n_relu=1, rhs_cap=17, ny=1, jitter=1e-8, **kw):
    return MatrixFreeGPModel(n_cap, 20, [1.0] * (n_relu + 1), [0.0] * (n_relu + 1), m=m, diag_reg=1e-3, tol=TOL, max_iter=1000,
                             rhs_cap=rhs_cap, chunk_rows=256, jitter=jitter, ny=ny, **kw)


@pytest.mark.parametrize("n,m", [(130, 0), (300, 40)])
def test_solver_against_numpy(n, m):
    x, y, _, _ = M.forest()
    x, y = x[:n], y[:n]
    kernel, diag = S.oracle_kernel(1)
    idx = M.forest_picks(1, n, m) if m > 0 else None
    ref = M.MatfreeReference(kernel, diag).fit(x, y, x[idx] if m > 0 else None, chunk_rows=256)
    b = np.random.default_rng(n).standard_normal((17, n))
    ref_x, ref_info = ref.solve(b)
    ref_exact = np.linalg.solve(ref.k + ref.sigma2 * np.eye(n), b.T).T
    ref_dist = float(np.abs(ref_x - ref_exact).max() / np.abs(ref_exact).max())

    model = model_for(n, m).fit(x, y, idx)
    info = model.info()
    assert abs(info["sigma2"] / ref.sigma2 - 1.0) <= 1e-14 and (info["n"], info["m"]) == (n, m)
    got = model.solve(b)
    info = model.info()
    k_dev = G.kernel_build(x, None, [1.0, 1.0], [0.0, 0.0], get=("nngp",))["nngp"]
    exact = np.linalg.solve(k_dev + info["sigma2"] * np.eye(n), b.T).T
    dist = float(np.abs(got - exact).max() / np.abs(exact).max())
    true_res = float(np.max(np.linalg.norm(b - got @ (k_dev + info["sigma2"] * np.eye(n)), axis=1) / np.linalg.norm(b, axis=1)))
    print("solver n %d m %d: device distance %.2e (reference's own %.2e), iterations %d (reference %d), reported true residual %.2e "
          "(NumPy's of the device result %.2e), K passes %d, restarts %d" % (n, m, dist, ref_dist, info["iterations"],
                                                                            ref_info["iterations"], info["rel_residual"], true_res,
                                                                            info["k_passes"], info["restarts"]))
    assert dist <= 10.0 * ref_dist
    assert info["iterations"] <= ref_info["iterations"] + 5
    assert info["converged"] and info["rel_residual"] <= TOL
    alone = model.solve(b[3:4])
    assert alone.tobytes() == got[3:4].tobytes()  # column 3 alone, byte for byte
    model.close()


# ---- 4. the model against the oracle ----

def distances(mean, var, case):
    return (float(np.abs(mean - case["oracle_mean"]).max() / np.abs(case["oracle_mean"]).max()),
            float(np.max(np.abs(var / case["oracle_var"] - 1.0))))


@pytest.mark.parametrize("n_relu", [1, 3])
def test_model_against_the_oracle(n_relu):
    """1000 forest rows, 200 test rows, m = 128 greedy, chunks of 256 (the last one 232)."""
    x, y, xt, _ = M.forest()
    case = M.forest_case(n_relu, 1000, 128)
    ref = case["ref"]
    model = model_for(1000, 128, n_relu=n_relu, rhs_cap=48).fit(x, y, case["idx"])
    fit = model.info()
    mean, var = model.predict(xt, "diag")
    pred = model.info()
    mean_only = model.predict(xt, None)
    e_mean, e_var = distances(mean, var, case)
    ref_pred_it = max(i["iterations"] for i in case["infos"])
    print("%d layer(s): mean %.2e of max |mean| (reference %.2e), variance %.2e relative (reference %.2e); alpha iterations %d "
          "(reference %d), true residual %.2e; predict iterations %d (reference %d), K passes %d, true residual %.2e; sigma2 %.17g"
          % (n_relu, e_mean, case["e_mean"], e_var, case["e_var"], fit["iterations"], ref.fit_info["iterations"], fit["rel_residual"],
             pred["iterations"], ref_pred_it, pred["k_passes"], pred["rel_residual"], fit["sigma2"]))
    assert abs(fit["sigma2"] / ref.sigma2 - 1.0) <= 1e-14
    assert (fit["n"], fit["m"]) == (1000, 128) and fit["converged"] and pred["converged"]
    assert fit["rel_residual"] <= TOL and pred["rel_residual"] <= TOL
    assert e_mean <= 10.0 * case["e_mean"] and e_var <= 10.0 * case["e_var"]
    assert fit["iterations"] <= ref.fit_info["iterations"] + 5 and pred["iterations"] <= ref_pred_it + 5
    np.testing.assert_array_equal(mean_only, mean)
    alpha = model.alpha()  # [n, 1]: its residual against the reference's float64 kernel (the two kernels differ by ~1e-15 per entry)
    res = float(np.linalg.norm(y - ref.apply(alpha.T).T) / np.linalg.norm(y))
    bound = TOL + 3e-14 * float(np.linalg.norm(np.abs(ref.k) @ np.abs(alpha)) / np.linalg.norm(y))  # tol + the build's entry error through K alpha
    print("alpha's residual in NumPy: %.2e (bound %.2e)" % (res, bound))
    assert alpha.shape == (1000, 1) and res <= bound
    model.close()


def test_unpreconditioned_fit_gives_the_same_posterior():
    """m = 0 on the first 300 rows against the oracle of those rows, by the rule of the preconditioned reference of that case."""
    x, y, xt, _ = M.forest()
    case = M.forest_case(1, 300, 40)
    model = model_for(300, 0, rhs_cap=48).fit(x[:300], y[:300])
    fit = model.info()
    mean, var = model.predict(xt, "diag")
    e_mean, e_var = distances(mean, var, case)
    print("m = 0, 300 rows: mean %.2e (reference %.2e), variance %.2e (reference %.2e), alpha iterations %d, predict iterations %d"
          % (e_mean, case["e_mean"], e_var, case["e_var"], fit["iterations"], model.info()["iterations"]))
    assert fit["m"] == 0 and abs(fit["sigma2"] / case["ref"].sigma2 - 1.0) <= 1e-14
    assert e_mean <= 10.0 * case["e_mean"] and e_var <= 10.0 * case["e_var"]
    model.close()


def test_two_outputs_and_the_block_width():
    x, y, xt, _ = M.forest()
    case = M.forest_case(1, 1000, 128)
    ref = case["ref"]
    y2 = np.concatenate([y, np.cos(y)], axis=1)
    model = model_for(1000, 128, rhs_cap=16, ny=2).fit(x, y2, case["idx"])
    mean2, var16 = model.predict(xt, "diag")
    model.close()
    a = ref.k + ref.sigma2 * np.eye(1000)
    want = ref.kernel(xt, x) @ np.linalg.solve(a, y2)
    e0 = float(np.abs(mean2[:, :1] - case["oracle_mean"]).max() / np.abs(case["oracle_mean"]).max())
    e1 = float(np.abs(mean2[:, 1] - want[:, 1]).max() / np.abs(want[:, 1]).max())
    wide = model_for(1000, 128, rhs_cap=48).fit(x, y, case["idx"])
    _, var48 = wide.predict(xt, "diag")
    wide.close()
    e_w = float(np.max(np.abs(var16 / var48 - 1.0)))
    print("ny = 2: column 0 %.2e, column 1 %.2e of max |mean| (reference %.2e); rhs_cap 16 against 48: variances %.2e relative "
          "(reference %.2e)" % (e0, e1, case["e_mean"], e_w, case["e_var"]))
    assert mean2.shape == (200, 2) and e0 <= 10.0 * case["e_mean"] and e1 <= 10.0 * case["e_mean"]
    assert e_w <= 10.0 * case["e_var"]


# ---- 5. failure is reported ----

def test_an_unconverged_solve_is_reported():
    x, y, xt, _ = M.forest()
    lib = _lib.load()
    model = MatrixFreeGPModel(300, 20, [1.0, 1.0], [0.0, 0.0], m=0, tol=TOL, max_iter=3, rhs_cap=16, chunk_rows=256)
    with pytest.raises(RuntimeError, match="residual") as e:
        model.fit(x[:300], y[:300])
    info = model.info()
    print("max_iter = 3: %s; info %s" % (e.value, info))
    assert not info["converged"] and info["iterations"] == 3 and info["rel_residual"] > TOL and info["k_passes"] == 4
    xd, yd = _lib.to_device_f64(x[:300], dev()), _lib.to_device_f64(y[:300], dev())
    assert lib.nngp_matfree_fit(model.handle, _lib.ptr(xd), _lib.ptr(yd), 300, None, 0, TOL, 3, _lib.stream_ptr()) == 1
    model.allow_unconverged = True
    model.fit(x[:300], y[:300])  # results are written all the same
    assert np.all(np.isfinite(model.predict(xt[:8], None)))
    model.close()


def test_duplicate_inducing_rows_pass_the_pivot_error_through():
    """The rows of the sparse test: (6, 2, 0, ...) twice with jitter 0 -- K_00 = K_11 = K_10 = 1 exactly, the pivot exactly 0."""
    x, y, xt, _ = M.forest()
    case = M.forest_case(1, 300, 40)
    dup = np.zeros((1, 20))
    dup[0, :2] = (6.0, 2.0)
    u = np.concatenate([dup, dup, x[case["idx"][:30]]])
    model = model_for(300, 40, rhs_cap=48, jitter=0.0)
    with pytest.raises(_lib.NngpError) as e:
        model.fit(x[:300], y[:300], u)
    print("duplicate rows: %s" % e.value)
    assert re.search(r"rc=-\d+", str(e.value)) and "column 1 " in str(e.value)
    with pytest.raises(_lib.NngpError):  # no fit now
        model.predict(xt, None)
    mean, var = model.fit(x[:300], y[:300], case["idx"]).predict(xt, "diag")  # the same handle takes a valid set
    e_mean, e_var = distances(mean, var, case)
    print("after the failed fit: mean %.2e, variance %.2e" % (e_mean, e_var))
    assert e_mean <= 10.0 * case["e_mean"] and e_var <= 10.0 * case["e_var"]
    model.close()


def test_argument_errors_on_a_live_handle():
    x, y, xt, _ = M.forest()
    lib = _lib.load()
    model = model_for(128, 16, rhs_cap=4)
    xd, yd, td = (_lib.to_device_f64(a, dev()) for a in (x[:200], y[:200], xt[:8]))
    mean, var = torch.zeros((8, 1), dtype=torch.float64, device=dev()), torch.zeros(8, dtype=torch.float64, device=dev())
    b, out = torch.zeros((8, 128), dtype=torch.float64, device=dev()), torch.zeros((8, 128), dtype=torch.float64, device=dev())
    s = _lib.stream_ptr()
    before = lib.nngp_alloc_count()

    def fit(n=128, u=xd, m=16, tol=TOL, it=1000):
        return lib.nngp_matfree_fit(model.handle, _lib.ptr(xd), _lib.ptr(yd), n, _lib.ptr(u), m, tol, it, s)

    def predict(mode=_lib.COV_DIAG, mt=8, tol=TOL, v=var):
        return lib.nngp_matfree_predict(model.handle, _lib.ptr(td), mt, mode, _lib.ptr(mean), _lib.ptr(v), tol, 1000, s)

    def solve(r=4, ld=128, tol=TOL):
        return lib.nngp_matfree_solve(model.handle, _lib.ptr(b), ld, r, _lib.ptr(out), ld, tol, 100, s)

    assert predict() == -2 and b"no fit" in lib.nngp_last_error()
    assert solve() == -2 and b"no fit" in lib.nngp_last_error()
    for rc in (fit(n=129), fit(n=0), fit(m=17), fit(u=None), fit(m=0), fit(tol=float("nan")), fit(tol=float("inf")), fit(tol=0.0), fit(it=0)):
        assert rc == -2, lib.nngp_last_error()
    assert fit() == 0
    assert predict(mode=_lib.COV_FULL) == -2 and b"full covariance" in lib.nngp_last_error()
    for rc in (predict(mt=0), predict(v=None), predict(tol=float("nan")), solve(r=5), solve(r=0), solve(ld=127), solve(tol=float("nan"))):
        assert rc == -2, lib.nngp_last_error()
    assert predict() == 0 and predict(mode=_lib.COV_NONE, v=None) == 0
    torch.cuda.synchronize()
    assert lib.nngp_alloc_count() == before
    model.close()


# ---- 6. memory ----

def test_no_allocations_after_create():
    x, y, xt, _ = M.forest()
    lib = _lib.load()
    idx = M.forest_picks(1, 300, 40)
    model = model_for(300, 40, rhs_cap=16)
    before = lib.nngp_alloc_count()
    model.fit(x[:300], y[:300], idx)
    model.solve(np.random.default_rng(0).standard_normal((5, 300)))
    model.predict(xt[:40], "diag")
    model.predict(xt[:40], None)
    model.fit(x[:200], y[:200], x[idx[:20]]).predict(xt[:20], "diag")  # fewer rows, the inducing rows themselves
    model.fit(x[:200], y[:200], np.zeros((0, 20))).predict(xt[:20], "diag")  # and without a preconditioner on the same handle
    assert lib.nngp_alloc_count() == before
    model.close()


# ---- 7. the surfaces ----

class _ForestEncoder:
    """Stands in for the query encoder: a query line is a row number of the fixture."""

    def __init__(self, x, y, xt):
        self.x, self.y, self.xt = x, y, xt

    def load_queries(self, path, use_aux, q_error_threshold, coef_var_threshold):
        return list(range(len(self.x))), list(self.y.ravel()), None

    def transform_to_arrays(self, queries, cards):
        return self.x[queries], np.asarray(cards).reshape(-1, 1)

    def parse_line_without_card_then_encode(self, line):
        return self.xt[int(line)]


def test_estimator_serves_from_the_matrix_free_model():
    from nngp_src_amd.estimator import Estimator
    x, y, xt, _ = M.forest()
    case = M.forest_case(1, 1000, 128)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        est = Estimator("forest", "", "", encoder=_ForestEncoder(x, y, xt), matrix_free=128)
        est.load_model()
        mean, std = est.predict([str(i) for i in range(len(xt))])
    text = buf.getvalue()
    assert "(1000, 1) (1000, 1000)" in text and "Model construction complete." in text and "prediction time=" in text
    np.testing.assert_array_equal(est.predict_fn.inducing, case["idx"])
    info = est.predict_fn.model_for("nngp").info()
    e_mean, e_var = distances(mean.reshape(-1, 1), std ** 2, case)
    print("Estimator(matrix_free=128): mean %.2e of max |mean| (reference %.2e), variance %.2e (reference %.2e)"
          % (e_mean, case["e_mean"], e_var, case["e_var"]))
    assert info["m"] == 128 and mean.shape == (200,) and std.shape == (200,)
    assert e_mean <= 10.0 * case["e_mean"] and e_var <= 10.0 * case["e_var"]


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


def test_train_cli_matrix_free_on_forest_queries(golden_dir, tmp_path):
    """The driver prints the EXACT model's "Mean Square Error" for the split: the oracle's posterior of the same rows, to the
    mean tolerance of the model test carried through the sum of squares."""
    from nngp_src_amd.util import train_test_val_split
    _write_queries(golden_dir, tmp_path)
    args = train_cli.parse_args(["--matrix_free", "128", "--query_path", str(tmp_path), "--max_num_train", "1000", "--max_num_test", "200"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
        xa, ya, _ = train_cli.load_training_data(args)
    text = buf.getvalue()
    for needle in ("(1000, 20) (200, 20)", "Kernel construction in", "Mean Square Error:", "Inference time=", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    x, y, _, xt, yt, _, _, _, _ = train_test_val_split(xa, ya, train_frac=0.6, test_frac=0.2, all_query_infos=None, max_num_train=1000)
    xt, yt = xt[:200], np.asarray(yt[:200], dtype=np.float64).reshape(-1, 1)
    kernel, diag = S.oracle_kernel(1)
    idx, _ = S.greedy_inducing(kernel, x, 128)
    ref_mean = M.MatfreeReference(kernel, diag).fit(x, y, x[idx]).predict(xt, None)
    o_mean = o.Posterior(x, y, o.make_arch(1), 1e-3).predict(xt, "nngp", False).reshape(-1, 1)
    ref_dist = float(np.abs(ref_mean - o_mean).max() / np.abs(o_mean).max())
    got = res["pred_mean"].reshape(-1, 1)
    dist = float(np.abs(got - o_mean).max() / np.abs(o_mean).max())
    want = float(np.sum(np.power(o_mean - yt, 2)))
    gate = 10.0 * ref_dist * np.abs(o_mean).max()  # per mean
    mse_gate = float(np.sum(gate * (2.0 * np.abs(o_mean - yt) + gate)))
    printed = float(re.search(r"Mean Square Error: ([0-9.eE+-]+)", text).group(1))
    print("train.py --matrix_free 128: means %.2e of max |mean| from the oracle (reference %.2e); printed %.12g, the exact model gives "
          "%.12g (difference %.2e, gate %.2e)" % (dist, ref_dist, printed, want, abs(printed - want), mse_gate))
    assert dist <= 10.0 * ref_dist and abs(printed - want) <= mse_gate
    fi = res["fit_info"]
    assert fi["m"] == 128 and fi["n"] == 1000 and fi["converged"] and np.all(res["pred_std"] > 0)
