"""The matrix-free exact NNGP posterior on the additive kernel, on the MI355X (include/nngp_matfree_additive.h, the additive
form of k_kmv_f64 in csrc/kmv_kernel.h, csrc/matfree.hip, matfree_additive.py).

1. The operator on identity columns against the additive angle referee (tests/additive_angle_reference.py), both triangles.
2. The operator and nngp_kernel_build_additive run one group walk: the lower triangle of OUT of the identity has the build's bytes.
3. The operator against the stored additive build times V in NumPy, by the plain operator test's gate
   3e-14 sum |K V| + 1e-13 sqrt(n) max|K| max|V| (section 14 of DESIGN.md states the additive build's NNGP entries at 1.3e-14 of
   max |K|, below the 3e-14 of the plain build, so the plain constant stands); determinism, independence of r, the plain table.
4. The model against additive_reference.Posterior on the forest golden with 10 pair groups: within 10 x max(the NumPy
   reference's own distance, the solve tolerance).
5. input_scale, 6. no allocation after create, 7. Estimator and train.py.
Every figure is printed before it is asserted; DESIGN.md section 26 records them.

Model figures (test 4; NumPy reference, tol 1e-10, all converged; alpha iterations, predict iterations, mean, variance):
  (1 layer, 1000, m 128, w0 1)   27  18   6.6e-11  6.9e-12
  (3 layers, 1000, m 128, w0 1)  39  26   1.2e-10  9.9e-10
  (1 layer, 300, m 0, w0 0)      195 147  5.4e-11  1.6e-6
"""
import contextlib
import ctypes
import functools
import io
import os
import re

import numpy as np
import pytest
import torch

import additive_angle_reference as AA
import additive_reference as R
import matfree_reference as M
import sparse_reference as S
from nngp_src_amd import _lib
from nngp_src_amd import train as train_cli
from nngp_src_amd.matfree_additive import AdditiveMatrixFreeGPModel
from nngp_src_amd.model import GPModel

pytestmark = pytest.mark.gpu
TOL = 1e-10


def dev():
    return torch.device("cuda", 0)


def _table(table):
    groups, weights, w0 = table
    return _lib.make_groups(tuple(groups), tuple(weights), w0)


def kmv_add(x, v, w_std, b_std, acts, table, diag_add=0.0, pad=0, sentinel=7.25, r=None):
    """nngp_kmv_additive_f64 on x [n, d] and the first r rows of v [rows, n]: out [rows, n + pad] with the sentinel wherever nothing
    was written.  V's padding columns and its rows beyond r hold NaN: they are never read."""
    lib = _lib.load()
    n, d = x.shape
    r = v.shape[0] if r is None else r
    ld = n + pad
    vd = torch.full((v.shape[0], ld), float("nan"), dtype=torch.float64, device=dev())
    vd[:r, :n] = torch.from_numpy(np.ascontiguousarray(v[:r], dtype=np.float64)).to(dev())
    out = torch.full((v.shape[0], ld), sentinel, dtype=torch.float64, device=dev())
    arch = _lib.make_arch_act(w_std, b_std, acts or [("relu",)] * (len(w_std) - 1))
    tab = _table(table)
    xd = _lib.to_device_f64(x, dev())
    _lib.check(lib.nngp_kmv_additive_f64(_lib.ptr(out), ld, _lib.ptr(vd), ld, r, _lib.ptr(xd), n, d, ctypes.byref(arch), ctypes.byref(tab),
                                         diag_add, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def build_add(x, w_std, b_std, acts, table):
    """nngp_kernel_build_additive: the symmetric NNGP kernel of x, float64."""
    lib = _lib.load()
    xd = _lib.to_device_f64(x, dev())
    n, d = xd.shape
    out = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev())
    arch = _lib.make_arch_act(w_std, b_std, acts or [("relu",)] * (len(w_std) - 1))
    tab = _table(table)
    _lib.check(lib.nngp_kernel_build_additive(_lib.ptr(xd), n, None, n, d, ctypes.byref(arch), ctypes.byref(tab), _lib.DTYPE_F64,
                                              _lib.ptr(out), None, n, 0, n, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. the operator, entry by entry ----

REFEREE_CASES = ([(n, t) for n in ("relu1", "relu2_bias", "erf_abc") for t in ("base_full", "base")] + [("comp3", "base_full")]
                 + [("relu1", t) for t in AA.DEVICE_TABLES if t != "base_full"])


@pytest.mark.parametrize("name,tname", REFEREE_CASES)
def test_operator_on_identity_columns_meets_the_additive_gate(name, tname):
    """75 rows (two tiles a side), d = 40: OUT = K entry for entry, both triangles, for the three-group table with and without
    the whole-input term and, for relu1, every device table (chunk boundaries, overlap, widths 3 and 7, a zero weight)."""
    net = AA.NETS[name][0]
    table = AA.TABLES[tname]
    x, _, blk = AA.block("sym", net, tname)
    n = x.shape[0]
    out = kmv_add(x, np.eye(n), net.w_std, net.b_std, net.acts, table)
    assert np.all(np.isfinite(out))
    for tag, k in (("lower", out), ("upper", out.T)):
        ratio, at, of_scale = blk.ratio(k, "nngp")
        print("%s %s %s triangle: worst error / gate %.3f at %s (error %.2e of scale there)" % (name, tname, tag, ratio, at, of_scale))
        assert ratio <= 1.0, (name, tname, tag, ratio, at)
    shifted = kmv_add(x, np.eye(n), net.w_std, net.b_std, net.acts, table, diag_add=0.375)
    np.testing.assert_array_equal(shifted, out + 0.375 * np.eye(n))


# ---- 2. one group walk ----

@pytest.mark.parametrize("tname", ["base_full", "chunks"])
@pytest.mark.parametrize("name", ["relu1", "relu2_bias", "erf_abc"])
def test_operator_and_build_run_one_group_walk(name, tname):
    """OUT of the identity (diag_add = 0) has the additive build's bits on the lower triangle (row >= column): the same tile with
    the same operand roles in both kernels, through group_walk / group_map of kernel_tile.h and, for the whole-input term, the one
    Gram loop and layer map; a one-hot vector makes the second MFMA, the wave sum and the split reduction exact."""
    net = AA.NETS[name][0]
    table = AA.TABLES[tname]
    x, _ = AA.block_rows("sym")
    n = x.shape[0]
    k = build_add(x, net.w_std, net.b_std, net.acts, table)
    out = kmv_add(x, np.eye(n), net.w_std, net.b_std, net.acts, table)
    assert out.shape == k.shape
    low = np.tril_indices(n)
    differ = out[low] != k[low]
    print("%s %s: n %d, %d of %d lower entries differ from the additive build" % (name, tname, n, int(differ.sum()), differ.size))
    assert np.array_equal(out[low], k[low])


# ---- 3. the operator against the stored additive build ----

NETS = {"relu1": ([1.0, 1.0], [0.0, 0.0], None), "relu3": ([1.3] * 4, [0.0] * 4, None), "bias2": ([1.4] * 3, [0.25] * 3, None),
        "erf": ([1.1, 1.1], [0.3, 0.3], [("erf", 0.8, 1.7, 0.3)])}
ODD = [(9, 17), (9, 18), (7, 24)]  # widths 8, 9 and 17 from odd offsets: every chunk boundary of the group walk


def _pairs(d, w0):
    return (R.pair_groups(d), [1.0] * (d // 2), w0)


@pytest.mark.parametrize("n,d,r,net,table", [(1, 4, 1, "relu1", _pairs(4, 1.0)), (63, 20, 7, "bias2", _pairs(20, 0.0)),
                                             (65, 33, 17, "relu3", (ODD, [1.0, 0.5, 2.0], 1.0)),
                                             (129, 40, 33, "erf", (ODD, [1.0, 0.5, 2.0], 0.7)), (200, 20, 40, "relu1", _pairs(20, 1.0))])
def test_operator_against_the_stored_additive_build(n, d, r, net, table):
    """Tile tails (63, 65, 129, 200), the r tail (7, 17, 33, 40: wide passes and narrow ones), ld = n + 6 with NaN in V's padding
    and beyond r, a sentinel in OUT's padding; pair groups, the odd-offset table at d = 33 and d = 40, w0 = 0 in one case."""
    w_std, b_std, acts = NETS[net]
    rng = np.random.default_rng(n * 1000 + r)
    x = rng.standard_normal((n, d))
    v = rng.standard_normal((r + 2, n))  # two rows beyond r: NaN on the device, sentinel rows in OUT
    k = build_add(x, w_std, b_std, acts, table)
    diag_add = 0.0123
    out = kmv_add(x, v, w_std, b_std, acts, table, diag_add=diag_add, pad=6, r=r)
    assert np.all(out[:, n:] == 7.25) and np.all(out[r:] == 7.25)  # the padding and the rows beyond r survive
    want = v[:r] @ k + diag_add * v[:r]
    gate = 3e-14 * (np.abs(v[:r]) @ np.abs(k) + diag_add * np.abs(v[:r])) + 1e-13 * np.sqrt(n) * np.abs(k).max() * np.abs(v[:r]).max()
    ratio = float(np.max(np.abs(out[:r, :n] - want) / gate))
    print("additive kmv n %d d %d r %d %s, %d groups, w0 %g: worst error %.2e, worst error / gate %.4f"
          % (n, d, r, net, len(table[0]), table[2], np.abs(out[:r, :n] - want).max(), ratio))
    assert np.all(np.isfinite(out[:r, :n])) and ratio <= 1.0
    again = kmv_add(x, v, w_std, b_std, acts, table, diag_add=diag_add, pad=6, r=r)
    assert again.tobytes() == out.tobytes()  # two identical calls: identical bytes
    alone = kmv_add(x, v[r - 1:r], w_std, b_std, acts, table, diag_add=diag_add, pad=6)
    assert alone[0, :n].tobytes() == out[r - 1, :n].tobytes()  # a vector's result does not depend on r or on its place in the block


@pytest.mark.parametrize("net", ["relu3", "erf"])
def test_the_plain_table_gives_the_plain_operator(net):
    """n_groups = 0 and full_weight = 1 through nngp_kmv_additive_f64: the bytes of nngp_kmv_f64."""
    w_std, b_std, acts = NETS[net]
    rng = np.random.default_rng(11)
    n, d, r = 130, 20, 18
    x, v = rng.standard_normal((n, d)), rng.standard_normal((r, n))
    got = kmv_add(x, v, w_std, b_std, acts, ([], [], 1.0), diag_add=0.5, pad=2)
    lib = _lib.load()
    ld = n + 2
    vd = torch.full((r, ld), float("nan"), dtype=torch.float64, device=dev())
    vd[:, :n] = torch.from_numpy(v).to(dev())
    out = torch.full((r, ld), 7.25, dtype=torch.float64, device=dev())
    arch = _lib.make_arch_act(w_std, b_std, acts or [("relu",)] * (len(w_std) - 1))
    xd = _lib.to_device_f64(x, dev())
    _lib.check(lib.nngp_kmv_f64(_lib.ptr(out), ld, _lib.ptr(vd), ld, r, _lib.ptr(xd), n, d, ctypes.byref(arch), 0.5, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert got.tobytes() == out.cpu().numpy().tobytes()


# ---- 4. the model against the oracle ----

def _net(layers):
    return [1.0] * (layers + 1), [0.0] * (layers + 1)


@functools.lru_cache(maxsize=None)
def forest_additive_case(layers, n, m, w0):
    """The shared reference of a case: the first n forest rows, 10 pair groups of weight 1 and the whole-input term of weight w0,
    m greedy inducing rows of the summed kernel (0: none), chunks of 256, the 200 test rows, and additive_reference.Posterior.
    Computed once per process; callers must not modify it."""
    x, y, xt, _ = M.forest()
    x, y = x[:n], y[:n]
    w_std, b_std = _net(layers)
    groups = R.pair_groups(x.shape[1])

    def kernel(x1, x2=None):
        return R.kernel_fn(x1, x2, "nngp", w_std, b_std, None, groups, None, w0)

    def diag(rows):
        return R.diag_kernel(rows, w_std, b_std, None, groups, None, w0)[0]

    idx = S.greedy_inducing(kernel, x, m)[0] if m > 0 else np.zeros(0, dtype=np.int64)
    ref = M.MatfreeReference(kernel, diag).fit(x, y, x[idx] if m > 0 else None, chunk_rows=256)
    o_mean, o_cov = R.Posterior(x, y, w_std, b_std, None, groups, None, w0, 1e-3).predict(xt, "nngp", True)
    o_var = np.diag(o_cov)
    mean, var, infos = ref.predict(xt, "diag", rhs_cap=48)
    e_mean = float(np.abs(mean - o_mean).max() / np.abs(o_mean).max())
    e_var = float(np.max(np.abs(var / o_var - 1.0)))
    return dict(ref=ref, idx=idx, infos=infos, oracle_mean=o_mean, oracle_var=o_var, e_mean=e_mean, e_var=e_var, groups=groups)


def distances(mean, var, case):
    return (float(np.abs(mean - case["oracle_mean"]).max() / np.abs(case["oracle_mean"]).max()),
            float(np.max(np.abs(var / case["oracle_var"] - 1.0))))


def additive_model(n_cap, m, layers, w0, rhs_cap=48, **kw):
    w_std, b_std = _net(layers)
    return AdditiveMatrixFreeGPModel(n_cap, 20, w_std, b_std, m=m, diag_reg=1e-3, tol=TOL, max_iter=1000, rhs_cap=rhs_cap, chunk_rows=256,
                                     jitter=1e-8, groups="pairs", full_weight=w0, **kw)


@pytest.mark.parametrize("layers,n,m,w0", [(1, 1000, 128, 1.0), (3, 1000, 128, 1.0), (1, 300, 0, 0.0)])
def test_model_against_the_additive_oracle(layers, n, m, w0):
    """Forest golden, 10 pair groups (+ the whole input), 200 test rows in blocks of 48: sigma2, convergence, iteration counts
    and the distances to the exact posterior, by the plain model test's rule with the reference's own distance floored at the
    solve tolerance (a reference that overshot the tolerance says nothing about what the tolerance promises)."""
    x, y, xt, _ = M.forest()
    case = forest_additive_case(layers, n, m, w0)
    ref = case["ref"]
    model = additive_model(n, m, layers, w0).fit(x[:n], y[:n], case["idx"] if m > 0 else None)
    fit = model.info()
    mean, var = model.predict(xt, "diag")
    pred = model.info()
    e_mean, e_var = distances(mean, var, case)
    ref_pred_it = max(i["iterations"] for i in case["infos"])
    print("%d layer(s), n %d, m %d, w0 %g: mean %.2e of max |mean| (reference %.2e), variance %.2e relative (reference %.2e); alpha "
          "iterations %d (reference %d), true residual %.2e; predict iterations %d (reference %d), K passes %d, true residual %.2e; "
          "sigma2 %.17g" % (layers, n, m, w0, e_mean, case["e_mean"], e_var, case["e_var"], fit["iterations"], ref.fit_info["iterations"],
                            fit["rel_residual"], pred["iterations"], ref_pred_it, pred["k_passes"], pred["rel_residual"], fit["sigma2"]))
    assert abs(fit["sigma2"] / ref.sigma2 - 1.0) <= 1e-14
    assert (fit["n"], fit["m"]) == (n, m) and fit["converged"] and pred["converged"]
    assert fit["rel_residual"] <= TOL and pred["rel_residual"] <= TOL
    assert fit["iterations"] <= ref.fit_info["iterations"] + 5 and pred["iterations"] <= ref_pred_it + 5
    assert e_mean <= 10.0 * max(case["e_mean"], TOL) and e_var <= 10.0 * max(case["e_var"], TOL)
    model.close()


# ---- 5. input_scale ----

def test_input_scale_is_the_model_on_scaled_rows():
    """A model with input_scale = s gives the bytes of a model without it on the rows x * s (train, inducing and test rows)."""
    x, y, xt, _ = M.forest()
    x, y = x[:300], y[:300]
    s = np.array([0.3, 1.7, 0.0, 1.1, 0.9, 2.3, 0.7, 1.3, 0.6, 1.9, 1.0, 0.1, 3.1, 0.77, 1.21, 0.45, 2.9, 0.33, 1.57, 0.81])
    idx = np.arange(0, 300, 8)[:40]
    scaled = additive_model(300, 40, 1, 1.0, rhs_cap=16, input_scale=s).fit(x, y, idx)
    plain = additive_model(300, 40, 1, 1.0, rhs_cap=16).fit(x * s, y, idx)
    assert scaled.alpha().tobytes() == plain.alpha().tobytes()
    for a, b in zip(scaled.predict(xt[:40], "diag"), plain.predict(xt[:40] * s, "diag")):
        assert a.tobytes() == b.tobytes()
    rows = additive_model(300, 40, 1, 1.0, rhs_cap=16, input_scale=s).fit(x, y, x[idx])  # the inducing rows themselves are scaled too
    assert rows.alpha().tobytes() == plain.alpha().tobytes()
    b = np.random.default_rng(3).standard_normal((4, 300))
    assert scaled.solve(b).tobytes() == plain.solve(b).tobytes()  # right-hand sides are not rows: nothing to scale
    for mdl in (scaled, plain, rows):
        mdl.close()


# ---- 6. memory ----

def test_no_allocations_after_create():
    x, y, xt, _ = M.forest()
    lib = _lib.load()
    idx = np.arange(0, 300, 8)[:40]
    model = additive_model(300, 40, 1, 1.0, rhs_cap=16)
    before = lib.nngp_alloc_count()
    model.fit(x[:300], y[:300], idx)
    model.solve(np.random.default_rng(0).standard_normal((5, 300)))
    model.predict(xt[:40], "diag")
    model.predict(xt[:40], None)
    model.fit(x[:200], y[:200], np.zeros((0, 20))).predict(xt[:20], "diag")  # m = 0 on the same handle: the grouped diagonal's trace
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


def test_estimator_serves_from_the_additive_matrix_free_model():
    """Estimator(matrix_free=128, matrix_free_groups="pairs"): the inducing rows are the summed kernel's greedy picks, and the means
    are held against the oracle and against GPModel(groups="pairs") on the same rows by the gate of the plain surface test, 10 x
    the reference's distance.  The case is (1, 1000, 128, 1) of the model test, so the reference's distance takes that test's floor
    at the solve tolerance, for the reason given there (DESIGN.md section 26 says so).  The variance against GPModel is printed
    only: GPModel's float32-factor pipeline stands 1.1e-7 from the oracle itself."""
    from nngp_src_amd.estimator import Estimator
    x, y, xt, _ = M.forest()
    case = forest_additive_case(1, 1000, 128, 1.0)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        est = Estimator("forest", "", "", encoder=_ForestEncoder(x, y, xt), matrix_free=128, matrix_free_groups="pairs")
        est.load_model()
        mean, std = est.predict([str(i) for i in range(len(xt))])
    text = buf.getvalue()
    assert "(1000, 1) (1000, 1000)" in text and "Model construction complete." in text and "prediction time=" in text
    np.testing.assert_array_equal(est.predict_fn.inducing, case["idx"])  # chosen by the summed kernel
    model = est.predict_fn.model_for("nngp")
    assert isinstance(model, AdditiveMatrixFreeGPModel) and model.info()["m"] == 128 and len(model.spec.groups) == 10
    exact = GPModel(1000, 20, [1.0, 1.0], [0.0, 0.0], ny=1, groups="pairs")
    exact.fit(x, y)
    g_mean, g_var = exact.predict(xt, cov="diag")
    d_mean = float(np.abs(mean.reshape(-1, 1) - np.asarray(g_mean).reshape(-1, 1)).max() / np.abs(case["oracle_mean"]).max())
    d_var = float(np.max(np.abs(std ** 2 / np.asarray(g_var).ravel() - 1.0)))
    e_mean, e_var = distances(mean.reshape(-1, 1), std ** 2, case)
    g_e_mean, g_e_var = distances(np.asarray(g_mean).reshape(-1, 1), np.asarray(g_var).ravel(), case)  # GPModel's own distance to the oracle
    print("Estimator(matrix_free=128, matrix_free_groups='pairs'): mean %.2e of max |mean| from the oracle (reference %.2e), variance "
          "%.2e (reference %.2e); from GPModel(groups='pairs'): mean %.2e, variance %.2e (GPModel from the oracle: %.2e, %.2e)"
          % (e_mean, case["e_mean"], e_var, case["e_var"], d_mean, d_var, g_e_mean, g_e_var))
    assert mean.shape == (200,) and std.shape == (200,)
    gate_mean, gate_var = 10.0 * max(case["e_mean"], TOL), 10.0 * max(case["e_var"], TOL)
    assert e_mean <= gate_mean and e_var <= gate_var
    assert d_mean <= gate_mean  # against GPModel, the same gate


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


def test_train_cli_matrix_free_groups_on_forest_queries(golden_dir, tmp_path):
    """The driver prints the exact additive model's "Mean Square Error" for the split: additive_reference.Posterior of the same
    rows, to the mean tolerance of the model test carried through the sum of squares (the plain CLI test's gate, with the
    reference's distance floored at the solve tolerance as in the model test: the same kernel and sizes)."""
    from nngp_src_amd.util import train_test_val_split
    _write_queries(golden_dir, tmp_path)
    args = train_cli.parse_args(["--matrix_free", "128", "--matrix_free_groups", "pairs", "--query_path", str(tmp_path), "--max_num_train",
                                 "1000", "--max_num_test", "200"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
        xa, ya, _ = train_cli.load_training_data(args)
    text = buf.getvalue()
    for needle in ("(1000, 20) (200, 20)", "Kernel construction in", "Mean Square Error:", "Inference time=", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    x, y, _, xt, yt, _, _, _, _ = train_test_val_split(xa, ya, train_frac=0.6, test_frac=0.2, all_query_infos=None, max_num_train=1000)
    xt, yt = xt[:200], np.asarray(yt[:200], dtype=np.float64).reshape(-1, 1)
    w_std, b_std = _net(1)
    groups = R.pair_groups(20)

    def kernel(x1, x2=None):
        return R.kernel_fn(x1, x2, "nngp", w_std, b_std, None, groups, None, 1.0)

    def diag(rows):
        return R.diag_kernel(rows, w_std, b_std, None, groups, None, 1.0)[0]

    idx, _ = S.greedy_inducing(kernel, x, 128)
    ref_mean = M.MatfreeReference(kernel, diag).fit(x, y, x[idx]).predict(xt, None)
    o_mean = R.Posterior(x, y, w_std, b_std, None, groups, None, 1.0, 1e-3).predict(xt, "nngp", False).reshape(-1, 1)
    ref_dist = max(float(np.abs(ref_mean - o_mean).max() / np.abs(o_mean).max()), TOL)
    got = res["pred_mean"].reshape(-1, 1)
    dist = float(np.abs(got - o_mean).max() / np.abs(o_mean).max())
    want = float(np.sum(np.power(o_mean - yt, 2)))
    gate = 10.0 * ref_dist * np.abs(o_mean).max()  # per mean
    mse_gate = float(np.sum(gate * (2.0 * np.abs(o_mean - yt) + gate)))
    printed = float(re.search(r"Mean Square Error: ([0-9.eE+-]+)", text).group(1))
    print("train.py --matrix_free 128 --matrix_free_groups pairs: means %.2e of max |mean| from the oracle (reference %.2e); printed "
          "%.12g, the exact additive model gives %.12g (difference %.2e, gate %.2e)" % (dist, ref_dist, printed, want, abs(printed - want), mse_gate))
    assert dist <= 10.0 * ref_dist and abs(printed - want) <= mse_gate
    fi = res["fit_info"]
    assert fi["m"] == 128 and fi["n"] == 1000 and fi["converged"] and np.all(res["pred_std"] > 0)
