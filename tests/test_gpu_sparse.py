"""The sparse (inducing-point, DTC) NNGP posterior on the MI355X (include/nngp_sparse.h, csrc/sparse_gp.hip) against the NumPy
float64 reference (sparse_reference.py) and, in the limit U = X, against the oracle's exact posterior.

Bounds.  The Gram kernel: |delta| <= 1e-13 sqrt(rows) max|A|^2 per entry -- float64 accumulation of `rows` products, a factor 10 over
the random-sign estimate.  The model at cond(K_uu) <= 1e5 (asserted with NumPy first): means within 1e-8 of max |mean|, variances
within 1e-8 K(x, x) -- the kernel build is documented at <= 3e-14 of sqrt(K_ii K_jj), the solve with L_u amplifies by at most
cond(K_uu), that is 3e-9, times a margin of 3.  The exact limit at cond 3.2e6: 1e-6 (3e-14 x 3.2e6 ~ 1e-7, x 10).  Every test
prints what it measured before it asserts; DESIGN.md section 16 records the figures.
"""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import additive_reference as AR
import nngp_oracle as o
import sparse_reference as S
from nngp_src_amd import _lib, stax
from nngp_src_amd import train as train_cli
from nngp_src_amd.sparse import SparseGPModel, select_inducing

pytestmark = pytest.mark.gpu

COND_CAP = 1e5
TOL = 1e-8


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def forest(golden_dir):
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    return g["X_train"], g["Y_train"], g["X_test"], g["Y_test"]


@pytest.fixture(scope="module")
def plain():
    return S.oracle_kernel(1)


@pytest.fixture(scope="module")
def picks(forest, plain):
    """The reference's greedy inducing rows of the 1000 forest rows: {m: (indices, smallest relative gap)}."""
    return {m: S.greedy_inducing(plain[0], forest[0], m) for m in (128, 200)}


@pytest.fixture(scope="module")
def ref200(forest, plain, picks):
    """The float64 reference of the main case: all 1000 rows, 200 greedy inducing rows, jitter 1e-8, chunks of 256."""
    x, y, xt, _ = forest
    ref = S.SparseReference(plain[0], plain[1], jitter=1e-8).fit(x, y, x[picks[200][0]], chunk_rows=256)
    mean, cov = ref.predict(xt, "full")
    _, var = ref.predict(xt, "diag")
    return ref, mean, var, cov


def model_for(m_cap, jitter=1e-8, chunk_rows=256, ny=1, **kw):
    return SparseGPModel(m_cap, 20, [1.0, 1.0], [0.0, 0.0], diag_reg=1e-3, chunk_rows=chunk_rows, jitter=jitter, test_cap=128, ny=ny, **kw)


def errors(mean, var, ref_mean, ref_var, kdiag):
    return (float(np.abs(mean - ref_mean).max() / np.abs(ref_mean).max()), float(np.max(np.abs(var - ref_var) / kdiag)))


# ---- 1. the Gram kernel alone ----

def syrk(c, r, a, y, rows, mp, beta):
    lib = _lib.load()
    ny = 1 if y is None else y.shape[1]
    _lib.check(lib.nngp_syrk_tn_f64(_lib.ptr(c), c.stride(0), _lib.ptr(r), _lib.ptr(a), a.stride(0), _lib.ptr(y), rows, mp, ny, beta,
                                    _lib.stream_ptr()), lib)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,mp,ny", [(1, 128, 1), (17, 128, 2), (300, 384, 1), (4100, 384, 3), (520, 1024, 1)])
def test_syrk_tn_against_numpy(rows, mp, ny):
    rng = np.random.default_rng(rows + mp)
    lda, ldc, sentinel = mp + 6, mp + 3, 7.25
    data = [(rng.standard_normal((rows, mp)), rng.standard_normal((rows, ny))) for _ in range(2)]

    def run():
        c = torch.full((mp, ldc), sentinel, dtype=torch.float64, device=dev())
        r = torch.full((mp, ny), sentinel, dtype=torch.float64, device=dev())
        out = []
        for step, (a, y) in enumerate(data):
            ad = torch.full((rows, lda), float("nan"), dtype=torch.float64, device=dev())  # the padding columns are never read
            ad[:, :mp] = torch.from_numpy(a).to(dev())
            syrk(c, r, ad, torch.from_numpy(y).to(dev()), rows, mp, 0.0 if step == 0 else 1.0)  # beta = 0, then accumulate
            out.append((c.cpu().numpy(), r.cpu().numpy()))
        return out

    got = run()
    blocks = np.arange(mp) // 128
    lower = blocks[:, None] >= blocks[None, :]  # the 128 x 128 tiles on or below the diagonal
    want_c, want_r = np.zeros((mp, mp)), np.zeros((mp, ny))
    for step, (a, y) in enumerate(data):
        want_c, want_r = want_c + a.T @ a, want_r + a.T @ y
        c, r = got[step]
        # the bound of one call, also after the beta = 1 step that has summed 2 rows products (max|A| over both calls' data)
        tol = 1e-13 * np.sqrt(rows) * max(np.abs(d[0]).max() for d in data[:step + 1]) ** 2
        tol_r = 1e-13 * np.sqrt(rows) * max(np.abs(d[0]).max() * np.abs(d[1]).max() for d in data[:step + 1])
        e_c = np.abs(c[:, :mp] - want_c)[lower].max()
        e_r = np.abs(r - want_r).max()
        print("syrk rows %d mp %d ny %d step %d: C err %.2e (bound %.2e), R err %.2e (bound %.2e)" % (rows, mp, ny, step, e_c, tol, e_r, tol_r))
        assert e_c <= tol and e_r <= tol_r
        assert np.all(c[:, :mp][~lower] == sentinel) and np.all(c[:, mp:] == sentinel)  # nothing above the diagonal blocks is written
    again = run()
    for (c0, r0), (c1, r1) in zip(got, again):  # two identical sequences of calls: the same bits
        assert c0.tobytes() == c1.tobytes() and r0.tobytes() == r1.tobytes()


def test_syrk_tn_without_r_leaves_it_alone():
    a = torch.randn((200, 256), dtype=torch.float64, device=dev())
    c = torch.zeros((256, 256), dtype=torch.float64, device=dev())
    syrk(c, None, a, None, 200, 256, 0.0)
    want = (a.T @ a).cpu().numpy()
    got = c.cpu().numpy()
    assert np.abs(got - want)[128:, :].max() <= 1e-13 * np.sqrt(200) * float(a.abs().max()) ** 2 and np.all(got[:128, 128:] == 0.0)


# ---- 2. the model against the reference ----

def test_model_against_the_reference(forest, plain, picks, ref200):
    x, y, xt, _ = forest
    idx, gap = picks[200]
    ref, ref_mean, ref_var, ref_cov = ref200
    cond = np.linalg.cond(ref.kuu.astype(np.float64))
    print("cond(K_uu + jitter) = %.2e (m = 200, smallest pick gap %.1e)" % (cond, gap))
    assert cond <= COND_CAP
    kdiag = plain[1](xt)
    model = model_for(200).set_inducing(x[idx]).add_rows(x, y).finish()
    info = model.info()
    assert (info["n"], info["m"], info["m_padded"], info["chunks"]) == (1000, 200, 256, 4)
    mean, var = model.predict(xt, "diag")
    mean_f, cov = model.predict(xt, "full")
    mean_n = model.predict(xt, None)
    e_mean, e_var = errors(mean, var, ref_mean, ref_var, kdiag)
    e_cov = float(np.max(np.abs(cov - ref_cov) / np.sqrt(np.outer(kdiag, kdiag))))
    # the reference's own distance to 80-bit arithmetic, same case
    ld = S.SparseReference(plain[0], plain[1], jitter=1e-8, dtype=np.longdouble).fit(x, y, x[idx], chunk_rows=256)
    mean_l, var_l = ld.predict(xt, "diag")
    r_mean, r_var = errors(ref_mean, ref_var, mean_l.astype(np.float64), var_l.astype(np.float64), kdiag)
    d_mean, d_var = errors(mean, var, mean_l.astype(np.float64), var_l.astype(np.float64), kdiag)
    print("device vs float64 reference: mean %.2e of max |mean|, variance %.2e K(x,x), full covariance %.2e sqrt(K_ii K_jj)" % (e_mean, e_var, e_cov))
    print("float64 reference vs 80-bit: mean %.2e, variance %.2e; device vs 80-bit: mean %.2e, variance %.2e" % (r_mean, r_var, d_mean, d_var))
    print("sigma2 %.17g (reference %.17g), jitter added %.3e" % (info["sigma2"], float(ref.sigma2), info["jitter_added"]))
    assert e_mean <= TOL and e_var <= TOL and e_cov <= TOL
    assert np.array_equal(cov, cov.T)
    np.testing.assert_allclose(mean_f, mean, rtol=0, atol=1e-12 * np.abs(mean).max())  # one block of 200 rows against blocks of 128
    np.testing.assert_array_equal(mean_n, mean)
    np.testing.assert_allclose(np.diag(cov), var, rtol=0, atol=TOL * kdiag.max())
    np.testing.assert_allclose(info["jitter_added"], float(ref.jitter_added), rtol=1e-12)
    model.close()


# ---- 3. the exact limit ----

def test_exact_limit_against_the_oracle(forest):
    x, y, xt, _ = forest
    x, y = x[:256], y[:256]
    model = model_for(256, jitter=0.0).fit(x, y, x)
    mean, var = model.predict(xt, "diag")
    mean_o, cov_o = o.Posterior(x, y, o.make_arch(1), 1e-3).predict(xt, "nngp", True)
    e_mean = float(np.abs(mean - mean_o).max() / np.abs(mean_o).max())
    e_var = float(np.abs(var / np.diag(cov_o) - 1.0).max())
    print("exact limit (256 rows, jitter 0): mean %.2e of max |mean|, variance %.2e relative" % (e_mean, e_var))
    assert e_mean <= 1e-6 and e_var <= 1e-6
    model.close()


# ---- 4. rows added after a finish ----

def test_rows_added_after_a_finish(forest, plain, picks):
    x, y, xt, _ = forest
    u = x[picks[200][0]]
    model = model_for(200).set_inducing(u)
    model.add_rows(x[:512], y[:512]).finish()
    s512 = model.info()["sigma2"]
    first = model.predict(xt, "diag")
    model.add_rows(x[512:], y[512:]).finish()
    s1000 = model.info()["sigma2"]
    second = model.predict(xt, "diag")
    fresh = model_for(200).set_inducing(u).add_rows(x, y).finish()  # chunks of 256: the same boundaries
    third = fresh.predict(xt, "diag")
    assert second[0].tobytes() == third[0].tobytes() and second[1].tobytes() == third[1].tobytes()
    assert first[0].tobytes() != second[0].tobytes()
    kd = plain[1](x)
    want512, want1000 = 1e-3 * (np.sum(kd[:512]) / 512), 1e-3 * (np.sum(kd) / 1000)
    print("sigma2: 512 rows %.17g (reference %.17g), 1000 rows %.17g (reference %.17g)" % (s512, want512, s1000, want1000))
    np.testing.assert_allclose([s512, s1000], [want512, want1000], rtol=1e-14)
    assert model.info()["chunks"] == 4 and fresh.info()["chunks"] == 4
    model.close()
    fresh.close()


def test_fewer_inducing_rows_than_the_capacity_at_the_default_chunk():
    """A handle created for m_cap = 2560 and given 2048 inducing rows, one chunk of 8192 rows (the default chunk_rows).  The Gram
    kernel's partial workspace is NOT monotone in mp: mp = 2048 has 136 tiles and cuts 8192 rows into 16 splits, 36 175 872 doubles,
    while mp = 2560 has 210 tiles and 10 splits, 34 816 000.  A workspace sized for the capacity alone is too small for this call;
    the handle sizes it for the largest count over every mp it can be given.  The result equals, bit for bit, that of a handle whose
    capacity is 2048: the same mp, so the same kernels on the same grid."""
    rng = np.random.default_rng(11)
    x, xt = rng.standard_normal((8192, 20)), rng.standard_normal((64, 20))
    y = np.sin(x[:, :1]) + 0.1 * rng.standard_normal((8192, 1))
    out = []
    for m_cap in (2560, 2048):
        model = model_for(m_cap, chunk_rows=8192).set_inducing(x[:2048]).add_rows(x, y).finish()
        info = model.info()
        assert (info["n"], info["m"], info["m_padded"], info["chunks"]) == (8192, 2048, 2048, 1)
        out.append(model.predict(xt, "diag"))
        model.close()
    (mean_a, var_a), (mean_b, var_b) = out
    print("m_cap 2560 / 2048 with m = 2048: max |mean| %.4f, variances %.3e .. %.3e" % (np.abs(mean_a).max(), var_a.min(), var_a.max()))
    assert np.all(np.isfinite(mean_a)) and np.all(var_a > 0)
    assert mean_a.tobytes() == mean_b.tobytes() and var_a.tobytes() == var_b.tobytes()


# ---- 5. two outputs; an additive kernel ----

def test_two_outputs(forest, plain, picks):
    x, y, xt, _ = forest
    rng = np.random.default_rng(5)
    y2 = np.concatenate([y, 0.5 * y - 3.0 + 0.1 * rng.standard_normal(y.shape)], axis=1)  # a linear map of the first plus noise
    idx = picks[200][0]
    ref = S.SparseReference(plain[0], plain[1], jitter=1e-8).fit(x, y2, x[idx], chunk_rows=256)
    ref_mean, ref_var = ref.predict(xt, "diag")
    model = model_for(200, ny=2).fit(x, y2, idx)
    mean, var = model.predict(xt, "diag")
    e = [float(np.abs(mean[:, c] - ref_mean[:, c]).max() / np.abs(ref_mean[:, c]).max()) for c in range(2)]
    e_var = float(np.max(np.abs(var - ref_var) / plain[1](xt)))
    print("ny = 2: mean %.2e / %.2e of max |mean| per column, variance %.2e K(x,x)" % (e[0], e[1], e_var))
    assert mean.shape == (200, 2) and max(e) <= TOL and e_var <= TOL
    model.close()


def test_additive_groups(forest):
    x, y, xt, _ = forest
    groups, w, b = list(stax.pair_groups(20)), [1.0, 1.0], [0.0, 0.0]

    def kernel(x1, x2=None):
        return AR.kernel_fn(x1, x2, "nngp", w, b, None, groups, None, 1.0, exact_same=True)

    def diag(xx):
        return AR.diag_kernel(xx, w, b, None, groups, None, 1.0)[0]

    idx, gap = S.greedy_inducing(kernel, x, 80)  # 80 rows: cond 7.4e4 (96 rows are past the cap, 1.1e5)
    ref = S.SparseReference(kernel, diag, jitter=1e-8).fit(x, y, x[idx], chunk_rows=256)
    cond = np.linalg.cond(ref.kuu)
    print("additive pairs + full: cond(K_uu + jitter) = %.2e (m = 80, smallest pick gap %.1e)" % (cond, gap))
    assert cond <= COND_CAP
    ref_mean, ref_var = ref.predict(xt, "diag")
    model = model_for(80, groups=groups).fit(x, y, idx)
    mean, var = model.predict(xt, "diag")
    e_mean, e_var = errors(mean, var, ref_mean, ref_var, diag(xt))
    print("additive: mean %.2e of max |mean|, variance %.2e K(x,x)" % (e_mean, e_var))
    assert e_mean <= TOL and e_var <= TOL
    model.close()


# ---- 6. duplicate inducing rows; the checks on a live handle ----

def test_duplicate_inducing_rows_are_an_error_code(forest, plain, picks):
    """Two identical rows, jitter 0: the second one's pivot is K_11 - K_10^2 / K_00.  The rows are (6, 2, 0, ...): |x|^2 / d = 2, so
    K_00 = K_11 = K_10 = 1 exactly (one ReLU layer halves q), the factor's entry is 1 and the pivot is exactly 0."""
    x, y, xt, _ = forest
    idx = picks[200][0]
    dup = np.zeros((1, 20))
    dup[0, :2] = (6.0, 2.0)
    u = np.concatenate([dup, dup, x[idx[:60]]])
    model = model_for(200, jitter=0.0)
    with pytest.raises(_lib.NngpError) as e:
        model.set_inducing(u)
    print("duplicate rows: %s" % e.value)
    assert re.search(r"rc=-\d+", str(e.value)) and "column 1 " in str(e.value)
    with pytest.raises(_lib.NngpError):  # the handle has no inducing set now
        model.add_rows(x[:10], y[:10])
    # the same handle takes a valid set and gives the main case's result (at this handle's jitter, 0)
    ref = S.SparseReference(plain[0], plain[1], jitter=0.0).fit(x, y, x[idx], chunk_rows=256)
    assert np.linalg.cond(ref.kuu) <= COND_CAP
    ref_mean, ref_var = ref.predict(xt, "diag")
    mean, var = model.fit(x, y, idx).predict(xt, "diag")
    e_mean, e_var = errors(mean, var, ref_mean, ref_var, plain[1](xt))
    print("after the failed set: mean %.2e, variance %.2e" % (e_mean, e_var))
    assert e_mean <= TOL and e_var <= TOL
    model.close()


def test_state_checks_on_a_live_handle(forest):
    """The -2 cases of include/nngp_sparse.h that need a handle: no GPU work is enqueued by any of them."""
    x, y, xt, _ = forest
    lib = _lib.load()
    model = model_for(128)
    xd, yd, td = (_lib.to_device_f64(a, dev()) for a in (x[:64], y[:64], xt[:8]))
    mean, var = torch.zeros((8, 1), dtype=torch.float64, device=dev()), torch.zeros(8, dtype=torch.float64, device=dev())
    before = lib.nngp_alloc_count()
    s = _lib.stream_ptr()

    def predict(mode=_lib.COV_DIAG, mt=8, out=var):
        return lib.nngp_sparse_predict(model.handle, _lib.ptr(td), mt, mode, _lib.ptr(mean), _lib.ptr(out), s)

    for rc in (lib.nngp_sparse_add_rows(model.handle, _lib.ptr(xd), _lib.ptr(yd), 64, s), lib.nngp_sparse_finish(model.handle, s), predict()):
        assert rc == -2 and b"no inducing set" in lib.nngp_last_error()
    assert lib.nngp_sparse_set_inducing(model.handle, _lib.ptr(xd), 0, s) == -2
    assert lib.nngp_sparse_set_inducing(model.handle, _lib.ptr(xd), 129, s) == -2
    model.set_inducing(x[:64])
    assert lib.nngp_sparse_finish(model.handle, s) == -2 and b"no training rows" in lib.nngp_last_error()
    assert predict() == -2 and b"finish" in lib.nngp_last_error()
    assert lib.nngp_sparse_add_rows(model.handle, _lib.ptr(xd), _lib.ptr(yd), 0, s) == -2
    assert lib.nngp_sparse_add_rows(model.handle, None, _lib.ptr(yd), 64, s) == -2
    model.add_rows(x[:64], y[:64])
    assert predict() == -2 and b"finish" in lib.nngp_last_error()
    model.finish()
    assert predict() == 0
    assert predict(mode=7) == -2 and predict(mt=0) == -2 and predict(out=None) == -2
    model.add_rows(x[64:128], y[64:128])  # rows after a finish: predict wants the next finish
    assert predict() == -2 and b"finish" in lib.nngp_last_error()
    assert predict(mode=_lib.COV_NONE, out=None) == -2
    model.finish()
    assert predict(mode=_lib.COV_NONE, out=None) == 0
    torch.cuda.synchronize()
    assert lib.nngp_alloc_count() == before
    model.close()


# ---- 7. select_inducing on the device ----

@pytest.mark.parametrize("m", [128, 200])
def test_select_inducing_greedy_on_the_device(forest, picks, m):
    _, _, kernel_fn = stax.serial(stax.Dense(512), stax.Relu(), stax.Dense(1))
    idx, gap = picks[m]
    print("select_inducing m = %d: smallest relative gap of the reference %.1e" % (m, gap))
    assert gap >= 1e-6  # far above the build's 3e-14: the picks must be equal, in order
    np.testing.assert_array_equal(select_inducing(forest[0], m, kernel_fn, method="greedy"), idx)


# ---- 8. sparse beats a subset ----

def test_sparse_beats_a_subset_on_the_device(forest, plain, picks):
    x, y, xt, yt = forest
    idx = picks[128][0]
    ref_mean = S.SparseReference(plain[0], plain[1], jitter=1e-8).fit(x, y, x[idx], chunk_rows=256).predict(xt, None)
    mse_ref = float(np.mean((ref_mean.ravel() - yt.ravel()) ** 2))
    model = model_for(128).fit(x, y, idx)
    mse = float(np.mean((model.predict(xt, None).ravel() - yt.ravel()) ** 2))
    sub = o.Posterior(x[idx], y[idx], o.make_arch(1), 1e-3).predict(xt, "nngp", False)
    mse_sub = float(np.mean((sub.ravel() - yt.ravel()) ** 2))
    print("m = 128: device %.6f, reference %.6f, subset %.6f, ratio %.4f" % (mse, mse_ref, mse_sub, mse / mse_sub))
    assert mse <= 0.75 * mse_sub
    np.testing.assert_allclose(mse, mse_ref, rtol=1e-6)
    model.close()


# ---- 9. no allocations after create ----

def test_no_allocations_after_create(forest, picks):
    x, y, xt, _ = forest
    lib = _lib.load()
    model = model_for(200)
    u = x[picks[200][0]]
    before = lib.nngp_alloc_count()
    model.set_inducing(u)
    model.add_rows(x, y)
    model.finish()
    model.predict(xt, "diag")
    model.predict(xt, None)
    model.add_rows(x[:300], y[:300]).finish().predict(xt, "diag")
    assert lib.nngp_alloc_count() == before
    model.predict(xt, "full")  # the one documented exception: the full covariance's scratch, on first use ...
    after_full = lib.nngp_alloc_count()
    assert after_full > before
    model.predict(xt[:100], "full")  # ... and not again for fewer rows
    assert lib.nngp_alloc_count() == after_full
    model.close()


# ---- 10. the command line ----

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


def test_train_cli_sparse_on_forest_queries(golden_dir, tmp_path, plain):
    from nngp_src_amd.util import train_test_val_split
    _write_queries(golden_dir, tmp_path)
    args = train_cli.parse_args(["--sparse", "128", "--query_path", str(tmp_path), "--max_num_train", "1000", "--max_num_test", "200"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
        xa, ya, _ = train_cli.load_training_data(args)
    text = buf.getvalue()
    for needle in ("(1000, 20) (200, 20)", "Kernel construction in", "Mean Square Error:", "Inference time=", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    x, y, _, xt, yt, _, _, _, _ = train_test_val_split(xa, ya, train_frac=0.6, test_frac=0.2, all_query_infos=None, max_num_train=1000)
    xt, yt = xt[:200], yt[:200]
    idx, gap = S.greedy_inducing(plain[0], x, 128)
    ref_mean = S.SparseReference(plain[0], plain[1], jitter=1e-8).fit(x, y, x[idx]).predict(xt, None)
    want = float(np.sum(np.power(ref_mean - np.asarray(yt, dtype=np.float64).reshape(ref_mean.shape), 2)))
    printed = float(re.search(r"Mean Square Error: ([0-9.eE+-]+)", text).group(1))
    print("train.py --sparse 128: printed %.6f, the reference predicts %.6f (smallest pick gap %.1e)" % (printed, want, gap))
    np.testing.assert_allclose(printed, want, rtol=5e-5)  # 4 significant digits
    assert res["fit_info"]["m"] == 128 and res["fit_info"]["n"] == 1000 and np.all(res["pred_std"] > 0)


# ---- 11. the serving class ----

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


def test_estimator_serves_from_the_sparse_model(forest, plain, picks):
    from nngp_src_amd.estimator import Estimator
    x, y, xt, _ = forest
    idx = picks[128][0]
    ref = S.SparseReference(plain[0], plain[1], jitter=1e-8).fit(x, y, x[idx])
    cond = np.linalg.cond(ref.kuu.astype(np.float64))
    assert cond <= COND_CAP
    ref_mean, ref_var = ref.predict(xt, "diag")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        est = Estimator("forest", "", "", encoder=_ForestEncoder(x, y, xt), sparse=128)
        est.load_model()  # nothing to prepare for serving: the sparse model has no explicit inverse
        mean, std = est.predict([str(i) for i in range(len(xt))])
    text = buf.getvalue()
    assert "(1000, 1) (1000, 1000)" in text and "Model construction complete." in text and "prediction time=" in text
    np.testing.assert_array_equal(est.predict_fn.inducing, idx)
    assert est.predict_fn.model_for("nngp").info()["m"] == 128
    e_mean, e_var = errors(mean, std ** 2, ref_mean.ravel(), ref_var, plain[1](xt))
    print("Estimator(sparse=128): cond %.2e, mean %.2e of max |mean|, variance %.2e K(x,x)" % (cond, e_mean, e_var))
    assert mean.shape == (200,) and std.shape == (200,) and e_mean <= TOL and e_var <= TOL
    with pytest.raises(ValueError):
        Estimator("forest", "", "", encoder=_ForestEncoder(x, y, xt), sparse=128, kernel_type="ntk")
