"""The sparse (inducing-point, DTC) NNGP posterior without a GPU: the NumPy reference (sparse_reference.py) against the textbook
form, against the exact oracle posterior in the limit U = X, and against a subset-of-data fit; the argument checks of
include/nngp_sparse.h that need no device, its bindings, the command line, and select_inducing's NumPy path."""
import ctypes
import os
import re

import numpy as np
import pytest

import nngp_oracle as o
import pool_greedy_reference as R
import sparse_reference as S
from nngp_src_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def forest(golden_dir):
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    return g["X_train"], g["Y_train"], g["X_test"], g["Y_test"]


@pytest.fixture(scope="module")
def synthetic():
    """m = 24 inducing rows out of N = 90 Gaussian rows, d = 8, 30 test rows: well conditioned."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((90, 8))
    y = np.sin(x[:, :1]) + 0.3 * x[:, 1:2] + 0.05 * rng.standard_normal((90, 1))
    return x, y, x[rng.choice(90, 24, replace=False)], rng.standard_normal((30, 8))


def test_v_form_equals_the_explicit_form(synthetic):
    x, y, u, xt = synthetic
    kernel, diag = S.oracle_kernel(1)
    assert np.linalg.cond(kernel(u, None)) < 1e6
    mean, cov = S.SparseReference(kernel, diag).fit(x, y, u).predict(xt, "full")
    _, var = S.SparseReference(kernel, diag).fit(x, y, u).predict(xt, "diag")
    mean_e, cov_e = S.explicit(kernel, diag, x, y, u, xt)
    print("V-form vs explicit: mean %.2e, cov %.2e" % (np.abs(mean - mean_e).max() / np.abs(mean_e).max(),
                                                       np.abs(cov - cov_e).max() / np.abs(cov_e).max()))
    np.testing.assert_allclose(mean, mean_e, rtol=0, atol=1e-9 * np.abs(mean_e).max())
    np.testing.assert_allclose(cov, cov_e, rtol=0, atol=1e-9 * np.abs(cov_e).max())
    np.testing.assert_allclose(var, np.diag(cov_e), rtol=1e-9)
    assert np.all(var > 0)


def test_exact_limit_is_the_oracle_posterior(forest):
    """U = X (the first 256 forest rows), jitter 0: the DTC posterior is the exact one."""
    x, y, xt, _ = forest
    x, y = x[:256], y[:256]
    kernel, diag = S.oracle_kernel(1)
    mean, var = S.SparseReference(kernel, diag, jitter=0.0).fit(x, y, x).predict(xt, "diag")
    mean_o, cov_o = o.Posterior(x, y, o.make_arch(1), 1e-3).predict(xt, "nngp", True)
    e_mean = np.abs(mean - mean_o).max() / np.abs(mean_o).max()
    e_var = np.abs(var / np.diag(cov_o) - 1.0).max()
    print("exact limit, 256 rows: mean %.2e of max |mean|, variance %.2e relative, cond(K_uu) %.1e" % (e_mean, e_var, np.linalg.cond(kernel(x, None))))
    assert e_mean <= 1e-9 and e_var <= 1e-9


def test_reference_does_not_depend_on_the_chunking(synthetic):
    x, y, u, xt = synthetic
    kernel, diag = S.oracle_kernel(1)
    mean, cov = S.SparseReference(kernel, diag).fit(x, y, u).predict(xt, "full")
    for chunk in (7, 32, 89):
        ref = S.SparseReference(kernel, diag).set_inducing(u)
        ref.add_rows(x[:50], y[:50], chunk).finish()  # a finish in between changes nothing either
        mean_c, cov_c = ref.add_rows(x[50:], y[50:], chunk).finish().predict(xt, "full")
        print("chunks of %d: mean %.2e, cov %.2e" % (chunk, np.abs(mean_c - mean).max() / np.abs(mean).max(), np.abs(cov_c - cov).max() / np.abs(cov).max()))
        np.testing.assert_allclose(mean_c, mean, rtol=0, atol=1e-12 * np.abs(mean).max())
        np.testing.assert_allclose(cov_c, cov, rtol=0, atol=1e-12 * np.abs(cov).max())


def test_sparse_beats_a_subset_of_the_data(forest):
    """128 greedy inducing rows with all 1000 labels against the exact posterior fitted on those 128 rows alone."""
    x, y, xt, yt = forest
    kernel, diag = S.oracle_kernel(1)
    idx, gap = S.greedy_inducing(kernel, x, 128)
    mean = S.SparseReference(kernel, diag, jitter=1e-8).fit(x, y, x[idx], chunk_rows=256).predict(xt, None)
    mse_sparse = float(np.mean((mean.ravel() - yt.ravel()) ** 2))
    mean_sub = o.Posterior(x[idx], y[idx], o.make_arch(1), 1e-3).predict(xt, "nngp", False)
    mse_subset = float(np.mean((mean_sub.ravel() - yt.ravel()) ** 2))
    print("m = 128: sparse %.3f, subset %.3f, ratio %.3f, smallest pick gap %.1e" % (mse_sparse, mse_subset, mse_sparse / mse_subset, gap))
    assert mse_sparse <= 0.75 * mse_subset
    np.testing.assert_allclose([mse_sparse, mse_subset], [9.536, 14.104], rtol=1e-3)  # the figures of DESIGN.md section 16


def test_longdouble_referee_agrees_with_float64(synthetic):
    x, y, u, xt = synthetic
    kernel, diag = S.oracle_kernel(1)
    mean, var = S.SparseReference(kernel, diag).fit(x, y, u, 32).predict(xt, "diag")
    mean_l, var_l = S.SparseReference(kernel, diag, dtype=np.longdouble).fit(x, y, u, 32).predict(xt, "diag")
    assert mean_l.dtype == np.longdouble
    np.testing.assert_allclose(mean, mean_l.astype(np.float64), rtol=0, atol=1e-11 * np.abs(mean).max())
    np.testing.assert_allclose(var, var_l.astype(np.float64), rtol=1e-10)


def _arch():
    return _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("relu",)])


def test_argument_validation_without_gpu():
    """Every -2 of include/nngp_sparse.h that needs no handle: these fail their checks before any GPU work.  (The checks on a live
    handle's state -- rows before an inducing set, predict before finish, finish without rows -- are in test_gpu_sparse.py.)"""
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced
    arch = _arch()
    h = ctypes.c_void_p()
    good = dict(m_cap=256, chunk=256, test=128, d=8, ny=1, reg=1e-3, absolute=0, jitter=1e-8)

    def create(out=ctypes.byref(h), a=ctypes.byref(arch), **kw):
        p = dict(good, **kw)
        return lib.nngp_sparse_create(out, p["m_cap"], p["chunk"], p["test"], p["d"], p["ny"], a, None, p["reg"], p["absolute"], p["jitter"])

    for kw, word in ((dict(out=None), b"NULL"), (dict(a=None), b"NULL"), (dict(m_cap=0), b"m_cap"), (dict(m_cap=16385), b"m_cap"),
                     (dict(chunk=0), b"chunk_rows"), (dict(chunk=200), b"chunk_rows"), (dict(test=0), b"test_cap"), (dict(d=0), b"d >= 1"),
                     (dict(ny=0), b"ny"), (dict(ny=17), b"ny"), (dict(jitter=-1e-9), b"jitter"), (dict(jitter=float("nan")), b"jitter"),
                     (dict(jitter=float("inf")), b"jitter"), (dict(reg=-1.0), b"diag_reg"), (dict(reg=float("nan")), b"diag_reg"),
                     (dict(reg=float("inf")), b"diag_reg")):
        rc = create(**kw)
        assert rc == -2 and word in lib.nngp_last_error(), (kw, rc, lib.nngp_last_error())
        assert not h.value
    for rc in (lib.nngp_sparse_set_inducing(None, one, 4, None), lib.nngp_sparse_set_inducing(one, None, 4, None),
               lib.nngp_sparse_add_rows(None, one, one, 4, None), lib.nngp_sparse_finish(None, None),
               lib.nngp_sparse_predict(None, one, 4, _lib.COV_DIAG, one, one, None), lib.nngp_sparse_info(None, None)):
        assert rc == -2 and b"NULL" in lib.nngp_last_error()
    assert lib.nngp_sparse_destroy(None) == 0
    syrk = lib.nngp_syrk_tn_f64
    for args, word in (((None, 128, None, one, 128, None, 5, 128, 1, 0.0, None), b"NULL"),
                       ((one, 128, None, None, 128, None, 5, 128, 1, 0.0, None), b"NULL"),
                       ((one, 128, one, one, 128, None, 5, 128, 1, 0.0, None), b"NULL"),   # r without y
                       ((one, 128, None, one, 128, None, 0, 128, 1, 0.0, None), b"rows"),
                       ((one, 128, None, one, 128, None, 5, 100, 1, 0.0, None), b"multiple of 128"),
                       ((one, 128, None, one, 128, None, 5, 16512, 1, 0.0, None), b"16384"),
                       ((one, 128, None, one, 126, None, 5, 128, 1, 0.0, None), b"lda"),
                       ((one, 128, None, one, 129, None, 5, 128, 1, 0.0, None), b"lda"),
                       ((one, 127, None, one, 128, None, 5, 128, 1, 0.0, None), b"ldc"),
                       ((one, 128, None, ctypes.c_void_p(8), 128, None, 5, 128, 1, 0.0, None), b"aligned"),
                       ((one, 128, one, one, 128, one, 5, 128, 17, 0.0, None), b"ny"),
                       ((one, 128, one, one, 128, one, 5, 128, 0, 0.0, None), b"ny"),
                       ((one, 128, None, one, 128, None, 5, 128, 1, float("nan"), None), b"beta")):
        rc = syrk(*args)
        assert rc == -2 and word in lib.nngp_last_error(), (args, lib.nngp_last_error())
    with pytest.raises(_lib.NngpError):
        _lib.check(rc)
    from nngp_src_amd import sparse
    for bad in (dict(m_cap=0), dict(m_cap=16385), dict(chunk_rows=100), dict(test_cap=0), dict(ny=17), dict(jitter=-1.0),
                dict(diag_reg=float("nan"))):
        with pytest.raises(ValueError):
            sparse.check_sparse_arguments(**dict(dict(m_cap=128, chunk_rows=128, test_cap=1, ny=1, diag_reg=1e-3, jitter=0.0), **bad))


def test_the_sparse_prototypes_bind_and_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_sparse.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.SPARSE_ABI_SYMBOLS)
    lib = _lib.load()
    counts = {}
    for name, body in re.findall(r"\bint (nngp_\w+)\(([^;]*)\);", text):
        counts[name] = len([a for a in body.split(",") if a.strip()])
    for name in _lib.SPARSE_ABI_SYMBOLS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == counts[name] and fn.restype is ctypes.c_int, name
    struct = re.search(r"typedef struct nngp_sparse_info_t \{(.*?)\} nngp_sparse_info_t;", text, re.S).group(1)
    fields = re.findall(r"\b(int64_t|double)\s+(\w+);", struct)
    ctype = {"int64_t": ctypes.c_int64, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.NngpSparseInfo._fields_)
    with open(os.path.join(ROOT, "include", "nngp_hip.h")) as f:
        assert "nngp_sparse" not in f.read()  # that header's symbol set is pinned to ABI_SYMBOLS
    import nngp_src_amd
    from nngp_src_amd import sparse
    assert nngp_src_amd.SparseGPModel is sparse.SparseGPModel and nngp_src_amd.select_inducing is sparse.select_inducing


def test_cli_sparse_flags_and_their_conflicts(capsys):
    from nngp_src_amd import train
    args = train.parse_args([])
    assert args.sparse == 0 and args.sparse_select == "greedy" and args.sparse_chunk == 8192 and args.sparse_jitter == 1e-8
    args = train.parse_args(["--sparse", "128", "--sparse_select", "random", "--sparse_chunk", "256", "--sparse_jitter", "1e-6"])
    assert (args.sparse, args.sparse_select, args.sparse_chunk, args.sparse_jitter) == (128, "random", 256, 1e-6)
    for bad in (["--sparse", "64", "--kernel_type", "ntk"], ["--sparse", "64", "--kernel_type", "gp"], ["--sparse", "64", "--loo"],
                ["--sparse", "64", "--tune_hyper", "5"], ["--sparse", "64", "--tune_hyper", "5", "--tune_ard"],
                ["--sparse", "64", "--sparse_chunk", "100"], ["--sparse", "-1"], ["--sparse", "64", "--sparse_select", "best"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2 and "--sparse" in capsys.readouterr().err, bad
    assert train.parse_args(["--kernel_type", "ntk", "--loo"]).sparse == 0  # without the flag nothing changes


def test_select_inducing_numpy_path_equals_the_reference(forest):
    from nngp_src_amd.sparse import select_inducing
    x = forest[0][:400]
    kernel, _ = S.oracle_kernel(1)

    def kernel_fn(x1, x2=None, get="nngp"):  # no device model behind it: the rule runs in NumPy
        assert get == "nngp" and x2 is None
        return kernel(x1, None)

    got = select_inducing(x, 60, kernel_fn, method="greedy")
    np.testing.assert_array_equal(got, R.greedy(kernel(x, None), 60, 0.0)[0])
    # more rows than candidates: the candidates are a seeded draw without replacement, the picks index x
    cand = np.sort(np.random.RandomState(10).choice(400, size=150, replace=False))
    got = select_inducing(x, 40, kernel_fn, method="greedy", candidates=150, seed=10)
    np.testing.assert_array_equal(got, cand[R.greedy(kernel(x[cand], None), 40, 0.0)[0]])
    rnd = select_inducing(x, 40, kernel_fn, method="random", seed=3)
    assert len(set(rnd.tolist())) == 40 and rnd.min() >= 0 and rnd.max() < 400
    np.testing.assert_array_equal(rnd, select_inducing(x, 40, kernel_fn, method="random", seed=3))
    for bad in (dict(m=0), dict(m=401), dict(m=10, method="best"), dict(m=10, candidates=5)):
        with pytest.raises(ValueError):
            select_inducing(x, kernel_fn=kernel_fn, **bad)
