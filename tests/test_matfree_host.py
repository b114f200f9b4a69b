"""The matrix-free exact NNGP posterior without a GPU: the NumPy reference (matfree_reference.py: PCG with the sparse model's
Woodbury preconditioner) against the oracle's exact posterior on the forest golden, column independence of the reference, the
argument checks of include/nngp_matfree.h that need no device, its bindings, and the command line.

The forest figures (oracle kernel, diag_reg 1e-3, greedy inducing rows, tol 1e-10; measured in NumPy float64, printed again here):

  hidden ReLU layers   m      CG iterations for alpha   worst over 200 cross columns   mean error / max|mean|   variance, relative
  1                    0      669                       (not formed here)              1.2e-10                  (not formed here)
  1                    128    68                        47                             1.3e-10                  8.4e-8
  3                    128    105                       73                             1.5e-10                  1.4e-7
  1, first 300 rows    40     100                       76                             1.2e-10                  5.5e-8
"""
import ctypes
import os
import re

import numpy as np
import pytest

import matfree_reference as M
import sparse_reference as S
from nngp_src_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_against_the_oracle_on_the_forest_golden():
    """alpha iterations <= 120 at m = 128; without a preconditioner at least 4 x as many; means within 1e-8 of max |mean| and
    variances within 1e-5 relative of oracle.Posterior."""
    none = M.forest_case(1, 1000, 0, with_var=False)
    it0 = none["ref"].fit_info["iterations"]
    print("1 layer, m = 0: alpha iterations %d, mean %.2e of max |mean|" % (it0, none["e_mean"]))
    assert none["ref"].fit_info["converged"] and none["e_mean"] <= 1e-8
    for n_relu, n, m in ((1, 1000, 128), (3, 1000, 128), (1, 300, 40)):
        case = M.forest_case(n_relu, n, m)
        info = case["ref"].fit_info
        worst = max(int(i["col_iterations"].max()) for i in case["infos"])
        print("%d layer(s), n = %d, m = %d: alpha iterations %d, worst over the 200 cross columns %d, mean %.2e of max |mean|, "
              "variance %.2e relative, true residual %.2e, restarts %d" % (n_relu, n, m, info["iterations"], worst, case["e_mean"],
                                                                         case["e_var"], info["rel_residual"].max(), info["restarts"]))
        assert info["converged"] and all(i["converged"] for i in case["infos"])
        assert info["rel_residual"].max() <= 1e-10
        assert case["e_mean"] <= 1e-8 and case["e_var"] <= 1e-5
        if m == 128:
            assert info["iterations"] <= 120
    assert it0 >= 4 * M.forest_case(1, 1000, 128)["ref"].fit_info["iterations"]


def test_a_column_alone_equals_the_column_inside_a_block():
    x, y, xt, _ = M.forest()
    x, y = x[:200], y[:200]
    kernel, diag = S.oracle_kernel(1)
    ref = M.MatfreeReference(kernel, diag, columnwise=True).fit(x, y, x[M.forest_picks(1, 200, 24)], chunk_rows=128)
    b = np.random.default_rng(5).standard_normal((7, 200))
    b[4] = 0.0  # a zero right-hand side is solved before the first step
    block, info = ref.solve(b)
    alone, info1 = ref.solve(b[3:4])
    print("block of 7: iterations %d, per column %s; column 3 alone: %d" % (info["iterations"], info["col_iterations"].tolist(),
                                                                           info1["iterations"]))
    assert alone.tobytes() == block[3:4].tobytes()
    assert info1["iterations"] == info["col_iterations"][3] <= info["iterations"]
    assert info["col_iterations"][4] == 0 and np.all(block[4] == 0.0)
    np.testing.assert_allclose(block, np.linalg.solve(ref.k + ref.sigma2 * np.eye(200), b.T).T, rtol=0, atol=1e-7 * np.abs(block).max())


def test_a_stalled_solve_is_reported():
    x, y, _, _ = M.forest()
    kernel, diag = S.oracle_kernel(1)
    ref = M.MatfreeReference(kernel, diag, max_iter=3).fit(x[:200], y[:200])
    info = ref.fit_info
    assert not info["converged"] and info["iterations"] == 3 and info["rel_residual"].max() > 1e-10 and info["k_passes"] == 4


def _arch():
    return _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("relu",)])


def test_argument_validation_without_gpu():
    """Every -2 of include/nngp_matfree.h that needs no handle: these fail their checks before any GPU work.  (The checks on a
    live handle -- n > n_cap, r > rhs_cap, the full covariance, a non-finite tol -- are in test_gpu_matfree.py.)"""
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced
    other = ctypes.c_void_p(4096)
    arch = _arch()
    h = ctypes.c_void_p()
    good = dict(n_cap=1000, m_cap=128, chunk=256, rhs=16, d=8, ny=1, get=_lib.GET_NNGP, reg=1e-3, absolute=0, jitter=1e-8)
    table = _lib.make_groups(((0, 2), (2, 4)), (1.0, 1.0), 1.0)

    def create(out=ctypes.byref(h), a=ctypes.byref(arch), groups=None, **kw):
        p = dict(good, **kw)
        return lib.nngp_matfree_create(out, p["n_cap"], p["m_cap"], p["chunk"], p["rhs"], p["d"], p["ny"], a, groups, p["get"], p["reg"],
                                       p["absolute"], p["jitter"])

    for kw, word in ((dict(out=None), b"NULL"), (dict(a=None), b"NULL"), (dict(get=_lib.GET_NTK), b"NNGP"),
                     (dict(groups=ctypes.byref(table)), b"additive"), (dict(n_cap=0), b"n_cap"), (dict(m_cap=-1), b"m_cap"),
                     (dict(m_cap=16385), b"m_cap"), (dict(chunk=0), b"chunk_rows"), (dict(chunk=200), b"chunk_rows"),
                     (dict(rhs=0), b"rhs_cap"), (dict(rhs=4097), b"rhs_cap"), (dict(d=0), b"d >= 1"), (dict(ny=0), b"ny"),
                     (dict(ny=17), b"ny"), (dict(jitter=-1e-9), b"jitter"), (dict(jitter=float("nan")), b"jitter"),
                     (dict(reg=-1.0), b"diag_reg"), (dict(reg=float("inf")), b"diag_reg")):
        rc = create(**kw)
        assert rc == -2 and word in lib.nngp_last_error(), (kw, rc, lib.nngp_last_error())
        assert not h.value
    for rc in (lib.nngp_matfree_fit(None, one, one, 4, None, 0, 1e-10, 10, None), lib.nngp_matfree_solve(None, one, 4, 1, other, 4, 1e-10, 10, None),
               lib.nngp_matfree_predict(None, one, 4, _lib.COV_DIAG, one, one, 1e-10, 10, None), lib.nngp_matfree_alpha(None, one, None),
               lib.nngp_matfree_info(None, None)):
        assert rc == -2 and b"NULL" in lib.nngp_last_error()
    assert lib.nngp_matfree_destroy(None) == 0
    kmv = lib.nngp_kmv_f64
    a = ctypes.byref(arch)
    for args, word in (((None, 8, one, 8, 1, other, 8, 4, a, 0.0, None), b"NULL"), ((one, 8, None, 8, 1, other, 8, 4, a, 0.0, None), b"NULL"),
                       ((one, 8, other, 8, 1, None, 8, 4, a, 0.0, None), b"NULL"), ((one, 8, one, 8, 1, other, 8, 4, a, 0.0, None), b"aliases"),
                       ((one, 8, other, 8, 1, other, 8, 4, None, 0.0, None), b"arch"), ((one, 8, other, 8, 1, other, 0, 4, a, 0.0, None), b"n"),
                       ((one, 8, other, 8, 0, other, 8, 4, a, 0.0, None), b"r"), ((one, 8, other, 8, 1, other, 8, 0, a, 0.0, None), b"d >= 1"),
                       ((one, 7, other, 8, 1, other, 8, 4, a, 0.0, None), b"ldo"), ((one, 8, other, 7, 1, other, 8, 4, a, 0.0, None), b"ldv"),
                       ((one, 8, other, 8, 1, other, 8, 4, a, float("nan"), None), b"diag_add"),
                       ((one, 8, other, 8, 1, other, 8, 4, a, float("inf"), None), b"diag_add")):
        rc = kmv(*args)
        assert rc == -2 and word in lib.nngp_last_error(), (args, lib.nngp_last_error())
    with pytest.raises(_lib.NngpError):
        _lib.check(rc)
    from nngp_src_amd import matfree
    ok = dict(n_cap=100, m=16, chunk_rows=128, rhs_cap=16, ny=1, diag_reg=1e-3, jitter=0.0, tol=1e-10, max_iter=100)
    matfree.check_matfree_arguments(**ok)
    for bad in (dict(n_cap=0), dict(m=-1), dict(m=16385), dict(chunk_rows=100), dict(rhs_cap=0), dict(rhs_cap=4097), dict(ny=17),
                dict(jitter=-1.0), dict(diag_reg=float("nan")), dict(tol=0.0), dict(tol=1.0), dict(tol=float("nan")), dict(max_iter=0)):
        with pytest.raises(ValueError):
            matfree.check_matfree_arguments(**dict(ok, **bad))


def test_python_refuses_what_the_model_does_not_cover():
    from nngp_src_amd import matfree, stax
    from nngp_src_amd.kernel_spec import KernelSpec
    spec = KernelSpec([1.0, 1.0], [0.0, 0.0])
    assert matfree.check_matfree_spec(spec) is spec
    with pytest.raises(ValueError, match="NNGP"):
        matfree.check_matfree_spec(spec, get="ntk")
    with pytest.raises(ValueError, match="groups"):
        matfree.check_matfree_spec(spec.replace(groups="pairs"))
    with pytest.raises(ValueError, match="input_scale"):
        matfree.check_matfree_spec(spec.replace(input_scale=np.ones(4)))
    assert matfree.check_cov(None) == _lib.COV_NONE and matfree.check_cov("diag") == _lib.COV_DIAG
    for cov in ("full", True):
        with pytest.raises(ValueError, match="cov"):
            matfree.check_cov(cov)
    # the constructor refuses before it looks for a device
    kernel_fn = stax.serial(stax.Dense(512), stax.Relu(), stax.Dense(1))[2]
    for kw in (dict(get="ntk"), dict(groups="pairs"), dict(input_scale=np.ones(4))):
        with pytest.raises(ValueError):
            matfree.MatrixFreeGPModel(100, 4, [1.0, 1.0], [0.0, 0.0], m=8, **kw)
    with pytest.raises(ValueError):
        matfree.MatrixFreeGPModel.from_kernel_fn(kernel_fn.with_groups("pairs"), 100, 4, m=8)


def test_the_matfree_prototypes_bind_and_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_matfree.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.MATFREE_ABI_SYMBOLS)
    lib = _lib.load()
    counts = {}
    for name, body in re.findall(r"\bint (nngp_\w+)\(([^;]*)\);", text):
        counts[name] = len([a for a in body.split(",") if a.strip()])
    for name in _lib.MATFREE_ABI_SYMBOLS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == counts[name] and fn.restype is ctypes.c_int, name
    struct = re.search(r"typedef struct nngp_matfree_info_t \{(.*?)\} nngp_matfree_info_t;", text, re.S).group(1)
    fields = re.findall(r"\b(int64_t|int32_t|double)\s+(\w+);", struct)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.NngpMatfreeInfo._fields_)
    for header in ("nngp_hip.h", "nngp_sparse.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert "nngp_matfree" not in f.read()  # those headers' symbol sets are pinned
    import nngp_src_amd
    from nngp_src_amd import matfree
    assert nngp_src_amd.MatrixFreeGPModel is matfree.MatrixFreeGPModel and nngp_src_amd.matfree_mse_ensemble is matfree.matfree_mse_ensemble


def test_cli_matrix_free_flags_and_their_conflicts(capsys):
    from nngp_src_amd import train
    args = train.parse_args([])
    assert args.matrix_free == 0 and args.matrix_free_tol == 1e-10 and args.matrix_free_iters == 1000
    args = train.parse_args(["--matrix_free", "128", "--matrix_free_tol", "1e-8", "--matrix_free_iters", "50"])
    assert (args.matrix_free, args.matrix_free_tol, args.matrix_free_iters) == (128, 1e-8, 50)
    for bad in (["--matrix_free", "64", "--sparse", "64"], ["--matrix_free", "64", "--kernel_type", "ntk"],
                ["--matrix_free", "64", "--kernel_type", "gp"], ["--matrix_free", "64", "--loo"], ["--matrix_free", "64", "--tune_hyper", "5"],
                ["--matrix_free", "64", "--tune_hyper", "5", "--tune_ard"],
                ["--matrix_free", "64", "--tune_hyper", "5", "--additive", "pairs", "--tune_additive"],
                ["--matrix_free", "64", "--additive", "pairs"], ["--matrix_free", "-1"], ["--matrix_free", "64", "--matrix_free_tol", "0"],
                ["--matrix_free", "64", "--matrix_free_iters", "0"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2 and "--matrix_free" in capsys.readouterr().err, bad
    assert train.parse_args(["--kernel_type", "ntk", "--loo"]).matrix_free == 0  # without the flag nothing changes


def test_estimator_refuses_matrix_free_with_sparse_or_ntk():
    from nngp_src_amd.estimator import Estimator
    for kw in (dict(sparse=64), dict(kernel_type="ntk"), dict(groups="pairs")):
        with pytest.raises(ValueError, match="matrix_free"):
            Estimator("forest", "", "", encoder=object(), matrix_free=64, **kw)
