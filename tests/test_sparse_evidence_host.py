"""The sparse NNGP evidence without a GPU: the NumPy reference (sparse_evidence_reference.py) against central differences of its
own value, against the exact evidence of nngp_mll_reference.py in the limit U = X, the ordering of the bounds, its own distance
to 80-bit arithmetic on every case of the GPU tests, the tuning loop on the NumPy evaluator, the command line and the bindings."""
import ctypes
import os
import re

import numpy as np
import pytest

import nngp_mll_reference as MR
import sparse_evidence_reference as E
import sparse_reference as S
from nngp_src_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    """60 Gaussian rows, d = 6, 9 of them as inducing rows: well conditioned, so the difference quotients are clean."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 6))
    y = np.sin(x[:, 0]) + 0.1 * rng.standard_normal(60)
    return E.SparseEvidence(x, y, x[rng.choice(60, 9, replace=False)], jitter=1e-6)


NETS = [(2, ("relu",)), (4, ("relu",)), (3, ("abrelu", 0.1, 1.0))]


@pytest.mark.parametrize("bound", E.BOUNDS)
@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("b_std", [0.0, 0.05])
@pytest.mark.parametrize("nd,act", NETS)
def test_gradient_against_central_differences_of_the_value(small, nd, act, b_std, absolute, bound):
    """Five-point stencil with h = 1e-4 of the parameter (of 1e-2 where the parameter is 0: the value is smooth in c_l through 0).
    Its truncation error is h^4 f^(5) / 30 ~ 1e-16 relative and its rounding error eps |f| / h ~ 1e-16 * 1e2 / 1e-6 = 1e-8 absolute
    at worst, against halves of 1e0 .. 1e2: 1e-6 of max(|quad|, |trace|) leaves two digits of margin."""
    v, c, acts, lam = [1.3] * nd, [b_std ** 2] * nd, [act] * (nd - 1), 1e-2
    o = small.evaluate64(v, c, acts, lam, absolute, bound)
    worst = 0.0
    for p in range(2 * nd + 1):
        base = lam if p == 2 * nd else (v[p // 2] if p % 2 == 0 else max(c[p // 2], 1e-2))
        h = 1e-4 * base

        def f(dt):
            vv, cc, ll = list(v), list(c), lam
            if p == 2 * nd:
                ll += dt
            elif p % 2 == 0:
                vv[p // 2] += dt
            else:
                cc[p // 2] += dt
            return small.value_var(vv, cc, acts, ll, absolute, bound)

        fd = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        scale = max(abs(o["quad"][p]), abs(o["trace"][p]))
        worst = max(worst, abs(fd - o["grad"][p]) / scale)
        assert abs(fd - o["grad"][p]) <= 1e-6 * scale, (p, fd, o["grad"][p], scale)
    print("%d Dense %s b_std %g %s %s: worst |fd - grad| / max(|quad|, |trace|) = %.2e" % (nd, act[0], b_std, bound,
                                                                                         "absolute" if absolute else "relative", worst))


@pytest.fixture(scope="module")
def forest256(golden_dir):
    g = np.load(os.path.join(golden_dir, "forest_n256_m64.npz"))
    return g["X_train"][:256], g["Y_train"][:256].reshape(-1)


EXACT_NETS = E.EXACT_NETS


@pytest.mark.parametrize("net", EXACT_NETS)
@pytest.mark.parametrize("absolute,lam", [(False, 1e-3), (True, 1.0)])
def test_exact_limit_is_the_exact_evidence(forest256, net, absolute, lam):
    """U = X (the first 256 forest rows), jitter 0: both bounds are the exact NLML, and so are their gradients.  The bound is 10 x
    the distance between the float64 reference and its 80-bit rerun, measured here and printed."""
    x, y = forest256
    res, exact = E.exact_limit(x, y, net, absolute, lam)
    for bound, (got, (b_val, b_grad)) in res.items():
        e_val, e_grad = E.distance(got, exact)
        print("exact limit %s, %d Dense, %s: value %.2e (bound %.2e), gradient %.2e of max(|quad|, |trace|) (bound %.2e), cond(K) %.1e"
              % (bound, len(net[0]), "absolute" if absolute else "relative", e_val, b_val, e_grad, b_grad, got["cond_kuu"]))
        assert e_val <= b_val and e_grad <= b_grad


def test_ordering_of_the_bounds(golden_dir):
    """NLML_vfe >= NLML_dtc (their difference is a trace of a positive semi-definite matrix) and NLML_vfe >= the exact NLML (it
    is a lower bound of the evidence)."""
    x, y = E.case_rows(golden_dir, "unit", 300)
    for w, b, acts in EXACT_NETS:
        v, c = MR.variances(w, b)
        kernel, _ = E.kernels(v, c, acts)
        exact = MR.Oracle(x, y).full(v, c, acts, 1e-3, with_grad=False)["nlml"]
        for m in (20, 70, 150):
            idx, _ = S.greedy_inducing(kernel, x, m)
            ev = E.SparseEvidence(x, y, x[idx])
            dtc, vfe = (ev.value_var(v, c, acts, 1e-3, bound=bnd) for bnd in E.BOUNDS)
            print("%d Dense, m = %d: dtc %.6f, vfe %.6f, exact %.6f" % (len(w), m, dtc, vfe, exact))
            assert vfe >= dtc and vfe >= exact


@pytest.mark.parametrize("case", E.cases(), ids=E.case_id)
def test_reference_error_on_the_gpu_cases(golden_dir, case):
    """The float64 reference against its 80-bit rerun on every case the GPU tests use: within 1e-9, so that the GPU gate of
    max(1e-8, 10 x this) cannot hide a device error; and cond(K~_uu) <= 1e5, which the gate's factor 10 assumes."""
    _, _, _, ref, (d_val, d_grad) = E.case_reference(golden_dir, case)
    print("%s: cond(K~_uu) %.2e, float64 vs 80-bit: value %.2e, gradient %.2e" % (E.case_id(case), ref["cond_kuu"], d_val, d_grad))
    assert ref["cond_kuu"] <= E.COND_CAP and d_val <= 1e-9 and d_grad <= 1e-9


def test_tuning_loop_on_the_numpy_evaluator(golden_dir):
    from nngp_src_amd import sparse, stax
    x, y = E.case_rows(golden_dir, "unit", 400)
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.0, b_std=0.05), stax.Relu(), stax.Dense(1, W_std=1.0, b_std=0.05))
    idx, _ = S.greedy_inducing(E.kernels(*MR.variances(kf.w_std, kf.b_std), kf.activations)[0], x, 64)
    printed = []
    kf_t, lam_t, hist = sparse.tune_hyperparameters(kf, x, y, 64, bound="vfe", steps=10, lr=0.05, report=printed.append,
                                                    evaluator=E.Evaluator(x, y, x[idx], "vfe"))
    print("history: %s; tuned W_std %s b_std %s diag_reg %.6g" % (["%.3f" % h for h in hist], kf_t.w_std, kf_t.b_std, lam_t))
    assert len(hist) == 10 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, h) for i, h in enumerate(hist)]
    assert len(kf_t.w_std) == 2 and lam_t > 0
    # what the evidence does not cover is refused with a message, before any evaluation
    for bad, word in ((kf.with_groups("pairs"), "groups"), (kf.with_input_scale(np.ones(20)), "input_scale")):
        with pytest.raises(ValueError, match=word):
            sparse.tune_hyperparameters(bad, x, y, 64, steps=1, report=None, evaluator=E.Evaluator(x, y, x[idx]))
    with pytest.raises(ValueError, match="bound"):
        sparse.tune_hyperparameters(kf, x, y, 64, bound="fitc", steps=1, evaluator=E.Evaluator(x, y, x[idx]))
    _, _, kf_erf = stax.serial(stax.Dense(8), stax.Erf(), stax.Dense(1))
    with pytest.raises(ValueError, match="Erf"):
        sparse.tune_hyperparameters(kf_erf, x, y, 64, steps=1, evaluator=E.Evaluator(x, y, x[idx]))


def test_cli_sparse_tune_flags(capsys):
    from nngp_src_amd import train
    args = train.parse_args([])
    assert args.sparse_tune == 0 and args.sparse_bound == "vfe"
    args = train.parse_args(["--sparse", "128", "--sparse_tune", "7", "--sparse_bound", "dtc"])
    assert (args.sparse, args.sparse_tune, args.sparse_bound) == (128, 7, "dtc")
    for bad, word in ((["--sparse_tune", "3"], "--sparse"), (["--sparse", "64", "--sparse_tune", "-1"], "--sparse_tune"),
                      (["--sparse", "64", "--sparse_tune", "3", "--sparse_bound", "fitc"], "--sparse_bound"),
                      (["--sparse", "64", "--sparse_tune", "3", "--tune_hyper", "5"], "--sparse"),
                      (["--sparse", "64", "--tune_hyper", "5"], "--sparse"), (["--sparse", "64", "--tune_hyper", "5", "--tune_ard"], "--sparse"),
                      (["--sparse", "64", "--loo"], "--sparse"), (["--sparse", "64", "--kernel_type", "ntk"], "--sparse")):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad


def test_the_evidence_prototypes_bind_and_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_sparse_evidence.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.SPARSE_EVIDENCE_ABI_SYMBOLS)
    lib = _lib.load()
    for name, body in re.findall(r"\bint (nngp_\w+)\(([^;]*)\);", text):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in body.split(",") if a.strip()]) and fn.restype is ctypes.c_int, name
    codes = dict(re.findall(r"#define NNGP_BOUND_(\w+) (\d+)", text))
    assert {k.lower(): int(v) for k, v in codes.items()} == _lib.BOUNDS
    # every -2 that needs no handle
    one = ctypes.c_void_p(16)  # never dereferenced
    out = ctypes.c_double()
    arch = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("relu",)])
    erf = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])
    for rc in (lib.nngp_sparse_reserve_evidence(None), lib.nngp_sparse_set_kernel(None, ctypes.byref(arch), 1e-3, 0),
               lib.nngp_sparse_evidence(None, 1, ctypes.byref(out), None), lib.nngp_sparse_evidence_terms(None, ctypes.byref(out), 1),
               lib.nngp_sparse_evidence_grad(None, one, one, 4, 1, ctypes.byref(out), ctypes.byref(out), None),
               lib.nngp_sparse_adjoint_rect(None, 4, one, 4, 3, ctypes.byref(arch), one, 4, one, one, ctypes.byref(out), None)):
        assert rc == -2 and b"NULL" in lib.nngp_last_error()
    rect = lib.nngp_sparse_adjoint_rect
    assert rect(one, 4, one, 4, 3, ctypes.byref(arch), one, 3, one, one, ctypes.byref(out), None) == -2 and b"ld" in lib.nngp_last_error()
    assert rect(one, 0, one, 4, 3, ctypes.byref(arch), one, 4, one, one, ctypes.byref(out), None) == -2
    assert rect(one, 4, one, 4, 3, ctypes.byref(erf), one, 4, one, one, ctypes.byref(out), None) == -2 and b"Erf" in lib.nngp_last_error()
    from nngp_src_amd import sparse
    assert sparse.bound_code("vfe") == 1 and sparse.bound_code("dtc") == 0
