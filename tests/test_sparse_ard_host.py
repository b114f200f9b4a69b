"""Per-feature relevances on the sparse NNGP evidence without a GPU: the NumPy reference (sparse_ard_reference.py) against
differences of its own 80-bit value, its distance to 80-bit arithmetic on every case of the GPU tests, the exact evidence's
relevance gradient in the limit U = X, the tuning loop on the NumPy evaluator, the command line and the bindings."""
import ctypes
import os
import re

import numpy as np
import pytest

import nngp_ard_reference as AR
import nngp_mll_reference as MR
import sparse_ard_reference as A
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
    u = x[rng.choice(60, 9, replace=False)]
    return A.SparseArdEvidence(x, y, u, jitter=1e-6), A.SparseArdEvidence(x, y, u, jitter=1e-6, dtype=np.longdouble)


NETS = [(2, ("relu",)), (4, ("relu",)), (3, ("abrelu", 0.1, 1.0))]


@pytest.mark.parametrize("bound", E.BOUNDS)
@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("nd,act,b_std", [(nd, act, b) for (nd, act), b in zip(NETS, (0.0, 0.05, 0.05))])
def test_relevance_gradient_against_differences_of_the_80_bit_value(small, nd, act, b_std, absolute, bound):
    """Central differences of the reference's own 80-bit value with step h = 1e-5 max(s_k, 1): truncation h^2 f''' / 6 ~ 1e-10 of
    the halves, and the 80-bit value's noise (float64 kernel blocks: 1e-16 of sums of size 1e2) over h stays below that.  Gate:
    1e-6 of max(|quad_k|, |trace_k|).  The feature with s_k = 0 has no left neighbour (a relevance is >= 0); it takes the
    second-order one-sided quotient (-3 f(0) + 4 f(h) - f(2h)) / 2h, whose truncation is h^2 f''' / 3."""
    r64, r80 = small
    v, c, acts, lam = [1.3] * nd, [b_std ** 2] * nd, [act] * (nd - 1), 1e-2
    rel = A.relevances(6, zero_at=2)
    o = r64.evaluate64(v, c, acts, lam, rel, absolute, bound)
    worst = 0.0
    for k in range(6):
        h = 1e-5 * max(rel[k], 1.0)

        def f(dt):
            rr = rel.copy()
            rr[k] += dt
            return r80.value(v, c, acts, lam, rr, absolute, bound)

        fd = (f(h) - f(-h)) / (2 * h) if rel[k] > 0.0 else (-3 * f(0.0) + 4 * f(h) - f(2 * h)) / (2 * h)
        scale = max(abs(o["quad_s"][k]), abs(o["trace_s"][k]))
        worst = max(worst, abs(float(fd) - o["grad_s"][k]) / scale)
        assert abs(float(fd) - o["grad_s"][k]) <= 1e-6 * scale, (k, float(fd), o["grad_s"][k], scale)
    print("%d Dense %s b_std %g %s %s: worst |fd - grad_s| / max(|quad|, |trace|) = %.2e" % (nd, act[0], b_std, bound,
                                                                                           "absolute" if absolute else "relative", worst))


def test_relevance_one_is_the_plain_evidence(small):
    """s = 1 scales nothing: value, gradient and halves are those of sparse_evidence_reference on the same rows."""
    r64, _ = small
    v, c, acts = [1.3, 1.3], [0.0025, 0.0025], [("relu",)]
    o = r64.evaluate64(v, c, acts, 1e-2, np.ones(6), False, "vfe")
    p = E.SparseEvidence(r64.x, r64.y, r64.u, jitter=1e-6).evaluate64(v, c, acts, 1e-2, False, "vfe")
    assert o["nlml"] == p["nlml"] and np.array_equal(o["grad"], p["grad"])


@pytest.mark.parametrize("case", A.cases(), ids=A.case_id)
def test_reference_error_on_the_gpu_cases(golden_dir, case):
    """The float64 reference against its 80-bit rerun on every case the GPU tests use: within 1e-9 for the value, the gradient and
    the relevance gradient, so that the GPU gate of max(1e-8, 10 x this) cannot hide a device error; and cond(K~_uu) <= 1e5."""
    _, _, rel, _, ref, (d_val, d_grad, d_s) = A.case_reference(golden_dir, case)
    print("%s: cond(K~_uu) %.2e, float64 vs 80-bit: value %.2e, gradient %.2e, relevance gradient %.2e"
          % (A.case_id(case), ref["cond_kuu"], d_val, d_grad, d_s))
    assert np.sum(rel == 0.0) == 1 and np.all(rel >= 0.0)
    assert ref["cond_kuu"] <= E.COND_CAP and d_val <= 1e-9 and d_grad <= 1e-9 and d_s <= 1e-9


@pytest.fixture(scope="module")
def forest256(golden_dir):
    g = np.load(os.path.join(golden_dir, "forest_n256_m64.npz"))
    return g["X_train"][:256], g["Y_train"][:256].reshape(-1)


def exact_limit_s(x, y, net, rel, absolute, lam):
    """({bound: (sparse reference at U = X, jitter 0, 10 x its distance to its 80-bit rerun as (value, gradient, relevance gradient
    -- the last with the exact reference's distance to its own 80-bit rerun added))}, the exact reference
    nngp_ard_reference.Oracle, its scale max(|half1|, |half2|)) -- shared with the GPU test of the same limit."""
    w, b, acts = net
    v, c = MR.variances(w, b)
    exact = AR.Oracle(x, y).full(v, c, acts, lam, rel, absolute)
    g80, h1, h2 = A.exact_grad_s(x, y, rel, v, c, acts, lam, absolute, np.longdouble)
    scale = np.maximum(np.abs(h1), np.abs(h2)).astype(np.float64)
    d_exact = float(np.max(np.abs(exact["grad_s"] - g80.astype(np.float64)) / scale))
    r64 = A.SparseArdEvidence(x, y, x, jitter=0.0)
    r80 = A.SparseArdEvidence(x, y, x, jitter=0.0, dtype=np.longdouble)
    r80._tan = r64._tan
    out = {}
    for bound in E.BOUNDS:
        got = r64.evaluate64(v, c, acts, lam, rel, absolute, bound)
        d_val, d_grad, d_s = A.distance(got, r80.full(v, c, acts, lam, rel, absolute, bound))
        out[bound] = (got, (10.0 * d_val, 10.0 * d_grad, 10.0 * (d_s + d_exact)))
    return out, exact, scale


@pytest.mark.parametrize("net", E.EXACT_NETS)
@pytest.mark.parametrize("absolute,lam", [(False, 1e-3), (True, 1.0)])
def test_exact_limit_is_the_exact_relevance_gradient(forest256, net, absolute, lam):
    """U = X (the first 256 forest rows), jitter 0: both bounds are the exact NLML at the same relevances, and so are their
    relevance gradients -- a rectangular pass over K(X, X) without the diagonal rule and a symmetric one with it against the one
    symmetric pass of the exact evidence.  Bound: 10 x the two references' combined distance to their 80-bit reruns."""
    x, y = forest256
    rel = A.relevances(20)
    res, exact, scale = exact_limit_s(x, y, net, rel, absolute, lam)
    for bound, (got, (b_val, _, b_s)) in res.items():
        e_val = abs(got["nlml"] - exact["nlml"]) / abs(exact["nlml"])
        e_s = float(np.max(np.abs(got["grad_s"] - exact["grad_s"]) / scale))
        print("exact limit %s, %d Dense, %s: value %.2e (bound %.2e), relevance gradient %.2e of max(|half1|, |half2|) (bound %.2e)"
              % (bound, len(net[0]), "absolute" if absolute else "relative", e_val, b_val, e_s, b_s))
        assert e_val <= max(b_val, 1e-12) and e_s <= b_s


def tuning_run(x, y, idx, steps, ard_groups=None, chunk_rows=None, report=None):
    """sparse.tune_hyperparameters(ard=True) driven by the NumPy evaluator -- shared with the GPU test that reproduces it."""
    from nngp_src_amd import sparse, stax
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.0, b_std=0.05), stax.Relu(), stax.Dense(1, W_std=1.0, b_std=0.05))
    return kf, sparse.tune_hyperparameters(kf, x, y, len(idx), bound="vfe", steps=steps, lr=0.05, report=report, ard=True,
                                           ard_groups=ard_groups, evaluator=A.Evaluator(x, y, x[idx], "vfe", chunk_rows=chunk_rows))


def test_tuning_loop_with_relevances_on_the_numpy_evaluator(golden_dir):
    from nngp_src_amd import sparse
    x, y = E.case_rows(golden_dir, "unit", 400)
    idx, _ = S.greedy_inducing(E.kernels(*MR.variances([1.0, 1.0], [0.05, 0.05]), [("relu",)])[0], x, 64)
    printed = []
    kf, (kf_t, lam_t, hist) = tuning_run(x, y, idx, 10, report=printed.append)
    s = kf_t.input_scale ** 2
    print("history: %s; tuned W_std %s b_std %s diag_reg %.6g\nrelevances %s" % (["%.3f" % h for h in hist], kf_t.w_std, kf_t.b_std, lam_t, s))
    assert len(hist) == 10 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, h) for i, h in enumerate(hist)]
    assert s.shape == (20,) and np.all(s > 0.0) and abs(np.mean(np.log(s))) <= 1e-12 and np.ptp(s) > 0.0
    _, (kf_p, _, hist_p) = tuning_run(x, y, idx, 10, ard_groups="pairs")
    sp = kf_p.input_scale ** 2
    assert hist_p[-1] < hist_p[0] and np.array_equal(sp[0::2], sp[1::2]) and abs(np.mean(np.log(sp))) <= 1e-12 and np.ptp(sp) > 0.0
    # an input_scale is the start of the relevances with ard, and still refused without
    start = np.exp(0.1 * np.arange(20))
    _, _, h_in = sparse.tune_hyperparameters(kf.with_input_scale(np.sqrt(start)), x, y, 64, steps=1, report=None, ard=True,
                                             evaluator=A.Evaluator(x, y, x[idx]))
    _, _, h_ri = sparse.tune_hyperparameters(kf, x, y, 64, steps=1, report=None, ard=True, relevance_init=start,
                                             evaluator=A.Evaluator(x, y, x[idx]))
    assert np.allclose(h_in, h_ri, rtol=1e-12, atol=0.0) and h_in[0] != hist[0]  # sqrt(start)^2 is start to an ulp
    with pytest.raises(ValueError, match="input_scale"):
        sparse.tune_hyperparameters(kf.with_input_scale(np.ones(20)), x, y, 64, steps=1, report=None, evaluator=E.Evaluator(x, y, x[idx]))
    with pytest.raises(ValueError, match="groups"):
        sparse.tune_hyperparameters(kf.with_groups("pairs"), x, y, 64, steps=1, report=None, ard=True, evaluator=A.Evaluator(x, y, x[idx]))


def test_cli_sparse_tune_ard_flags(capsys):
    from nngp_src_amd import train
    args = train.parse_args([])
    assert args.sparse_tune_ard is False
    args = train.parse_args(["--sparse", "128", "--sparse_tune", "7", "--sparse_tune_ard", "--ard_groups", "pairs"])
    assert (args.sparse, args.sparse_tune, args.sparse_tune_ard, args.ard_groups) == (128, 7, True, "pairs")
    for bad, word in ((["--sparse_tune_ard"], "--sparse_tune_ard"), (["--sparse", "64", "--sparse_tune_ard"], "--sparse_tune_ard"),
                      (["--sparse_tune", "3", "--sparse_tune_ard"], "--sparse_tune_ard"),
                      (["--sparse", "64", "--sparse_tune", "3", "--sparse_tune_ard", "--ard_groups", "triples"], "--ard_groups"),
                      (["--sparse", "64", "--sparse_tune", "3", "--sparse_tune_ard", "--tune_ard"], "--sparse"),
                      (["--sparse", "64", "--tune_hyper", "5", "--tune_ard"], "--sparse")):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad


def test_the_sparse_ard_prototypes_bind_and_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_sparse_ard.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.SPARSE_ARD_ABI_SYMBOLS)
    lib = _lib.load()
    for name, body in re.findall(r"\bint (nngp_\w+)\(([^;]*)\);", text):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len([a for a in body.split(",") if a.strip()]) and fn.restype is ctypes.c_int, name
    # every -2 that needs no handle
    one = ctypes.c_void_p(16)  # never dereferenced
    out = ctypes.c_double()
    pout = ctypes.byref(out)
    arch = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("relu",)])
    erf = _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)])
    s3 = (ctypes.c_double * 3)(1.0, 0.0, 2.0)
    for rc in (lib.nngp_sparse_reserve_ard(None), lib.nngp_sparse_set_relevance(None, s3), lib.nngp_sparse_ard_terms(None, pout, 1),
               lib.nngp_sparse_evidence_grad_ard(None, one, one, 4, 1, pout, pout, pout, None),
               lib.nngp_sparse_evidence_grad_ard(one, one, one, 4, 1, pout, pout, None, None),
               lib.nngp_sparse_ard_rect(None, 4, one, 4, 3, ctypes.byref(arch), s3, one, 4, one, one, pout, None),
               lib.nngp_sparse_ard_rect(one, 4, one, 4, 3, ctypes.byref(arch), None, one, 4, one, one, pout, None)):
        assert rc == -2 and b"NULL" in lib.nngp_last_error()
    rect = lib.nngp_sparse_ard_rect
    assert rect(one, 4, one, 4, 3, ctypes.byref(arch), s3, one, 3, one, one, pout, None) == -2 and b"ld" in lib.nngp_last_error()
    assert rect(one, 0, one, 4, 3, ctypes.byref(arch), s3, one, 4, one, one, pout, None) == -2
    assert rect(one, 4, one, 4, 3, ctypes.byref(erf), s3, one, 4, one, one, pout, None) == -2 and b"Erf" in lib.nngp_last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        sb = (ctypes.c_double * 3)(1.0, bad, 2.0)
        assert rect(one, 4, one, 4, 3, ctypes.byref(arch), sb, one, 4, one, one, pout, None) == -2
        assert b"relevance 1" in lib.nngp_last_error()
