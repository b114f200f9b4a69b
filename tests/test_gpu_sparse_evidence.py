"""The sparse NNGP evidence and its gradient on the MI355X (include/nngp_sparse_evidence.h, csrc/sparse_evidence.hip) against the
NumPy float64 reference (sparse_evidence_reference.py: forward-mode tangents, 80-bit referee).

Gate.  Value: 1e-9 relative.  Each gradient component: g * max(|quad_p|, |trace_p|), the form of the exact evidence's gate, with
g = max(1e-8, 10 x the reference's own float64-vs-80-bit distance on the case) computed here and printed -- the factor 10 allows
for the cross build's 3e-14 times cond(K~_uu) <= 1e5, which enters twice (through M and through P).  On every case the reference's
distance is below 1e-9 (test_sparse_evidence_host.py asserts it on the CPU), so g = 1e-8 throughout.  Every test prints what it
measured before it asserts; DESIGN.md section 18 records the figures.
"""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import nngp_mll_reference as MR
import sparse_evidence_reference as E
from nngp_src_amd import _lib, mll, sparse, stax
from nngp_src_amd import train as train_cli
from nngp_src_amd.sparse import SparseGPModel

pytestmark = pytest.mark.gpu

LAM = 1e-3


def dev():
    return torch.device("cuda", 0)


def make_model(m_cap, net, chunk_rows, absolute=False, jitter=E.JITTER, reserve=True, **kw):
    w, b, acts = net
    model = SparseGPModel(m_cap, 20, w, b, activations=acts, diag_reg=LAM, chunk_rows=chunk_rows, jitter=jitter, test_cap=128,
                          diag_reg_absolute_scale=absolute, **kw)
    return model.reserve_evidence() if reserve else model


def gate_of(dist):
    return max(1e-8, 10.0 * dist[1])


def grad_error(g, ref):
    scale = np.maximum(np.abs(ref["quad"]), np.abs(ref["trace"]))
    return float(np.max(np.abs(g - ref["grad"]) / scale))


# ---- 1. value and gradient against the reference ----

@pytest.mark.parametrize("case", E.cases(), ids=E.case_id)
def test_value_and_gradient_against_the_reference(golden_dir, case):
    n, m, chunk, bound, absolute, net, _ = case
    x, y, idx, ref, dist = E.case_reference(golden_dir, case)
    g_gate = gate_of(dist)
    print("%s: cond(K~_uu) %.2e; reference vs 80-bit: value %.2e, gradient %.2e; gate g = %.1e" % (E.case_id(case), ref["cond_kuu"],
                                                                                                  dist[0], dist[1], g_gate))
    assert ref["cond_kuu"] <= E.COND_CAP
    model = make_model(m, net, chunk, absolute).set_inducing(x[idx]).add_rows(x, y).finish()
    info = model.info()
    assert (info["n"], info["m"], info["m_padded"], info["chunks"]) == (n, m, -(-m // 128) * 128, -(-n // chunk))
    value = model.evidence(bound)
    nlml, g = model.evidence_grad(x, y, bound)
    t = model.evidence_terms()
    e_val, e_grad = abs(nlml - ref["nlml"]) / abs(ref["nlml"]), grad_error(g, ref)
    print("device vs reference: value %.2e relative, gradient %.2e of max(|quad|, |trace|)" % (e_val, e_grad))
    print("  grad      %s\n  reference %s" % (g, ref["grad"]))
    scalars = [(k, float(t[k]), float(ref[k])) for k in ("logdet_half", "yy_cc", "tr_kff", "tr_g", "sigma2", "tr_binv", "b_b")]
    print("  " + ", ".join("%s %.3e" % (k, abs(a - b) / abs(b)) for k, a, b in scalars))
    assert e_val <= 1e-9
    assert e_grad <= g_gate
    assert value == nlml  # the value alone has the bits of the one that comes with the gradient
    assert np.array_equal(-0.5 * t["quad"] + 0.5 * t["trace"], g)
    assert abs(t["tr_kff"] - ref["tr_kff"]) <= 1e-12 * ref["tr_kff"] and abs(t["sigma2"] - ref["sigma2"]) <= 1e-12 * ref["sigma2"]
    nlml2, g2 = model.evidence_grad(x, y, bound)  # two identical evaluations: the same bits
    assert nlml2 == nlml and g2.tobytes() == g.tobytes()
    # a second fit on the same handle (new kernel and back): the same bits again
    model.set_kernel(([1.0] * len(net[0]), [0.1] * len(net[0]), net[2]), 2e-3).set_inducing(x[idx]).add_rows(x, y).finish()
    other = model.evidence_grad(x, y, bound)
    model.set_kernel(net, LAM).set_inducing(x[idx]).add_rows(x, y).finish()
    nlml3, g3 = model.evidence_grad(x, y, bound)
    assert other[0] != nlml and nlml3 == nlml and g3.tobytes() == g.tobytes()
    model.close()


# ---- 2. the exact limit on the device ----

@pytest.mark.parametrize("net", E.EXACT_NETS)
def test_exact_limit_against_the_exact_evidence_on_the_device(golden_dir, net):
    """U = X = the first 256 forest rows, jitter 0, against NNGPMarginalLikelihood.evaluate on the same rows.  cond(K) is 3e6 here,
    so the gate is not the 1e-8 of the cases above but what test_sparse_evidence_host.py measures for this limit -- the float64
    reference's distance to its 80-bit rerun -- times 10, with the floors of the gate above (1e-9 for the value, 1e-8 for g)."""
    g = np.load(os.path.join(golden_dir, "forest_n256_m64.npz"))
    x, y = g["X_train"][:256], g["Y_train"][:256].reshape(-1)
    res, _ = E.exact_limit(x, y, net, False, LAM)
    exact = mll.NNGPMarginalLikelihood(256, 20).set_train(x, y)
    nlml_e, g_e = exact.evaluate(net, LAM, False)
    te = exact.terms()
    scale = np.maximum(np.abs(te["quad"]), np.abs(te["trace"]))
    exact.close()
    model = make_model(256, net, 128, jitter=0.0).set_inducing(x).add_rows(x, y).finish()
    for bound in E.BOUNDS:
        b_val, b_grad = max(1e-9, res[bound][1][0]), max(1e-8, res[bound][1][1])
        nlml, grad = model.evidence_grad(x, y, bound)
        e_val, e_grad = abs(nlml - nlml_e) / abs(nlml_e), float(np.max(np.abs(grad - g_e) / scale))
        print("exact limit %s, %d Dense: value %.2e (gate %.2e), gradient %.2e of max(|quad|, |trace|) (gate %.2e)"
              % (bound, len(net[0]), e_val, b_val, e_grad, b_grad))
        assert e_val <= b_val and e_grad <= b_grad
    model.close()


# ---- 3. the rectangular adjoint pass alone ----

@pytest.mark.parametrize("c,m,d", [(65, 63, 33), (130, 128, 20)])
@pytest.mark.parametrize("net", [([1.2, 0.9], [0.05, 0.0], [("relu",)]),
                                 ([1.2, 0.9, 1.1, 1.0], [0.0, 0.1, 0.02, 0.05], [("relu",), ("abrelu", 0.1, 1.0), ("relu",)]),
                                 # 5 and 9 Dense layers: the NLC = 8 and NLC = 16 instantiations of the pass
                                 ([1.2, 0.9, 1.1, 1.0, 1.3], [0.0, 0.1, 0.02, 0.05, 0.0], [("relu",), ("abrelu", 0.1, 1.0)] * 2),
                                 ([1.2, 1.1] * 4 + [1.0], [0.0, 0.05, 0.0] * 3, [("relu",)] * 7 + [("abrelu", 0.1, 1.0)])])
def test_rectangular_adjoint_pass_alone(c, m, d, net):
    """A random dense seed (NaN beyond its m logical columns) and a random rank-one seed against the reference's contraction with
    the forward-mode tangents.  Bound: 1e-12 sum_ij |seed_ij dK_ij| -- the kernel build's documented 3e-14 per entry and layer, at
    most three hidden layers and the two factors of the reverse sweep, a factor 5 over their sum (a factor 2 for the eight hidden
    layers of the deepest network; per entry the pass is held far tighter in test_gpu_adjoint_angles.py)."""
    rng = np.random.default_rng(c + m)
    x, u = rng.standard_normal((c, d)), rng.standard_normal((m, d))
    u[3] = x[7]  # a training row that is also an inducing row takes the general formula
    x[11] = 0.0  # q = 0 with b_0 = 0 in the second network
    beta, gamma, seed = rng.standard_normal(c), rng.standard_normal(m), rng.standard_normal((c, m))
    ld = m + 5
    sd = torch.full((c, ld), float("nan"), dtype=torch.float64, device=dev())
    sd[:, :m] = torch.from_numpy(seed).to(dev())
    w, b, acts = net
    nd = len(w)
    lib = _lib.load()
    arch = _lib.make_arch_act(w, b, acts)
    xd, ud, bd, gd = (torch.from_numpy(a).to(dev()) for a in (x, u, beta, gamma))

    def run():
        out = (ctypes.c_double * (4 * nd))()
        _lib.check(lib.nngp_sparse_adjoint_rect(_lib.ptr(xd), c, _lib.ptr(ud), m, d, ctypes.byref(arch), _lib.ptr(sd), ld, _lib.ptr(bd),
                                                _lib.ptr(gd), out, _lib.stream_ptr()), lib)
        return np.array(out[:])

    got = run()
    v, cc = MR.variances(w, b)
    rank1 = np.outer(beta, gamma)
    worst = 0.0
    for p in range(2 * nd):
        dk = E.kernel_rect(x, u, v, cc, acts, param=p)[1]
        for half, s in ((0, rank1), (1, seed)):
            want, bound = float(np.sum(s * dk)), 1e-12 * float(np.sum(np.abs(s * dk)))
            err = abs(got[half * 2 * nd + p] - want)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    print("rectangular pass c %d m %d d %d, %d Dense: worst error %.2e of its bound" % (c, m, d, nd, worst))
    assert np.all(np.isfinite(got)) and worst <= 1.0
    assert run().tobytes() == got.tobytes()


# ---- 4. chunking ----

def test_chunks_of_128_against_one_chunk(golden_dir):
    case = E.cases()[4]  # n = 1000, m = 200, vfe
    n, m, _, bound, absolute, net, _ = case
    x, y, idx, ref, dist = E.case_reference(golden_dir, case)
    out = []
    for chunk in (128, 1024):
        model = make_model(m, net, chunk, absolute).set_inducing(x[idx]).add_rows(x, y).finish()
        out.append(model.evidence_grad(x, y, bound))
        model.close()
    scale = np.maximum(np.abs(ref["quad"]), np.abs(ref["trace"]))
    e_val, e_grad = abs(out[0][0] - out[1][0]) / abs(out[1][0]), float(np.max(np.abs(out[0][1] - out[1][1]) / scale))
    print("chunks of 128 vs one chunk: value %.2e, gradient %.2e of max(|quad|, |trace|) (gate %.1e)" % (e_val, e_grad, gate_of(dist)))
    assert e_val <= 1e-12 and e_grad <= gate_of(dist)


def test_m_padded_to_2048_takes_the_split_k_products(golden_dir):
    """m = 1930 (mp = 2048) with chunks of 1024 rows: the one size at which the float64 GEMM splits its K range -- the m^3 products
    of the once-per-call part, in place on their C_in, and D_c = K_cu M'.  2048 Gaussian rows, random inducing rows, jitter 1e-8.
    No 80-bit rerun at this size; the gate is that of the cases above with the conditioning put in: g = max(1e-8, 10 x 3e-14 x
    cond(K~_uu)), the cross build's error times the condition number with the same factor 10, value 1e-9 relative."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2048, 20))
    y = np.sin(x[:, 0]) + 0.3 * x[:, 1] + 0.05 * rng.standard_normal(2048)
    idx = np.sort(rng.choice(2048, size=1930, replace=False))
    net = ([1.2, 1.2], [0.05, 0.05], [("relu",)])
    ref = E.SparseEvidence(x, y, x[idx], E.JITTER, 1024).evaluate64(*MR.variances(net[0], net[1]), net[2], LAM, False, "vfe")
    g_gate = max(1e-8, 10.0 * 3e-14 * ref["cond_kuu"])
    model = make_model(1930, net, 1024).set_inducing(x[idx]).add_rows(x, y).finish()
    assert model.info()["m_padded"] == 2048
    nlml, g = model.evidence_grad(x, y, "vfe")
    e_val, e_grad = abs(nlml - ref["nlml"]) / abs(ref["nlml"]), grad_error(g, ref)
    print("mp = 2048: cond(K~_uu) %.2e, value %.2e relative, gradient %.2e of max(|quad|, |trace|) (gate %.2e)" % (ref["cond_kuu"], e_val,
                                                                                                               e_grad, g_gate))
    assert e_val <= 1e-9 and e_grad <= g_gate
    nlml2, g2 = model.evidence_grad(x, y, "vfe")
    assert nlml2 == nlml and g2.tobytes() == g.tobytes()
    model.close()


# ---- 5. allocations ----

def test_allocation_counts(golden_dir):
    case = E.cases()[0]
    n, m, chunk, bound, absolute, net, _ = case
    x, y, idx, _, _ = E.case_reference(golden_dir, case)
    lib = _lib.load()
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    before = lib.nngp_alloc_count()
    plain = make_model(m, net, chunk, absolute, reserve=False)
    created = lib.nngp_alloc_count() - before
    plain.set_inducing(x[idx]).add_rows(xd, yd).finish()
    plain.predict(x[:50], "diag")
    plain.evidence(bound)
    print("a handle that never reserves: %d allocations at create, %d after fit, predict and evidence" % (created, lib.nngp_alloc_count() - before))
    assert created == 18 and lib.nngp_alloc_count() - before == 18  # what nngp_sparse_create allocated before the evidence existed
    plain.close()
    model = make_model(m, net, chunk, absolute)
    base = lib.nngp_alloc_count()
    for w_std in (1.2, 0.9):
        model.set_kernel(([w_std] * len(net[0]), net[1], net[2]), LAM).set_inducing(x[idx]).add_rows(xd, yd).finish()
        model.evidence(bound)
        model.evidence_grad(xd, yd, bound)
    assert lib.nngp_alloc_count() == base
    model.reserve_evidence()  # repeatable
    assert lib.nngp_alloc_count() == base
    model.close()


# ---- 6. every argument error ----

def test_argument_errors(golden_dir):
    case = E.cases()[0]
    n, m, chunk, bound, absolute, net, _ = case
    x, y, idx, _, _ = E.case_reference(golden_dir, case)
    lib = _lib.load()
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    nlml, grad = ctypes.c_double(), (ctypes.c_double * 5)()

    def egrad(mdl, rows=n, code=1):
        return lib.nngp_sparse_evidence_grad(mdl.handle, _lib.ptr(xd), _lib.ptr(yd), rows, code, ctypes.byref(nlml), grad, _lib.stream_ptr())

    def value(mdl, code=1):
        return lib.nngp_sparse_evidence(mdl.handle, code, ctypes.byref(nlml), _lib.stream_ptr())

    plain = make_model(m, net, chunk, reserve=False).set_inducing(x[idx]).add_rows(xd, yd)
    assert value(plain) == -2 and b"finish" in lib.nngp_last_error()  # before finish
    plain.finish()
    assert value(plain) == 0
    assert egrad(plain) == -2 and b"reserve" in lib.nngp_last_error()  # no reserve
    assert lib.nngp_sparse_evidence_terms(plain.handle, grad, 5) == -2
    plain.reserve_evidence()
    assert egrad(plain, rows=n - 1) == -2 and b"rows were added" in lib.nngp_last_error()  # n mismatch
    assert egrad(plain, code=2) == -2 and value(plain, code=-1) == -2 and b"bound" in lib.nngp_last_error()
    assert egrad(plain) == 0
    assert lib.nngp_sparse_evidence_terms(plain.handle, grad, 5) == -2 and b"count" in lib.nngp_last_error()
    # set_kernel: another number of Dense layers, an Erf layer, a negative parameter -- and the handle keeps its fit
    for bad in (_lib.make_arch_act([1.0] * 3, [0.0] * 3, [("relu",)] * 2), _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("erf", 1.0, 1.0, 0.0)]),
                _lib.make_arch_act([1.0, -1.0], [0.0, 0.0], [("relu",)])):
        assert lib.nngp_sparse_set_kernel(plain.handle, ctypes.byref(bad), LAM, 0) == -2
    assert lib.nngp_sparse_set_kernel(plain.handle, ctypes.byref(_lib.make_arch_act(*net)), -1.0, 0) == -2
    assert value(plain) == 0
    # after set_kernel the handle has no inducing set: the rules of nngp_sparse.h hold
    plain.set_kernel(net, LAM)
    assert lib.nngp_sparse_add_rows(plain.handle, _lib.ptr(xd), _lib.ptr(yd), n, _lib.stream_ptr()) == -2
    assert lib.nngp_sparse_finish(plain.handle, _lib.stream_ptr()) == -2 and value(plain) == -2 and egrad(plain) == -2
    mean = torch.empty((4, 1), dtype=torch.float64, device=dev())
    assert lib.nngp_sparse_predict(plain.handle, _lib.ptr(xd), 4, _lib.COV_NONE, _lib.ptr(mean), None, _lib.stream_ptr()) == -2
    plain.set_inducing(x[idx]).add_rows(xd, yd)
    assert lib.nngp_sparse_predict(plain.handle, _lib.ptr(xd), 4, _lib.COV_NONE, _lib.ptr(mean), None, _lib.stream_ptr()) == -2  # before finish
    plain.close()
    # groups, an Erf layer, two output columns: -2 from the value and the gradient; the Python layer refuses the first before any call
    erf = make_model(m, (net[0], net[1], [("erf", 1.0, 1.0, 0.0)]), chunk, reserve=False).set_inducing(x[idx]).add_rows(xd, yd).finish()
    lib.nngp_sparse_reserve_evidence(erf.handle)
    assert value(erf) == -2 and b"Erf" in lib.nngp_last_error() and egrad(erf) == -2
    erf.close()
    grouped = make_model(m, net, chunk, reserve=False, groups="pairs").set_inducing(x[idx]).add_rows(xd, yd).finish()
    lib.nngp_sparse_reserve_evidence(grouped.handle)
    assert value(grouped) == -2 and b"groups" in lib.nngp_last_error() and egrad(grouped) == -2
    with pytest.raises(ValueError, match="groups"):
        grouped.reserve_evidence()
    grouped.close()
    two = make_model(m, net, chunk, reserve=False, ny=2).set_inducing(x[idx]).add_rows(xd, torch.stack([yd, yd], 1)).finish()
    lib.nngp_sparse_reserve_evidence(two.handle)
    assert value(two) == -2 and b"one output column" in lib.nngp_last_error() and egrad(two) == -2
    two.close()
    with pytest.raises(ValueError, match="input_scale"):
        make_model(m, net, chunk, reserve=False, input_scale=np.ones(20)).reserve_evidence()


# ---- 7. the tuning loop and the command line ----

def test_tune_hyperparameters_matches_the_numpy_driven_run(golden_dir):
    x, y = E.case_rows(golden_dir, "unit", 1000)
    _, _, kf = stax.serial(stax.Dense(512, W_std=1.0, b_std=0.05), stax.Relu(), stax.Dense(1, W_std=1.0, b_std=0.05))
    idx = sparse.select_inducing(x, 128, kf)
    printed = []
    kf_t, lam_t, hist = sparse.tune_hyperparameters(kf, x, y, 128, steps=5, lr=0.05, report=printed.append, inducing=idx, chunk_rows=256)
    kf_o, lam_o, hist_o = sparse.tune_hyperparameters(kf, x, y, 128, steps=5, lr=0.05, report=None,
                                                      evaluator=E.Evaluator(x, y, x[idx], "vfe", chunk_rows=256))
    print("history %s\nnumpy   %s\nrelative difference %s" % (hist, hist_o, np.abs(np.array(hist) / np.array(hist_o) - 1.0)))
    np.testing.assert_allclose(hist, hist_o, rtol=1e-8)
    np.testing.assert_allclose(kf_t.w_std, kf_o.w_std, rtol=1e-8)
    np.testing.assert_allclose(kf_t.b_std, kf_o.b_std, rtol=1e-8)
    assert abs(lam_t - lam_o) <= 1e-8 * lam_o and hist[-1] < hist[0]
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, v) for i, v in enumerate(hist)]
    # without given rows the tuner selects them itself, by the same rule: the same run
    _, _, hist_s = sparse.tune_hyperparameters(kf, x, y, 128, steps=2, lr=0.05, report=None, chunk_rows=256)
    assert hist_s == hist[:2]


def test_train_cli_sparse_tune_on_forest_queries(golden_dir, tmp_path):
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
    args = train_cli.parse_args(["--sparse", "128", "--sparse_tune", "3", "--query_path", str(tmp_path), "--max_num_train", "1000",
                                 "--max_num_test", "200"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    text = buf.getvalue()
    print(text[:1500])
    for i in range(3):
        assert "Step: %d, neg marginal likelihood:" % i in text
    for needle in ("Tuned W_std", "Kernel construction in", "Mean Square Error:", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    assert np.all(np.isfinite(res["pred_mean"])) and res["fit_info"]["m"] == 128 and res["fit_info"]["n"] == 1000
