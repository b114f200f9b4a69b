"""Per-feature relevances on the sparse NNGP evidence on the MI355X (include/nngp_sparse_ard.h, csrc/sparse_ard.hip) against the
NumPy float64 reference (sparse_ard_reference.py: forward-mode input tangents, dense assembly, 80-bit referee).

Gate.  Value: 1e-9 relative.  Each component of grad and grad_s: g * max(|quad|, |trace|) of that component, with
g = max(1e-8, 10 x the reference's own float64-vs-80-bit distance on the case), computed here and printed; on every case the
reference's distance is below 1e-9 (test_sparse_ard_host.py asserts it on the CPU), so g = 1e-8 throughout.  Every test prints what
it measured before it asserts.
"""
import ast
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import nngp_ard_reference as AR
import nngp_mll_reference as MR
import sparse_ard_reference as A
import sparse_evidence_reference as E
import sparse_reference as S
import test_sparse_ard_host as H
from nngp_src_amd import _lib, mll, sparse
from nngp_src_amd import train as train_cli
from nngp_src_amd.sparse import SparseGPModel

pytestmark = pytest.mark.gpu

LAM = A.LAM


def dev():
    return torch.device("cuda", 0)


def make_model(m_cap, net, chunk_rows, absolute=False, jitter=E.JITTER, reserve="ard", d=20, **kw):
    w, b, acts = net
    model = SparseGPModel(m_cap, d, w, b, activations=acts, diag_reg=LAM, chunk_rows=chunk_rows, jitter=jitter, test_cap=128,
                          diag_reg_absolute_scale=absolute, **kw)
    return model.reserve_evidence_ard() if reserve == "ard" else (model.reserve_evidence() if reserve else model)


def fit(model, x, y, idx, rel="keep"):
    if not isinstance(rel, str):
        model.set_relevance(rel)
    return model.set_inducing(x[idx]).add_rows(x, y).finish()


def gate_of(dist):
    return max(1e-8, 10.0 * max(dist[1], dist[2]))


def scaled_error(got, want, quad, trace):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(quad), np.abs(trace))))


# ---- 1. the rectangular pass with its contraction alone ----

RECT_NETS = [([1.2, 0.9], [0.05, 0.0], [("relu",)]),
             ([1.2, 0.9, 1.1, 1.0], [0.0, 0.1, 0.02, 0.05], [("relu",), ("abrelu", 0.1, 1.0), ("relu",)]),
             # 5 and 9 Dense layers: the NLC = 8 and NLC = 16 instantiations of the pass
             ([1.2, 0.9, 1.1, 1.0, 1.3], [0.0, 0.1, 0.02, 0.05, 0.0], [("relu",), ("abrelu", 0.1, 1.0)] * 2),
             ([1.2, 1.1] * 4 + [1.0], [0.0, 0.05, 0.0] * 3, [("relu",)] * 7 + [("abrelu", 0.1, 1.0)])]


@pytest.mark.parametrize("c,m,d", [(65, 63, 33), (130, 128, 20)])
@pytest.mark.parametrize("net", RECT_NETS)
def test_rectangular_relevance_pass_alone(c, m, d, net):
    """A random dense seed (NaN beyond its m logical columns) and a random rank-one seed against the reference's contraction of the
    forward-mode input tangents.  Bound per feature and half:
        (1e-12 + c m 2^-53) sum_ij |seed_ij| (|c_ij x_ik u_jk| + |e1_ij| x_ik^2 + |e2_ij| u_jk^2) / d
    -- 1e-12 is what test_rectangular_adjoint_pass_alone derives for the pass, c m 2^-53 the worst-case rounding of summing c m
    terms in any order.  d = 33: feature 32 is alone in the second feature chunk.  One relevance is exactly 0."""
    rng = np.random.default_rng(c + m)
    x, u = rng.standard_normal((c, d)), rng.standard_normal((m, d))
    u[3] = x[7]  # a training row that is also an inducing row takes the general formula
    x[11] = 0.0  # q = 0 with b_0 = 0 in the second network
    rel = A.relevances(d)
    beta, gamma, seed = rng.standard_normal(c), rng.standard_normal(m), rng.standard_normal((c, m))
    ld = m + 5
    sd = torch.full((c, ld), float("nan"), dtype=torch.float64, device=dev())
    sd[:, :m] = torch.from_numpy(seed).to(dev())
    w, b, acts = net
    lib = _lib.load()
    arch = _lib.make_arch_act(w, b, acts)
    xd, ud, bd, gd = (torch.from_numpy(a).to(dev()) for a in (x, u, beta, gamma))
    sh = (ctypes.c_double * d)(*rel)

    def run():
        out = (ctypes.c_double * (2 * d))()
        _lib.check(lib.nngp_sparse_ard_rect(_lib.ptr(xd), c, _lib.ptr(ud), m, d, ctypes.byref(arch), sh, _lib.ptr(sd), ld, _lib.ptr(bd),
                                            _lib.ptr(gd), out, _lib.stream_ptr()), lib)
        return np.array(out[:])

    got = run()
    v, cc = MR.variances(w, b)
    _, cm, e1, e2 = A.input_tangents(x, u, rel, v, cc, acts)
    factor = 1e-12 + c * m * 2.0 ** -53
    worst, worst_zero = 0.0, 0.0
    for half, s in ((0, np.outer(beta, gamma)), (1, seed)):
        want = A.contract_rect(s, x, u, cm, e1, e2)
        mass = A.contract_rect(np.abs(s), np.abs(x), np.abs(u), np.abs(cm), np.abs(e1), np.abs(e2))
        ratio = np.abs(got[half * d:(half + 1) * d] - want) / (factor * mass)
        worst, worst_zero = max(worst, float(ratio.max())), max(worst_zero, float(ratio[rel == 0.0].max()))
    print("relevance pass c %d m %d d %d, %d Dense: worst error %.2e of its bound (the feature with s_k = 0: %.2e; last feature: %.2e)"
          % (c, m, d, len(w), worst, worst_zero, float(ratio[d - 1])))
    assert np.all(np.isfinite(got)) and worst <= 1.0
    assert run().tobytes() == got.tobytes()
    assert torch.isnan(sd[:, m:]).all() and np.array_equal(sd[:, :m].cpu().numpy(), seed)  # the caller's seed is not written


# ---- 2. value and gradient against the reference ----

@pytest.mark.parametrize("case", A.cases(), ids=A.case_id)
def test_value_and_gradients_against_the_reference(golden_dir, case):
    n, m, chunk, bound, absolute, net, _ = case
    x, y, rel, idx, ref, dist = A.case_reference(golden_dir, case)
    g_gate = gate_of(dist)
    print("%s: cond(K~_uu) %.2e; reference vs 80-bit: value %.2e, gradient %.2e, relevance gradient %.2e; gate g = %.1e"
          % (A.case_id(case), ref["cond_kuu"], dist[0], dist[1], dist[2], g_gate))
    assert ref["cond_kuu"] <= E.COND_CAP
    model = fit(make_model(m, net, chunk, absolute), x, y, idx, rel)
    info = model.info()
    assert (info["n"], info["m"], info["m_padded"], info["chunks"]) == (n, m, -(-m // 128) * 128, -(-n // chunk))
    value = model.evidence(bound)
    nlml, g, gs = model.evidence_grad(x, y, bound, ard=True)
    t, ts = model.evidence_terms(), model.evidence_ard_terms()
    e_val = abs(nlml - ref["nlml"]) / abs(ref["nlml"])
    e_grad, e_s = scaled_error(g, ref["grad"], ref["quad"], ref["trace"]), scaled_error(gs, ref["grad_s"], ref["quad_s"], ref["trace_s"])
    e_ff = float(np.max(np.abs(ts["tr_dkff"] - ref["tr_dkff_s"]) / ref["tr_dkff_s"]))
    e_uu = float(np.max(np.abs(ts["tr_dkuu"] - ref["tr_dkuu_s"]) / ref["tr_dkuu_s"]))
    print("device vs reference: value %.2e relative, gradient %.2e, relevance gradient %.2e of max(|quad|, |trace|); "
          "tr dK_ff/ds %.2e, tr dK_uu/ds %.2e relative" % (e_val, e_grad, e_s, e_ff, e_uu))
    print("  grad_s    %s\n  reference %s" % (gs, ref["grad_s"]))
    assert e_val <= 1e-9
    assert e_grad <= g_gate and e_s <= g_gate
    assert e_ff <= 1e-12 and e_uu <= 1e-12
    assert value == nlml
    assert np.array_equal(-0.5 * t["quad"] + 0.5 * t["trace"], g) and np.array_equal(-0.5 * ts["quad"] + 0.5 * ts["trace"], gs)
    nlml2, g2, gs2 = model.evidence_grad(x, y, bound, ard=True)  # two identical evaluations: the same bits
    assert nlml2 == nlml and g2.tobytes() == g.tobytes() and gs2.tobytes() == gs.tobytes()
    model.close()


# ---- 3. bits ----

def test_bits_against_the_plain_evidence(golden_dir):
    case = A.cases()[0]
    n, m, chunk, bound, absolute, net, _ = case
    x, y, rel, idx, _, _ = A.case_reference(golden_dir, case, with_longdouble=False)
    plain = fit(make_model(m, net, chunk, absolute, reserve="plain"), x, y, idx)
    nlml_p, g_p = plain.evidence_grad(x, y, bound)
    mean_p, var_p = plain.predict(x[:50], "diag")
    plain.close()
    model = fit(make_model(m, net, chunk, absolute), x, y, idx, np.ones(20))
    nlml_1, g_1, gs_1 = model.evidence_grad(x, y, bound, ard=True)
    mean_1, var_1 = model.predict(x[:50], "diag")
    assert nlml_1 == nlml_p and g_1.tobytes() == g_p.tobytes() and np.all(np.isfinite(gs_1))  # s = 1: a handle that never saw one
    assert mean_1.tobytes() == mean_p.tobytes() and var_1.tobytes() == var_p.tobytes()
    fit(model, x, y, idx, rel)
    nlml_s, g_s, _ = model.evidence_grad(x, y, bound, ard=True)
    nlml_q, g_q = model.evidence_grad(x, y, bound)  # the plain gradient on the same handle, at the same relevances
    assert nlml_s == nlml_q and g_s.tobytes() == g_q.tobytes() and nlml_s != nlml_p
    # the same rows scaled by the caller, on a handle without relevances: the same bits
    xs = x * np.sqrt(rel)
    other = make_model(m, net, chunk, absolute, reserve="plain").set_inducing(xs[idx]).add_rows(xs, y).finish()
    nlml_o, g_o = other.evidence_grad(xs, y, bound)
    other.close()
    assert nlml_o == nlml_s and g_o.tobytes() == g_s.tobytes()
    fit(model, x, y, idx, None)  # set_relevance(NULL): the plain bytes again
    nlml_n, g_n = model.evidence_grad(x, y, bound)
    assert nlml_n == nlml_p and g_n.tobytes() == g_p.tobytes()
    model.close()


# ---- 4. chunking ----

def test_chunks_of_128_against_one_chunk(golden_dir):
    case = [c for c in A.cases() if c[:3] == (1000, 200, 256)][2]  # vfe, relative, 2 Dense
    n, m, _, bound, absolute, net, _ = case
    x, y, rel, idx, ref, dist = A.case_reference(golden_dir, case)
    out = []
    for chunk in (128, 1024):
        model = fit(make_model(m, net, chunk, absolute), x, y, idx, rel)
        out.append(model.evidence_grad(x, y, bound, ard=True))
        model.close()
    e_val = abs(out[0][0] - out[1][0]) / abs(out[1][0])
    e_s = scaled_error(out[0][2], out[1][2], ref["quad_s"], ref["trace_s"])
    print("chunks of 128 vs one chunk: value %.2e, relevance gradient %.2e of max(|quad|, |trace|) (gate %.1e)" % (e_val, e_s, gate_of(dist)))
    assert e_val <= 1e-12 and e_s <= gate_of(dist)


# ---- 5. the exact limit on the device ----

@pytest.mark.parametrize("net", E.EXACT_NETS)
def test_exact_limit_against_the_exact_evidence_on_the_device(golden_dir, net):
    """U = X = the first 256 forest rows, jitter 0, against NNGPMarginalLikelihood(ard=True).evaluate(relevance=s) on the same rows.
    cond(K) is large here, so the gate is what test_sparse_ard_host.py measures for this limit -- the references' distance to
    their 80-bit reruns -- times 10, with the floors of the gate above (1e-9 for the value, 1e-8 for the gradients)."""
    g = np.load(os.path.join(golden_dir, "forest_n256_m64.npz"))
    x, y = g["X_train"][:256], g["Y_train"][:256].reshape(-1)
    rel = A.relevances(20)
    res, _, _ = H.exact_limit_s(x, y, net, rel, False, LAM)
    exact = mll.NNGPMarginalLikelihood(256, 20, ard=True).set_train(x, y)
    nlml_e, g_e, gs_e = exact.evaluate(net, LAM, False, relevance=rel)
    te = exact.terms()
    scale = np.maximum(np.abs(te["quad"]), np.abs(te["trace"]))
    exact.close()
    model = fit(make_model(256, net, 128, jitter=0.0), x, y, np.arange(256), rel)
    for bound in E.BOUNDS:
        ref = res[bound][0]
        b_val, b_grad, b_s = max(1e-9, res[bound][1][0]), max(1e-8, res[bound][1][1]), max(1e-8, res[bound][1][2])
        nlml, grad, gs = model.evidence_grad(x, y, bound, ard=True)
        e_val, e_grad = abs(nlml - nlml_e) / abs(nlml_e), float(np.max(np.abs(grad - g_e) / scale))
        e_s = scaled_error(gs, gs_e, ref["quad_s"], ref["trace_s"])
        print("exact limit %s, %d Dense: value %.2e (gate %.2e), gradient %.2e (gate %.2e), relevance gradient %.2e (gate %.2e) of "
              "max(|quad|, |trace|)" % (bound, len(net[0]), e_val, b_val, e_grad, b_grad, e_s, b_s))
        assert e_val <= b_val and e_grad <= b_grad and e_s <= b_s
    model.close()


# ---- 6. predict under a relevance ----

def test_predict_under_a_relevance(golden_dir):
    case = A.cases()[0]  # n = 300, m = 70, chunks of 128
    n, m, chunk, bound, absolute, net, _ = case
    x, y, rel, idx, _, _ = A.case_reference(golden_dir, case, with_longdouble=False)
    xt = E.case_rows(golden_dir, "unit", 500)[0][300:]
    v, c = MR.variances(net[0], net[1])
    kernel, diag = E.kernels(v, c, net[2])
    xs, xts = AR.scaled(x, rel), AR.scaled(xt, rel)
    ref = S.SparseReference(kernel, diag, LAM, E.JITTER, absolute).fit(xs, y, xs[idx], chunk)
    ref_mean, ref_var = ref.predict(xts, "diag")
    _, ref_cov = ref.predict(xts, "full")
    kdiag = diag(xts)
    model = fit(make_model(m, net, chunk, absolute), x, y, idx, rel)
    mean, var = model.predict(xt, "diag")
    mean_f, cov = model.predict(xt, "full")
    e_mean = float(np.abs(mean - ref_mean).max() / np.abs(ref_mean).max())
    e_var = float(np.max(np.abs(var - ref_var) / kdiag))
    e_cov = float(np.max(np.abs(cov - ref_cov) / np.sqrt(np.outer(kdiag, kdiag))))
    print("predict under relevances: mean %.2e of max |mean|, variance %.2e K(x,x), full covariance %.2e sqrt(K_ii K_jj)" % (e_mean, e_var, e_cov))
    assert e_mean <= 1e-8 and e_var <= 1e-8 and e_cov <= 1e-8  # TOL of test_gpu_sparse.py
    np.testing.assert_allclose(mean_f, mean, rtol=0, atol=1e-12 * np.abs(mean).max())
    model.close()


# ---- 7. allocations ----

def test_allocation_counts(golden_dir):
    case = A.cases()[0]
    n, m, chunk, bound, absolute, net, _ = case
    x, y, rel, idx, _, _ = A.case_reference(golden_dir, case, with_longdouble=False)
    lib = _lib.load()
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    before = lib.nngp_alloc_count()
    plain = make_model(m, net, chunk, absolute, reserve=False)
    created = lib.nngp_alloc_count() - before
    plain.set_inducing(x[idx]).add_rows(xd, yd).finish()
    plain.predict(x[:50], "diag")
    plain.evidence(bound)
    after = lib.nngp_alloc_count() - before
    plain.reserve_evidence()
    reserved = lib.nngp_alloc_count()
    plain.evidence_grad(xd, yd, bound)
    print("a handle that never reserves relevances: %d allocations at create, %d after fit, predict and evidence" % (created, after))
    assert created == 18 and after == 18 and lib.nngp_alloc_count() == reserved
    plain.close()
    model = make_model(m, net, chunk, absolute)
    base = lib.nngp_alloc_count()
    for s in (rel, np.ones(20)):
        model.set_relevance(s).set_inducing(x[idx]).add_rows(xd, yd).finish()
        model.evidence_grad(xd, yd, bound, ard=True)
        model.predict(x[:50], "diag")
    assert lib.nngp_alloc_count() == base
    model.reserve_evidence_ard()  # repeatable
    assert lib.nngp_alloc_count() == base
    model.close()


# ---- 8. every argument error ----

def test_argument_errors(golden_dir):
    case = A.cases()[0]
    n, m, chunk, bound, absolute, net, _ = case
    x, y, rel, idx, _, _ = A.case_reference(golden_dir, case, with_longdouble=False)
    lib = _lib.load()
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    nlml, grad, gs = ctypes.c_double(), (ctypes.c_double * 5)(), (ctypes.c_double * 20)()
    pd = ctypes.POINTER(ctypes.c_double)

    def egrad(mdl, rows=n, code=1):
        return lib.nngp_sparse_evidence_grad_ard(mdl.handle, _lib.ptr(xd), _lib.ptr(yd), rows, code, ctypes.byref(nlml), grad, gs,
                                                 _lib.stream_ptr())

    def set_rel(mdl, s):
        return lib.nngp_sparse_set_relevance(mdl.handle, np.ascontiguousarray(s, dtype=np.float64).ctypes.data_as(pd))

    mdl = make_model(m, net, chunk, reserve=False)
    assert lib.nngp_sparse_reserve_ard(mdl.handle) == -2 and b"reserve_evidence" in lib.nngp_last_error()
    mdl.reserve_evidence()
    assert set_rel(mdl, rel) == -2 and b"reserve_ard" in lib.nngp_last_error()
    assert lib.nngp_sparse_set_relevance(mdl.handle, None) == 0  # nothing to take away
    mdl.set_inducing(x[idx]).add_rows(xd, yd).finish()
    assert lib.nngp_sparse_reserve_ard(mdl.handle) == 0
    assert egrad(mdl) == -2 and b"set_relevance" in lib.nngp_last_error()  # finished, but no relevances
    assert lib.nngp_sparse_ard_terms(mdl.handle, gs, 80) == -2
    for bad in (-1.0, float("nan"), float("inf")):
        s = rel.copy()
        s[5] = bad
        assert set_rel(mdl, s) == -2 and b"relevance 5" in lib.nngp_last_error()
    assert mdl.evidence(bound) == mdl.evidence(bound)  # a refused set_relevance leaves the fit alone
    assert set_rel(mdl, rel) == 0
    assert egrad(mdl) == -2 and b"finish" in lib.nngp_last_error()  # set_relevance dropped the fit
    mdl.set_inducing(x[idx]).add_rows(xd, yd)
    assert egrad(mdl) == -2 and b"finish" in lib.nngp_last_error()
    mdl.finish()
    assert egrad(mdl, rows=n - 1) == -2 and b"rows were added" in lib.nngp_last_error()
    assert egrad(mdl, code=2) == -2 and b"bound" in lib.nngp_last_error()
    assert egrad(mdl) == 0
    assert lib.nngp_sparse_ard_terms(mdl.handle, gs, 79) == -2 and b"count" in lib.nngp_last_error()
    assert lib.nngp_sparse_ard_terms(mdl.handle, (ctypes.c_double * 80)(), 80) == 0
    mdl.close()
    # an Erf layer, groups, two output columns
    erf = make_model(m, (net[0], net[1], [("erf", 1.0, 1.0, 0.0)]), chunk, reserve=False)
    assert lib.nngp_sparse_reserve_evidence(erf.handle) == 0 and lib.nngp_sparse_reserve_ard(erf.handle) == 0 and set_rel(erf, rel) == 0
    erf.set_inducing(x[idx]).add_rows(xd, yd).finish()
    assert egrad(erf) == -2 and b"Erf" in lib.nngp_last_error()
    erf.close()
    grouped = make_model(m, net, chunk, reserve=False, groups="pairs")
    assert lib.nngp_sparse_reserve_evidence(grouped.handle) == 0 and lib.nngp_sparse_reserve_ard(grouped.handle) == 0 and set_rel(grouped, rel) == 0
    grouped.set_inducing(x[idx]).add_rows(xd, yd).finish()
    assert egrad(grouped) == -2 and b"groups" in lib.nngp_last_error()
    with pytest.raises(ValueError, match="groups"):
        grouped.reserve_evidence_ard()
    grouped.close()
    two = make_model(m, net, chunk, reserve=False, ny=2)
    assert lib.nngp_sparse_reserve_evidence(two.handle) == 0 and lib.nngp_sparse_reserve_ard(two.handle) == 0 and set_rel(two, rel) == 0
    two.set_inducing(x[idx]).add_rows(xd, torch.stack([yd, yd], 1)).finish()
    assert egrad(two) == -2 and b"one output column" in lib.nngp_last_error()
    two.close()
    scaled = make_model(m, net, chunk, reserve=False, input_scale=np.ones(20))
    with pytest.raises(ValueError, match="input_scale"):
        scaled.set_relevance(rel)
    with pytest.raises(ValueError, match="input_scale"):
        scaled.reserve_evidence_ard()
    scaled.close()
    short = make_model(m, net, chunk)
    with pytest.raises(ValueError, match="one value per feature"):
        short.set_relevance(np.ones(19))
    short.close()


# ---- 9. the tuning loop and the command line ----

def test_tune_hyperparameters_matches_the_numpy_driven_run(golden_dir):
    x, y = E.case_rows(golden_dir, "unit", 1000)
    idx, _ = S.greedy_inducing(E.kernels(*MR.variances([1.0, 1.0], [0.05, 0.05]), [("relu",)])[0], x, 128)
    kf, (kf_o, lam_o, hist_o) = H.tuning_run(x, y, idx, 5, chunk_rows=256)
    printed = []
    kf_t, lam_t, hist = sparse.tune_hyperparameters(kf, x, y, 128, steps=5, lr=0.05, report=printed.append, inducing=idx, chunk_rows=256,
                                                    ard=True)
    s_t, s_o = kf_t.input_scale ** 2, kf_o.input_scale ** 2
    print("history %s\nnumpy   %s\nrelative difference %s\nrelevances: relative difference %s"
          % (hist, hist_o, np.abs(np.array(hist) / np.array(hist_o) - 1.0), np.abs(s_t / s_o - 1.0)))
    np.testing.assert_allclose(hist, hist_o, rtol=1e-8)
    np.testing.assert_allclose(s_t, s_o, rtol=1e-6)
    np.testing.assert_allclose(kf_t.w_std, kf_o.w_std, rtol=1e-6)
    np.testing.assert_allclose(kf_t.b_std, kf_o.b_std, rtol=1e-6)
    assert abs(lam_t - lam_o) <= 1e-6 * lam_o and hist[-1] < hist[0] and abs(np.mean(np.log(s_t))) <= 1e-12
    assert printed == ["Step: %d, neg marginal likelihood: %f" % (i, v) for i, v in enumerate(hist)]


def test_train_cli_sparse_tune_ard_on_forest_queries(golden_dir, tmp_path):
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
    args = train_cli.parse_args(["--sparse", "128", "--sparse_tune", "3", "--sparse_tune_ard", "--ard_groups", "pairs", "--query_path",
                                 str(tmp_path), "--max_num_train", "1000", "--max_num_test", "200"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = train_cli.main(args)
    text = buf.getvalue()
    print(text[:2500])
    for i in range(3):
        assert "Step: %d, neg marginal likelihood:" % i in text
    for needle in ("Tuned W_std", "Tuned relevances=[", "Kernel construction in", "Mean Square Error:", "Predict Result Profile of 200 Queries:"):
        assert needle in text, needle
    line = [ln for ln in text.splitlines() if ln.startswith("Tuned relevances=")][0]
    s = np.array(ast.literal_eval(line[len("Tuned relevances="):]))
    assert s.shape == (20,) and np.all(s > 0.0) and np.allclose(s[0::2], s[1::2], rtol=1e-12) and np.ptp(s) > 0.0
    assert np.all(np.isfinite(res["pred_mean"])) and res["fit_info"]["m"] == 128 and res["fit_info"]["n"] == 1000
