"""Cost of the sparse (inducing-point, DTC) NNGP (include/nngp_sparse.h) on synthetic encodings: d = 128, three hidden ReLU layers,
N in {65 536, 262 144} training rows, m in {1024, 4096} inducing rows chosen greedily from 16 384 candidates, chunks of 8192 rows.

Per (N, m):
    select_greedy_ms  select_inducing(method="greedy"), wall clock (it ends with a read-back of the indices)
    fit_ms            set_inducing + add_rows over all N rows (device-resident X, one call) + finish, wall clock
    set_inducing_ms, finish_ms   wall clock (both end in a synchronise for the pivot status)
    chunk             one chunk of 8192 rows, HIP-event medians: add_rows_ms (everything), build_ms (nngp_kernel_build_act of K(X_c, U) into
                      a [c, mp] buffer), syrk_ms (nngp_syrk_tn_f64 on the chunk's shape), trsm_ms_derived = add_rows - build - syrk (it also
                      carries the chunk's zeroing, row norms, diagonal and trace)
    stages            the same chunk on the handle's own path, timed directly: a second handle on the timing-knob build, where
                      add_rows can leave stages out (key 15 = 16 + mask: 1 cross build, 2 solve, 4 Gram kernel).  HIP-event medians of
                      add_rows with everything (all_ms), with none of the three (rest_ms: zeroing, row norms, diagonal, trace) and
                      with one stage each (build_ms, trsm_ms, syrk_ms, each still carrying rest_ms); trsm_tflops = c mp^2 flops over
                      trsm_ms - rest_ms.  The solve then works on a zeroed buffer: its GEMMs do not depend on the data.
    syrk_tflops       executed flops of the lower tiles, tiles * 2 * 128^2 * c, over syrk_ms, and its share of the 78.6 TF/s float64
                      MFMA peak (spec; DESIGN.md section 9 uses the same figure)
    predict_1024_ms   predict of 1024 rows with variances, HIP events
Per m, one A/B at c = 8192 rows: k_syrk_tn_f64 against an explicit transposed copy of the chunk (torch) followed by nngp_gemm_nt_f64,
the full mp x mp product -- alternating, in one loop; gemm_alone_ms leaves the transpose out.
Prints one JSON line and writes it to profiles/sparse_bench.json (or the path given as the argument)."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nngp_src_amd import _lib, stax, synth  # noqa: E402
from nngp_src_amd.sparse import SparseGPModel, select_inducing  # noqa: E402

D, N_HIDDEN, CHUNK, TEST = 128, 3, 8192, 1024
NS = [65536, 262144]
MS = [1024, 4096]
PEAK_F64_MFMA = 78.6e12
W, B = [1.0] * (N_HIDDEN + 1), [0.0] * (N_HIDDEN + 1)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return float(np.median(ts)), float(np.min(ts))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def syrk(lib, c, r, a, y, rows, mp, beta):
    _lib.check(lib.nngp_syrk_tn_f64(_lib.ptr(c), c.stride(0), _lib.ptr(r), _lib.ptr(a), a.stride(0), _lib.ptr(y), rows, mp, 1, beta,
                                    _lib.stream_ptr()), lib)


def gemm_nt(lib, c, a, b):
    m, k = a.shape
    _lib.check(lib.nngp_gemm_nt_f64(_lib.ptr(c), c.stride(0), None, 0, _lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0), m, b.shape[0], k,
                                    1.0, 0.0, _lib.stream_ptr()), lib)


def ab_case(lib, mp, rows=CHUNK, reps=7):
    """k_syrk_tn_f64 against transpose + full NT product, alternating."""
    a = torch.randn((rows, mp), dtype=torch.float64, device="cuda")
    y = torch.randn((rows, 1), dtype=torch.float64, device="cuda")
    c1 = torch.zeros((mp, mp), dtype=torch.float64, device="cuda")
    c2 = torch.zeros_like(c1)
    r = torch.zeros((mp, 1), dtype=torch.float64, device="cuda")
    at = a.t().contiguous()

    def run_syrk():
        syrk(lib, c1, r, a, y, rows, mp, 0.0)

    def run_gemm():
        t = a.t().contiguous()
        gemm_nt(lib, c2, t, t)

    def run_gemm_alone():
        gemm_nt(lib, c2, at, at)

    ts = {"syrk": [], "transpose_gemm": [], "gemm_alone": []}
    for fn in (run_syrk, run_gemm, run_gemm_alone):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in (("syrk", run_syrk), ("transpose_gemm", run_gemm), ("gemm_alone", run_gemm_alone)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts[name].append(t0.elapsed_time(t1))
    lower = torch.tril(torch.ones((mp // 128, mp // 128), device="cuda")).repeat_interleave(128, 0).repeat_interleave(128, 1).bool()
    diff = float(((c1 - c2).abs() * lower).max() / c2.abs().max())
    tiles = (mp // 128) * (mp // 128 + 1) // 2
    flops = tiles * 2.0 * 128 * 128 * rows
    out = {"mp": mp, "rows": rows, "max_rel_difference_lower_tiles": diff, "syrk_flops": flops, "gemm_flops": 2.0 * mp * mp * rows}
    for name, v in ts.items():
        out[name + "_ms"] = [float(np.median(v)), float(np.min(v))]
    out["syrk_tflops"] = flops / (out["syrk_ms"][0] * 1e-3) / 1e12
    out["syrk_share_of_f64_mfma_peak"] = out["syrk_tflops"] * 1e12 / PEAK_F64_MFMA
    out["gemm_alone_tflops"] = out["gemm_flops"] / (out["gemm_alone_ms"][0] * 1e-3) / 1e12
    out["syrk_wins"] = bool(out["syrk_ms"][0] < out["transpose_gemm_ms"][0])
    return out


def model_case(lib, kernel_fn, x, y, xt, n, m):
    row = {"N": n, "m": m}
    xs = x[:n]
    row["select_greedy_ms"], idx = wall(lambda: select_inducing(xs, m, kernel_fn, method="greedy", candidates=16384))
    xd, yd, td = (_lib.to_device_f64(a, torch.device("cuda", 0)) for a in (xs, y[:n], xt))
    jitter = 1e-8
    model = SparseGPModel(m, D, W, B, diag_reg=1e-3, chunk_rows=CHUNK, jitter=jitter, test_cap=TEST)
    try:
        model.set_inducing(xs[idx])
    except _lib.NngpError:  # the inducing kernel too close to singular for this jitter: say so and go on
        model.close()
        jitter = 1e-6
        model = SparseGPModel(m, D, W, B, diag_reg=1e-3, chunk_rows=CHUNK, jitter=jitter, test_cap=TEST)
    row["jitter"] = jitter
    ud = xd[torch.from_numpy(idx).cuda()].contiguous()
    row["set_inducing_ms"], _ = wall(lambda: model.set_inducing(ud))
    mp = model.info()["m_padded"]

    def fit():
        model.set_inducing(ud)
        _lib.check(lib.nngp_sparse_add_rows(model.handle, _lib.ptr(xd), _lib.ptr(yd), n, _lib.stream_ptr()), lib)
        model.finish()

    fit()
    row["fit_ms"] = min(wall(fit)[0] for _ in range(2))
    row["finish_ms"] = float(np.median([wall(model.finish)[0] for _ in range(5)]))
    row["sigma2"] = model.info()["sigma2"]
    # one chunk, by stage
    xc, yc = xd[:CHUNK], yd[:CHUNK]
    chunk = {}
    chunk["add_rows_ms"] = timed(lambda: _lib.check(lib.nngp_sparse_add_rows(model.handle, _lib.ptr(xc), _lib.ptr(yc), CHUNK, _lib.stream_ptr()), lib), 7)
    arch = _lib.make_arch_act(W, B, [("relu",)] * N_HIDDEN)
    kbuf = torch.zeros((CHUNK, mp), dtype=torch.float64, device="cuda")
    chunk["build_ms"] = timed(lambda: _lib.check(lib.nngp_kernel_build_act(_lib.ptr(xc), CHUNK, _lib.ptr(ud), m, D, ctypes.byref(arch), _lib.DTYPE_F64,
                                                                          _lib.ptr(kbuf), None, mp, 0, CHUNK, _lib.stream_ptr()), lib), 7)
    cbuf = torch.zeros((mp, mp), dtype=torch.float64, device="cuda")
    rbuf = torch.zeros((mp, 1), dtype=torch.float64, device="cuda")
    chunk["syrk_ms"] = timed(lambda: syrk(lib, cbuf, rbuf, kbuf, yc, CHUNK, mp, 1.0), 7)
    chunk["trsm_ms_derived"] = chunk["add_rows_ms"][0] - chunk["build_ms"][0] - chunk["syrk_ms"][0]
    tiles = (mp // 128) * (mp // 128 + 1) // 2
    chunk["syrk_tflops"] = tiles * 2.0 * 128 * 128 * CHUNK / (chunk["syrk_ms"][0] * 1e-3) / 1e12
    chunk["syrk_share_of_f64_mfma_peak"] = chunk["syrk_tflops"] * 1e12 / PEAK_F64_MFMA
    chunk["trsm_tflops_derived"] = float(CHUNK) * mp * mp / (max(chunk["trsm_ms_derived"], 1e-6) * 1e-3) / 1e12
    row["chunk"] = chunk
    # the stages on the handle's own path, one at a time
    klib = _lib.load(knobs=True)
    kmodel = SparseGPModel(m, D, W, B, diag_reg=1e-3, chunk_rows=CHUNK, jitter=jitter, test_cap=TEST, knobs=True)
    kmodel.set_inducing(ud)

    def stage(skip):
        klib.nngp_debug_set(15, 16 + skip)
        try:
            return timed(lambda: _lib.check(klib.nngp_sparse_add_rows(kmodel.handle, _lib.ptr(xc), _lib.ptr(yc), CHUNK, _lib.stream_ptr()), klib), 7)
        finally:
            klib.nngp_debug_set(15, 0)

    stages = {"all_ms": stage(0), "rest_ms": stage(7), "build_ms": stage(2 | 4), "trsm_ms": stage(1 | 4), "syrk_ms": stage(1 | 2)}
    stages["trsm_tflops"] = float(CHUNK) * mp * mp / (max(stages["trsm_ms"][0] - stages["rest_ms"][0], 1e-6) * 1e-3) / 1e12
    row["stages"] = stages
    kmodel.close()
    model.finish()
    row["predict_1024_ms"] = timed(lambda: model.predict(td, "diag", as_numpy=False), 7)
    mean, var = model.predict(td, "diag")
    row["predict_finite"] = bool(np.all(np.isfinite(mean)) and np.all(var > 0))
    model.close()
    del xd, yd, td, kbuf, cbuf
    torch.cuda.empty_cache()
    return row


def main():
    lib = _lib.load()
    _, _, kernel_fn = stax.serial(*([stax.Dense(512)] + [l for _ in range(N_HIDDEN) for l in (stax.Relu(), stax.Dense(512))]))
    res = {"d": D, "hidden_layers": N_HIDDEN, "chunk_rows": CHUNK, "device": torch.cuda.get_device_name(0),
           "f64_mfma_peak_tflops_spec": PEAK_F64_MFMA / 1e12, "ab": [], "cases": []}
    for mp in MS:
        res["ab"].append(ab_case(lib, mp))
    x, y = synth.synthetic_queries(max(NS) + TEST, D, seed=0)
    xt = x[max(NS):]
    for n in NS:
        for m in MS:
            res["cases"].append(model_case(lib, kernel_fn, x, y, xt, n, m))
            print(json.dumps(res["cases"][-1]), flush=True)
    print(json.dumps(res))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_bench.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
