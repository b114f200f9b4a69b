"""Cost of the matrix-free exact NNGP (include/nngp_matfree.h) on synthetic encodings: d = 128, three hidden ReLU layers.

operator   nngp_kmv_f64 at N in {32 768, 131 072, 262 144}: one pass of 16 vectors (the RB = 1 form) and of 64 (RB = 4), HIP events
           around the call after a warm-up, median and minimum; achieved flop/s counted from shapes (Gram 2 N^2 d + product 2 N^2 r
           per pass; the layer map is not counted).  Next to it the stand-alone symmetric build (nngp_kernel_build) of the same N
           timed in the same run where the N x N float64 output fits the budget given with --build_max_n (it computes half the tiles).
model      per (N, m): greedy selection, fit (sparse fit of the preconditioner + Vt + alpha by PCG; wall clock, the call ends in a
           synchronise), iterations, K passes, true residual, and a predict with variances of --predict_rows rows (wall clock).
agreement  at N = 32 768: the largest difference of alpha, means and variances against GPModel on the same data.
Stages run in the order above until --budget_s seconds of wall clock are used; what did not run is written as "not measured".
For scale: the exact fit takes 74 ms / 364 ms at N = 32 768 / 65 536 and stops a little above; the
sparse fit of N = 262 144 rows takes 52 ms at m = 1024 and 317 ms at m = 4096, selection apart.
Prints one JSON line and writes it to profiles/matfree_bench.json (or the path given with --out)."""
import argparse
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
from nngp_src_amd.matfree import MatrixFreeGPModel  # noqa: E402
from nngp_src_amd.sparse import select_inducing  # noqa: E402

D, N_HIDDEN = 128, 3
W, B = [1.0] * (N_HIDDEN + 1), [0.0] * (N_HIDDEN + 1)
PEAK_F64_MFMA = 78.6e12
NOT_MEASURED = "not measured"


def events(fn, reps):
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
    return [float(np.median(ts)), float(np.min(ts))]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def operator_case(lib, xd, n, build_max_n):
    arch = _lib.make_arch_act(W, B, [("relu",)] * N_HIDDEN)
    row = {"N": n, "d": D, "hidden_relu_layers": N_HIDDEN}
    reps = 5 if n <= 32768 else (2 if n <= 131072 else 1)
    for r in (16, 64):
        v = torch.randn((r, n), dtype=torch.float64, device="cuda")
        out = torch.empty_like(v)

        def run():
            _lib.check(lib.nngp_kmv_f64(_lib.ptr(out), n, _lib.ptr(v), n, r, _lib.ptr(xd), n, D, ctypes.byref(arch), 0.5, _lib.stream_ptr()), lib)

        ms = events(run, reps)
        flops = 2.0 * n * n * D + 2.0 * n * n * r
        row["pass_%d_vectors" % r] = {"ms_median_min": ms, "reps": reps, "flops_counted": flops, "tflops": flops / (ms[0] * 1e-3) / 1e12,
                                      "share_of_f64_mfma_peak": flops / (ms[0] * 1e-3) / PEAK_F64_MFMA, "ms_per_vector": ms[0] / r}
        del v, out
    if n <= build_max_n:
        k = torch.empty((n, n), dtype=torch.float64, device="cuda")
        a1 = _lib.make_arch(W, B)

        def build():
            _lib.check(lib.nngp_kernel_build(_lib.ptr(xd), n, None, n, D, ctypes.byref(a1), _lib.DTYPE_F64, _lib.ptr(k), None, n, 0, n,
                                             _lib.stream_ptr()), lib)

        ms = events(build, reps)
        row["symmetric_build"] = {"ms_median_min": ms, "note": "half the tiles, the composite ReLU map, K written to memory"}
        del k
    else:
        row["symmetric_build"] = NOT_MEASURED + " (the N x N output is above --build_max_n)"
    torch.cuda.empty_cache()
    return row


def model_case(kernel_fn, x, y, xt, n, m, max_iter, predict_rows, rhs_cap):
    row = {"N": n, "m": m, "tol": 1e-10, "max_iter": max_iter, "rhs_cap": rhs_cap}
    xs, ys = x[:n], y[:n]
    row["select_greedy_ms"], idx = wall(lambda: select_inducing(xs, m, kernel_fn, method="greedy", candidates=16384))
    jitter = 1e-8
    model = MatrixFreeGPModel(n, D, W, B, m=m, diag_reg=1e-3, tol=1e-10, max_iter=max_iter, rhs_cap=rhs_cap, chunk_rows=8192,
                              jitter=jitter, allow_unconverged=True)
    xd, yd = _lib.to_device_f64(xs, torch.device("cuda", 0)), _lib.to_device_f64(ys, torch.device("cuda", 0))
    try:
        row["fit_ms"], _ = wall(lambda: model.fit(xd, yd, idx))
    except _lib.NngpError as e:  # the inducing kernel too close to singular for this jitter: say so and stop this case
        row["fit_ms"] = NOT_MEASURED + " (%s)" % e
        model.close()
        return row, None
    info = model.info()
    row.update(jitter=jitter, fit_iterations=info["iterations"], fit_k_passes=info["k_passes"], fit_true_residual=info["rel_residual"],
               fit_converged=info["converged"], fit_restarts=info["restarts"], sigma2=info["sigma2"])
    if predict_rows > 0:
        td = _lib.to_device_f64(xt[:predict_rows], torch.device("cuda", 0))
        ms, _ = wall(lambda: model.predict(td, "diag", as_numpy=False))
        info = model.info()
        row["predict"] = {"rows": predict_rows, "ms": ms, "iterations": info["iterations"], "k_passes": info["k_passes"],
                          "true_residual": info["rel_residual"], "converged": info["converged"]}
    else:
        row["predict"] = NOT_MEASURED
    return row, model


def agreement(model, x, y, xt, n, rows):
    """The matrix-free model against GPModel on the same data (the exact model's float32-factor + CG pipeline)."""
    from nngp_src_amd.model import GPModel
    exact = GPModel(n, D, W, B, diag_reg=1e-3)
    exact.fit(x[:n], y[:n])
    mean_e, var_e = exact.predict(xt[:rows], cov="diag")
    alpha_e = exact.alpha()
    alpha_e = alpha_e.cpu().numpy() if hasattr(alpha_e, "cpu") else np.asarray(alpha_e)
    exact.close()
    mean, var = model.predict(xt[:rows], "diag")
    out = {"N": n, "rows": rows,
           "mean_max_difference_over_max_mean": float(np.abs(mean.ravel() - np.asarray(mean_e).ravel()).max() / np.abs(mean_e).max()),
           "variance_max_relative_difference": float(np.max(np.abs(var.ravel() / np.asarray(var_e).ravel() - 1.0)))}
    out["alpha_max_difference_over_max_alpha"] = float(np.abs(model.alpha().ravel() - alpha_e.ravel()).max() / np.abs(alpha_e).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matfree_bench.json"))
    ap.add_argument("--sizes", default="32768,131072,262144")
    ap.add_argument("--model", default="32768:1024,131072:1024,262144:1024,32768:4096,131072:4096,262144:4096", help="N:m cases, in order")
    ap.add_argument("--budget_s", type=float, default=3000.0)
    ap.add_argument("--build_max_n", type=int, default=32768)
    ap.add_argument("--max_iter", type=int, default=400)
    ap.add_argument("--predict_rows", type=int, default=1024)
    ap.add_argument("--predict_rows_large", type=int, default=64, help="rows predicted with variances above N = 32 768")
    args = ap.parse_args()
    t_start = time.perf_counter()
    left = lambda: args.budget_s - (time.perf_counter() - t_start)  # noqa: E731
    lib = _lib.load()
    sizes = [int(v) for v in args.sizes.split(",") if v]
    cases = [tuple(int(v) for v in c.split(":")) for c in args.model.split(",") if c]
    n_max = max(sizes + [n for n, _ in cases])
    x, y = synth.synthetic_queries(n_max, D, seed=0)
    xt, _ = synth.synthetic_queries(1024, D, seed=1)
    _, _, kernel_fn = stax.serial(*([stax.Dense(512), stax.Relu()] * N_HIDDEN + [stax.Dense(1)]))
    res = {"device": torch.cuda.get_device_name(0), "d": D, "hidden_relu_layers": N_HIDDEN, "operator": [], "model": [],
           "agreement": NOT_MEASURED,
           "for_scale": {"exact_fit_ms": {"32768": 74, "65536": 364}, "sparse_fit_ms_at_262144": {"1024": 52, "4096": 317},
                         "source": "DESIGN.md section 16"}}
    xd_all = _lib.to_device_f64(x, torch.device("cuda", 0))
    for n in sizes:
        if left() <= 0:
            res["operator"].append({"N": n, "result": NOT_MEASURED + " (time budget)"})
            continue
        res["operator"].append(operator_case(lib, xd_all[:n].contiguous(), n, args.build_max_n))
        print("operator N = %d: %s" % (n, json.dumps(res["operator"][-1])), flush=True)
    del xd_all
    torch.cuda.empty_cache()
    for n, m in cases:
        if left() <= 0:
            res["model"].append({"N": n, "m": m, "result": NOT_MEASURED + " (time budget)"})
            continue
        rows = args.predict_rows if n <= 32768 else args.predict_rows_large
        row, model = model_case(kernel_fn, x, y, xt, n, m, args.max_iter, rows, 64)
        res["model"].append(row)
        print("model N = %d m = %d: %s" % (n, m, json.dumps(row)), flush=True)
        if model is not None and n == 32768 and res["agreement"] == NOT_MEASURED and left() > 0:
            res["agreement"] = agreement(model, x, y, xt, n, min(rows, 256))
            print("agreement: %s" % json.dumps(res["agreement"]), flush=True)
        if model is not None:
            model.close()
        torch.cuda.empty_cache()
    res["wall_s"] = time.perf_counter() - t_start
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
