"""Cost of the matrix-free exact NNGP on the additive kernel (include/nngp_matfree_additive.h) on synthetic encodings: N = 32 768,
three hidden ReLU layers.

operator   one pass of 16 vectors (the RB = 1 form) and of 64 (RB = 4), HIP events around the call after a warm-up, median and
           minimum, for: the plain operator (nngp_kmv_f64) at d = 20 and d = 128; 10 pair groups + the whole input at d = 20;
           64 pair groups + the whole input at d = 128 (nngp_kmv_additive_f64; the stand-alone call also copies the table and
           waits for its stream, microseconds beside these passes).  Beside each the estimate made before any measurement
           (DESIGN.md section 26): 7 ms per group and pass on top of the plain pass.
model      one fit at N = 32 768, m = 1024, d = 20 with 10 pair groups + the whole input: greedy selection, fit (wall clock; the
           call ends in a synchronise), iterations, K passes, true residual.
Nothing is gated.  Prints one JSON line and writes it to profiles/matfree_additive_bench.json (or the path given with --out)."""
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
from nngp_src_amd.matfree_additive import AdditiveMatrixFreeGPModel  # noqa: E402
from nngp_src_amd.sparse import select_inducing  # noqa: E402

N_HIDDEN = 3
W, B = [1.0] * (N_HIDDEN + 1), [0.0] * (N_HIDDEN + 1)
MS_PER_GROUP_ESTIMATE = 7.0  # section 14's 3.5 ms per group over the lower entries, twice for all N^2 entries


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


def operator_case(lib, xd, n, d, n_groups, reps):
    """n_groups = 0: the plain operator; else pair groups (0, 2), (2, 4), ... of weight 1 and the whole input of weight 1."""
    arch = _lib.make_arch_act(W, B, [("relu",)] * N_HIDDEN)
    table = _lib.make_groups(tuple((2 * g, 2 * g + 2) for g in range(n_groups)), (1.0,) * n_groups, 1.0)
    row = {"N": n, "d": d, "hidden_relu_layers": N_HIDDEN, "pair_groups": n_groups, "full_weight": 1.0}
    for r in (16, 64):
        v = torch.randn((r, n), dtype=torch.float64, device="cuda")
        out = torch.empty_like(v)

        def run():
            if n_groups == 0:
                rc = lib.nngp_kmv_f64(_lib.ptr(out), n, _lib.ptr(v), n, r, _lib.ptr(xd), n, d, ctypes.byref(arch), 0.5, _lib.stream_ptr())
            else:
                rc = lib.nngp_kmv_additive_f64(_lib.ptr(out), n, _lib.ptr(v), n, r, _lib.ptr(xd), n, d, ctypes.byref(arch),
                                               ctypes.byref(table), 0.5, _lib.stream_ptr())
            _lib.check(rc, lib)

        ms = events(run, reps)
        row["pass_%d_vectors" % r] = {"ms_median_min": ms, "reps": reps, "ms_per_vector": ms[0] / r}
        del v, out
    torch.cuda.empty_cache()
    return row


def model_case(x, y, n, m, d, n_groups, max_iter):
    groups = [(2 * g, 2 * g + 2) for g in range(n_groups)]
    row = {"N": n, "m": m, "d": d, "pair_groups": n_groups, "full_weight": 1.0, "tol": 1e-10, "max_iter": max_iter}
    _, _, kernel_fn = stax.serial(*([stax.Dense(512), stax.Relu()] * N_HIDDEN + [stax.Dense(1)]))
    kernel_fn = kernel_fn.with_groups(groups)
    row["select_greedy_ms"], idx = wall(lambda: select_inducing(x[:n], m, kernel_fn, method="greedy", candidates=16384))
    model = AdditiveMatrixFreeGPModel(n, d, W, B, m=m, diag_reg=1e-3, tol=1e-10, max_iter=max_iter, rhs_cap=64, chunk_rows=8192,
                                      jitter=1e-8, groups=groups, allow_unconverged=True)
    xd, yd = _lib.to_device_f64(x[:n], torch.device("cuda", 0)), _lib.to_device_f64(y[:n], torch.device("cuda", 0))
    try:
        row["fit_ms"], _ = wall(lambda: model.fit(xd, yd, idx))
        info = model.info()
        row.update(fit_iterations=info["iterations"], fit_k_passes=info["k_passes"], fit_true_residual=info["rel_residual"],
                   fit_converged=info["converged"], fit_restarts=info["restarts"], sigma2=info["sigma2"])
    except _lib.NngpError as e:  # the inducing kernel too close to singular for this jitter: say so
        row["fit_ms"] = "not measured (%s)" % e
    model.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matfree_additive_bench.json"))
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--max_iter", type=int, default=300)
    ap.add_argument("--no_fit", action="store_true")
    args = ap.parse_args()
    t_start = time.perf_counter()
    lib = _lib.load()
    n = args.n
    res = {"device": torch.cuda.get_device_name(0), "hidden_relu_layers": N_HIDDEN, "operator": [], "model": "not measured",
           "estimate_before_measurement": {"ms_per_group_and_pass": MS_PER_GROUP_ESTIMATE, "plain_pass_64_vectors_ms_d128": 17.1,
                                           "pass_10_groups_ms": 87.0, "pass_64_groups_ms": 470.0, "source": "DESIGN.md sections 14, 23"}}
    data = {}
    for d in (20, 128):
        data[d] = synth.synthetic_queries(n, d, seed=0)
    for d, n_groups, reps in ((20, 0, 5), (128, 0, 5), (20, 10, 3), (128, 64, 2)):
        xd = _lib.to_device_f64(data[d][0], torch.device("cuda", 0))
        row = operator_case(lib, xd, n, d, n_groups, reps)
        res["operator"].append(row)
        print("operator d = %d, %d groups: %s" % (d, n_groups, json.dumps(row)), flush=True)
        del xd
    plain = {row["d"]: row for row in res["operator"] if row["pair_groups"] == 0}
    for row in res["operator"]:
        if row["pair_groups"] > 0:
            for r in (16, 64):
                extra = row["pass_%d_vectors" % r]["ms_median_min"][0] - plain[row["d"]]["pass_%d_vectors" % r]["ms_median_min"][0]
                row["pass_%d_vectors" % r]["ms_per_group_above_the_plain_pass"] = extra / row["pair_groups"]
    if not args.no_fit:
        res["model"] = model_case(data[20][0], data[20][1], n, args.m, 20, 10, args.max_iter)
        print("model: %s" % json.dumps(res["model"]), flush=True)
    res["wall_s"] = time.perf_counter() - t_start
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
