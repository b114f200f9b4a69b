"""Timing of leave-one-out cross-validation (include/nngp_loo.h) on one MI355X: ms per value-only LOO evaluation, per LOO
evaluation with gradient and, as the yardstick, per nngp_mll_evaluate with gradient -- the same process, handle and data --
at the reference's run size and at N = 32768 (HIP-event medians around calls that end in a stream synchronise).  With
``--kernel-stats`` (what a ``rocprofv3 --kernel-trace --stats`` run of this script wrote: its ``*_kernel_stats.csv``, or the
``*_results.db`` that newer releases write by default) it also records
the kernels' totals: the fused pass (k_nngp_loo_partial) next to the marginal likelihood's (k_nngp_mll_partial), the scaled
copy, the point kernel.  ``--square-c`` (library with timing knobs, NNGP_KNOBS=1) forms C as one square product instead of
row panels up to the diagonal, for the A/B of DESIGN.md section 12.  Prints one JSON line.

    python scripts/nngp_loo_bench.py [--cases 10800x20x1,32768x128x3] [--reps 3] [--objective nlpd] [--kernel-stats STATS.csv]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nngp_src_amd import _lib, loo, mll, synth  # noqa: E402


def _ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def run_case(n, d, n_relu, reps, objective):
    x, y = synth.synthetic_queries(n, d, seed=1)
    x = x / 1000.0  # unit range: a dense kernel matrix
    params = ([1.0] * (n_relu + 1), [0.0] * (n_relu + 1), [("relu",)] * n_relu)
    lo = loo.LeaveOneOut(n, d, objective).set_train(x, y.reshape(-1))
    ml = mll.NNGPMarginalLikelihood.__new__(mll.NNGPMarginalLikelihood)  # the marginal likelihood on the same device handle
    ml.__dict__.update(lo.__dict__)
    lo.evaluate(params, 1e-3)  # warm-up (code objects, first touch)
    ml.evaluate(params, 1e-3)
    t_value = _ms(lambda: lo.evaluate(params, 1e-3, with_grad=False), reps)
    t_grad = _ms(lambda: lo.evaluate(params, 1e-3, with_grad=True), reps)
    t_mll = _ms(lambda: ml.evaluate(params, 1e-3, with_grad=True), reps)
    t_mll_value = _ms(lambda: ml.evaluate(params, 1e-3, with_grad=False), reps)
    ml._h = None  # one owner
    lo.close()
    return {"n": n, "d": d, "n_relu": n_relu, "objective": objective, "ms_loo_value": round(t_value, 3),
            "ms_loo_grad": round(t_grad, 3), "ms_mll_grad": round(t_mll, 3), "ms_mll_value": round(t_mll_value, 3),
            "loo_grad_over_mll_grad": round(t_grad / t_mll, 3), "loo_value_over_mll_grad": round(t_value / t_mll, 3)}


def kernel_stats(path):
    """Per-kernel total / average ms and call count from a rocprofv3 --stats CSV or results database (view top_kernels, us)."""
    out = {}
    if path.endswith(".db"):
        import sqlite3
        for name, calls, tot, avg, pct in sqlite3.connect(path).execute(
                "select name, total_calls, total_duration, average, percentage from top_kernels"):
            out[name] = {"calls": int(calls), "avg_ms": round(avg * 1e-3, 4), "total_ms": round(tot * 1e-3, 3), "percent": float(pct)}
        return out
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            avg = float(row.get("AverageNs") or row.get("Average") or 0.0) * 1e-6
            tot = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0.0) * 1e-6
            out[name] = {"calls": int(row.get("Calls") or 0), "avg_ms": round(avg, 4), "total_ms": round(tot, 3),
                         "percent": float(row.get("Percentage") or 0.0)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10800x20x1,32768x128x3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--objective", default="nlpd", choices=sorted(loo.OBJECTIVES))
    ap.add_argument("--square-c", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.square_c:
        _lib.check(_lib.load(knobs=True).nngp_debug_set(15, 1))
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    out = {"metric": "nngp_loo_f64", "device": torch.cuda.get_device_name(0), "timing": "HIP-event medians",
           "c_product": "square" if args.square_c else "lower row panels",
           "cases": [run_case(n, d, r, args.reps, args.objective) for n, d, r in cases]}
    if args.kernel_stats:
        st = kernel_stats(args.kernel_stats)
        pick = lambda key: {k: v for k, v in st.items() if key in k}  # noqa: E731
        out["kernels"] = {"fused_pass_loo": pick("k_nngp_loo_partial"), "fused_pass_mll": pick("k_nngp_mll_partial"),
                          "scaled_copy": pick("k_loo_scale_cols"), "point": pick("k_loo_point"), "finish": pick("k_loo_finish"),
                          "all": st}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
