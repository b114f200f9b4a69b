"""Timing of the NNGP marginal likelihood (include/nngp_mll.h) on one MI355X: ms per NLML-only evaluation and per NLML + gradient
evaluation (HIP-event medians around calls that end in a stream synchronise), at the reference's run size and at N = 32768.
With ``--kernel-stats`` (the ``*_kernel_stats.csv`` of a ``rocprofv3 --kernel-trace --stats`` run of this script) it also
records the fused gradient pass alone (k_nngp_mll_partial) next to the forward per-layer kernel build of the same shape
(k_build_mfma inside the same evaluations) and the other kernels' totals.  Prints one JSON line.

    python scripts/nngp_mll_bench.py [--cases 10800x20x1,32768x128x3] [--reps 3] [--kernel-stats STATS.csv]
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
from nngp_src_amd import mll, synth  # noqa: E402


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


def run_case(n, d, n_relu, reps):
    x, y = synth.synthetic_queries(n, d, seed=1)
    x = x / 1000.0  # unit range: a dense kernel matrix
    params = ([1.0] * (n_relu + 1), [0.0] * (n_relu + 1), [("relu",)] * n_relu)
    m = mll.NNGPMarginalLikelihood(n, d).set_train(x, y.reshape(-1))
    m.evaluate(params, 1e-3)  # warm-up (code objects, first touch)
    t_grad = _ms(lambda: m.evaluate(params, 1e-3, with_grad=True), reps)
    t_nlml = _ms(lambda: m.evaluate(params, 1e-3, with_grad=False), reps)
    m.close()
    return {"n": n, "d": d, "n_relu": n_relu, "ms_nlml": round(t_nlml, 3), "ms_nlml_grad": round(t_grad, 3)}


def kernel_stats(path):
    """Per-kernel average ms and call count from a rocprofv3 --stats CSV."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            avg = float(row.get("AverageNs") or row.get("Average") or 0.0) * 1e-6
            out[name] = {"calls": int(row.get("Calls") or 0), "avg_ms": round(avg, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10800x20x1,32768x128x3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    out = {"metric": "nngp_mll_f64", "device": torch.cuda.get_device_name(0), "timing": "HIP-event medians",
           "cases": [run_case(n, d, r, args.reps) for n, d, r in cases]}
    if args.kernel_stats:
        st = kernel_stats(args.kernel_stats)
        pick = lambda key: {k: v for k, v in st.items() if key in k}  # noqa: E731
        out["kernels"] = {"fused_pass": pick("k_nngp_mll_partial"), "forward_build": pick("k_build_mfma"),
                          "all": st}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
