"""Cost and effect of per-feature input relevances (include/nngp_ard.h) on one MI355X.

Per case N x d x hidden layers: HIP-event medians of one NLML + gradient evaluation through nngp_mll_evaluate (what the parent
of this feature runs) and through nngp_mll_evaluate_ard with grad_s, on one handle in one session, and their ratio.  With
``--kernel-stats`` (the ``*_kernel_stats.csv`` of a ``rocprofv3 --kernel-trace --stats`` run of this script) the two new passes
alone: the adjoint pass with ARD set (k_nngp_ard_partial) next to the plain one (k_nngp_mll_partial), and the contraction
(k_ard_contract).  ``--qerror N``: held-out q-error on synth.synthetic_queries before tuning, after tuning without relevances and
after tuning with them (same steps).  Prints one JSON line.

    python scripts/nngp_ard_bench.py [--cases 10800x20x1,32768x128x3] [--reps 3] [--kernel-stats STATS.csv] [--qerror 4000]
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
from nngp_src_amd import mll, predict, stax, synth  # noqa: E402


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
    s = np.exp(np.random.default_rng(0).normal(size=d))
    m = mll.NNGPMarginalLikelihood(n, d, ard=True).set_train(x, y.reshape(-1))
    m.evaluate(params, 1e-3)  # warm-up (code objects, first touch)
    m.evaluate(params, 1e-3, relevance=s)
    t_plain = _ms(lambda: m.evaluate(params, 1e-3), reps)
    t_ard = _ms(lambda: m.evaluate(params, 1e-3, relevance=s), reps)
    m.close()
    return {"n": n, "d": d, "n_relu": n_relu, "ms_nlml_grad": round(t_plain, 3), "ms_nlml_grad_and_grad_s": round(t_ard, 3),
            "ratio": round(t_ard / t_plain, 4)}


def qerror(n_train, n_test, d, steps):
    x, y = synth.synthetic_queries(n_train + n_test, d, seed=3, join_block=True)
    x, y = x / 1000.0, y.reshape(-1)
    xtr, ytr, xte, yte = x[:n_train], y[:n_train], x[n_train:], y[n_train:]
    _, _, kf = stax.serial(stax.Dense(512), stax.Relu(), stax.Dense(1))

    def profile(kernel_fn, lam):
        mean = predict.gradient_descent_mse_ensemble(kernel_fn, xtr, ytr, diag_reg=lam)(x_test=xte, get="nngp")
        q = np.exp2(np.abs(np.ravel(mean) - yte))  # y is log2 of the cardinality
        return {"mean": round(float(np.mean(q)), 4), "median": round(float(np.median(q)), 4),
                "p95": round(float(np.percentile(q, 95)), 4), "mse_log2": round(float(np.mean((np.ravel(mean) - yte) ** 2)), 5)}

    out = {"n_train": n_train, "n_test": n_test, "d": d, "steps": steps, "untuned": profile(kf, 1e-3)}
    kf_t, lam_t, hist = mll.tune_hyperparameters(kf, xtr, ytr, steps=steps, report=None, b_std_init=0.05)
    out["tuned"] = dict(profile(kf_t, lam_t), nlml=round(hist[-1], 3))
    kf_a, lam_a, hist_a = mll.tune_hyperparameters(kf, xtr, ytr, steps=steps, report=None, b_std_init=0.05, ard=True)
    out["tuned_ard"] = dict(profile(kf_a, lam_a), nlml=round(hist_a[-1], 3),
                            relevances=[round(float(v), 5) for v in kf_a.input_scale ** 2])
    return out


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
    ap.add_argument("--qerror", type=int, default=0, help="training rows of the q-error study (0: skip)")
    ap.add_argument("--qerror-steps", type=int, default=50)
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")] if args.cases else []
    out = {"metric": "nngp_ard_f64", "device": torch.cuda.get_device_name(0), "timing": "HIP-event medians",
           "cases": [run_case(n, d, r, args.reps) for n, d, r in cases]}
    if args.qerror:
        out["qerror"] = qerror(args.qerror, args.qerror // 4, 20, args.qerror_steps)
    if args.kernel_stats:
        st = kernel_stats(args.kernel_stats)
        pick = lambda key: {k: v for k, v in st.items() if key in k}  # noqa: E731
        out["kernels"] = {"adjoint_pass_ard": pick("k_nngp_ard_partial"), "adjoint_pass": pick("k_nngp_mll_partial"),
                          "contraction": pick("k_ard_contract"), "finish": pick("k_ard_finish"), "scale": pick("k_ard_scale")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
