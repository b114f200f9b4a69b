"""Timing of the additive kernel's marginal likelihood (include/nngp_additive_mll.h) on one MI355X, beside the plain one of
include/nngp_mll.h in the same process on the same tree: ms per plain NLML + gradient evaluation, per additive NLML-only
evaluation and per additive NLML + gradient + weight-gradient evaluation (HIP-event medians around calls that end in a stream
synchronise), with slot pairs + the whole input as the groups.  With ``--kernel-stats`` (the ``*_kernel_stats.csv`` of a
``rocprofv3 --kernel-trace --stats`` run of this script) it also records the new pass alone (k_mll_add_partial) next to the
plain pass (k_nngp_mll_partial) and the finish kernels.  Prints one JSON line.

    python scripts/additive_mll_bench.py [--cases 10800x20x1,32768x128x3] [--reps 3] [--kernel-stats STATS.csv]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from nngp_mll_bench import _ms, kernel_stats  # noqa: E402
from nngp_src_amd import _lib, additive_mll, mll, synth  # noqa: E402


def run_case(n, d, n_relu, reps):
    x, y = synth.synthetic_queries(n, d, seed=1)
    x = x / 1000.0  # unit range: a dense kernel matrix
    params = ([1.0] * (n_relu + 1), [0.0] * (n_relu + 1), [("relu",)] * n_relu)
    groups = list(_lib.pair_groups(d))
    weights = [1.0] * (1 + len(groups))
    m = additive_mll.AdditiveMarginalLikelihood(n, d, groups).set_train(x, y.reshape(-1))
    plain = lambda with_grad: mll.NNGPMarginalLikelihood.evaluate(m, params, 1e-3, with_grad=with_grad)  # noqa: E731
    plain(True)  # warm-up (code objects, first touch)
    m.evaluate(params, 1e-3, weights=weights)
    t_plain = _ms(lambda: plain(True), reps)
    t_nlml = _ms(lambda: m.evaluate(params, 1e-3, with_grad=False, weights=weights), reps)
    t_grad = _ms(lambda: m.evaluate(params, 1e-3, with_grad=True, weights=weights), reps)
    m.close()
    return {"n": n, "d": d, "n_relu": n_relu, "terms": len(weights), "ms_plain_nlml_grad": round(t_plain, 3),
            "ms_additive_nlml": round(t_nlml, 3), "ms_additive_nlml_grad": round(t_grad, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10800x20x1,32768x128x3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    out = {"metric": "additive_mll_f64", "device": torch.cuda.get_device_name(0), "timing": "HIP-event medians",
           "cases": [run_case(n, d, r, args.reps) for n, d, r in cases]}
    if args.kernel_stats:
        st = kernel_stats(args.kernel_stats)
        pick = lambda key: {k: v for k, v in st.items() if key in k}  # noqa: E731
        out["kernels"] = {"additive_pass": pick("k_mll_add_partial"), "plain_pass": pick("k_nngp_mll_partial"),
                          "additive_finish": pick("k_mll_add_finish"), "term_qsums": pick("k_mll_add_qsums"),
                          "plain_finish": pick("k_mll_finish"), "additive_build": pick("k_build_add")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
