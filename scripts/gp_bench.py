"""Timing of the float64 RBF GP (--kernel_type gp) on one MI355X: ms per (NLML + gradient) evaluation, per NLML-only
evaluation and per diagonal predict, and the float64 Cholesky's rate (n^3 / 3 flops) against the float64 MFMA peak
(78.6 TF/s by spec, not measured here).  Prints one JSON line.

    python scripts/gp_bench.py [--cases 10800x20x3600,32768x128x1024] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nngp_src_amd import _lib, gp, synth  # noqa: E402

F64_MFMA_PEAK_TFS = 78.6


def _ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run_case(n, d, m, reps):
    x, y = synth.synthetic_queries(n, d, seed=1)
    xt, _ = synth.synthetic_queries(m, d, seed=2)
    x, xt = x / 1000.0, xt / 1000.0  # unit range: a dense kernel matrix
    model = gp.RBFGP(n, d, m).set_train(x, y)
    raw = np.array([0.0, -5.0, 0.0])
    model.evaluate(raw)  # warm-up (code objects, first touch)
    model.predict(xt)
    t_eval = _ms(lambda: model.evaluate(raw, True), reps)
    t_nlml = _ms(lambda: model.evaluate(raw, False), reps)
    t_pred = _ms(lambda: model.predict(xt, "diag"), reps)
    # the Cholesky alone, through the stand-alone operator, on the same kernel matrix
    np_ = (n + 127) // 128 * 128
    a = torch.eye(np_, dtype=torch.float64, device=_lib.require_gpu())
    a[:n, :n] = torch.from_numpy(0.7 * gp.kernel(x, None, 0.69)).to(a.device) + 1e-3 * torch.eye(n, dtype=torch.float64, device=a.device)
    lib = _lib.load()
    work = torch.empty_like(a)

    def chol():
        work.copy_(a)
        _lib.check(lib.nngp_potrf_f64(_lib.ptr(work), np_, np_, _lib.stream_ptr()), lib)

    chol()
    copy_ms = _ms(lambda: work.copy_(a), reps)
    t_chol = max(_ms(chol, reps) - copy_ms, 1e-6)
    tfs = (np_ ** 3 / 3.0) / (t_chol * 1e-3) / 1e12
    model.close()
    return {"n": n, "d": d, "m": m, "ms_eval_grad": round(t_eval, 3), "ms_eval_nlml": round(t_nlml, 3),
            "ms_predict_diag": round(t_pred, 3), "ms_potrf_f64": round(t_chol, 3), "potrf_tflops": round(tfs, 2),
            "potrf_frac_of_f64_mfma_peak": round(tfs / F64_MFMA_PEAK_TFS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10800x20x3600,32768x128x1024")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    out = {"metric": "gp_rbf_f64", "device": torch.cuda.get_device_name(0), "f64_mfma_peak_tflops_spec": F64_MFMA_PEAK_TFS,
           "cases": [run_case(n, d, m, args.reps) for n, d, m in cases]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
