"""Cost and gain of the greedy pool selection by conditional variance (include/nngp_pool.h) on synthetic encodings: a model fitted on
N = 4096 rows (d = 20, one hidden ReLU layer), pools of m = 4096 and m = 10800 rows, count = 1000 picks.  Per pool size:
    predict_full_ms   GPModel.predict(cov="full"), the covariance the operator reads
    greedy_ms         nngp_pool_select_greedy alone on that covariance (count launches, library workspace)
    select_score_ms   today's GPModel.select_pool (marginal score, top-k), predict(cov="diag") included
    select_greedy_ms  GPModel.select_pool(method="greedy"), predict(cov="full") and the read-back of the indices included
    remaining_variance  sum of the pool's posterior variances once the picks are labelled (noise = the fit's reg), for the greedy
                        picks and for the `count` largest marginal variances, from the device's covariance in NumPy float64
HIP-event medians (the select_* figures: wall clock around a call that ends with a read-back).  Prints one JSON line and writes it to
profiles/pool_greedy_bench.json (or the path given as the argument)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nngp_src_amd import _lib, synth  # noqa: E402
from nngp_src_amd.model import GPModel  # noqa: E402
from nngp_src_amd.pool import greedy_on_device  # noqa: E402

N, D, COUNT = 4096, 20, 1000
POOLS = [4096, 10800]


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


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts))


def remaining_variance(cov, picks, noise):
    a = cov[np.ix_(picks, picks)] + noise * np.eye(picks.size)
    return float(np.trace(cov) - np.sum(cov[picks, :] * np.linalg.solve(a, cov[picks, :])))


def main():
    lib = _lib.load()
    res = {"N": N, "d": D, "count": COUNT, "device": torch.cuda.get_device_name(0), "pools": []}
    x, y = synth.synthetic_queries(N + max(POOLS), D, seed=0)
    model = GPModel(N, D, [1.0, 1.0], [0.0, 0.0], get="nngp", diag_reg=1e-3).fit(x[:N], y[:N])
    noise = float(model.info()["reg"])
    for m in POOLS:
        xp = torch.from_numpy(x[N:N + m]).cuda()
        row = {"m": m, "noise": noise}
        row["predict_full_ms"] = timed(lambda: model.predict(xp, cov="full", as_numpy=False), reps=3)
        _, cov = model.predict(xp, cov="full", as_numpy=False)
        row["greedy_ms"] = timed(lambda: greedy_on_device(lib, cov, COUNT, noise, want_gains=True), reps=5)
        row["select_score_ms"] = wall(lambda: model.select_pool(xp, COUNT), reps=3)
        row["select_greedy_ms"] = wall(lambda: model.select_pool(xp, COUNT, method="greedy"), reps=3)
        picks = model.select_pool(xp, COUNT, method="greedy")
        again = greedy_on_device(lib, cov, COUNT, noise)[0].cpu().numpy()
        host = cov.cpu().numpy()
        host = 0.5 * (host + host.T)
        top = np.argsort(np.diag(host), kind="stable")[::-1][:COUNT]
        row["distinct_picks"] = int(np.unique(picks).size)
        row["same_picks_from_a_second_covariance"] = bool(np.array_equal(picks, again))
        row["picks_shared_with_top_k"] = int(np.intersect1d(picks, top).size)
        row["remaining_variance"] = {"before": float(np.trace(host)), "greedy": remaining_variance(host, picks, noise),
                                     "top_k": remaining_variance(host, top, noise)}
        row["factor_row_bytes_read"] = float(COUNT) * (COUNT - 1) / 2 * m * 8
        res["pools"].append(row)
        del cov, host
        torch.cuda.empty_cache()
    model.close()
    print(json.dumps(res))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pool_greedy_bench.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
