"""Cost of the additive kernel over feature groups (include/nngp_additive.h): the symmetric train-train build of a model
(nngp_model_build_rows: float64 K plus the float32 factor input) and one fit + predict (M = 1024, diagonal variance), grouped
(slot pairs + the whole input) against ungrouped, in the same process, at
    N = 32768, d = 128, 3 hidden ReLU layers   and   N = 10800, d = 20, 1 hidden ReLU layer (the forest run's size).
HIP-event medians.  The cost model to compare with is G + 1 evaluations of the layer map per entry against 1, plus one
read-modify-write of K.  Writes profiles/additive_bench.json (or the path given as the argument)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nngp_src_amd import synth  # noqa: E402
from nngp_src_amd.model import GPModel  # noqa: E402

M = 1024
SIZES = [(32768, 128, 3), (10800, 20, 1)]


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


def main():
    res = {"M": M, "device": torch.cuda.get_device_name(0), "sizes": []}
    for n, d, hidden in SIZES:
        x, y = synth.synthetic_queries(n + M, d, seed=0)
        xd, xt, yd = torch.from_numpy(x[:n]).cuda(), torch.from_numpy(x[n:]).cuda(), torch.from_numpy(y[:n]).cuda()
        w, b = [1.0] * (hidden + 1), [0.0] * (hidden + 1)
        row = {"N": n, "d": d, "hidden_layers": hidden, "groups": d // 2, "build_ms": {}, "fit_predict_ms": {}}
        for name, kw in (("ungrouped", {}), ("pairs_plus_full", dict(groups="pairs", full_weight=1.0))):
            model = GPModel(n, d, w, b, get="nngp", diag_reg=1e-3, m_cap=M, **kw)
            model.set_train(xd, yd)
            row["build_ms"][name] = timed(lambda: model.build_rows(0, n), reps=5)

            def step():
                model.fit(xd, yd)
                model.predict(xt, cov="diag", as_numpy=False)
            row["fit_predict_ms"][name] = timed(step, reps=3)
            row.setdefault("refine_iters", {})[name] = model.info()["refine_iters"]
            model.close()
            torch.cuda.empty_cache()
        g = row["groups"]
        row["build_ratio"] = row["build_ms"]["pairs_plus_full"][0] / row["build_ms"]["ungrouped"][0]
        row["step_ratio"] = row["fit_predict_ms"]["pairs_plus_full"][0] / row["fit_predict_ms"]["ungrouped"][0]
        row["model_ratio_maps"] = g + 1  # layer-map evaluations per entry, grouped / ungrouped
        res["sizes"].append(row)
    print(json.dumps(res, indent=1))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "additive_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
