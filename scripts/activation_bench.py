"""Cost of the activations: the kernel build (NNGP only, symmetric, float64) at N = 32768, d = 128, 3 hidden layers for ReLU with
the composite map, ReLU per layer (knob 5 = 63), LeakyRelu(0.1), Abs and Erf; and one fit + predict (M = 1024, diagonal
variance) per activation.  Writes profiles/activation_bench.json (or the path given as the argument)."""
import ctypes
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

N, D, HIDDEN, M = 32768, 128, 3, 1024
ACTS = {"relu": ("relu",), "leaky_relu": ("abrelu", 0.1, 1.0), "abs": ("abrelu", -1.0, 1.0), "erf": ("erf", 1.0, 1.0, 0.0)}


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    x, y = synth.synthetic_queries(N + M, D, seed=0)
    xd = torch.from_numpy(x[:N]).cuda()
    xt = torch.from_numpy(x[N:]).cuda()
    yd = torch.from_numpy(y[:N]).cuda()
    out = torch.empty((N, N), dtype=torch.float64, device="cuda")
    w, b = [1.0] * (HIDDEN + 1), [0.0] * (HIDDEN + 1)
    res = {"N": N, "d": D, "hidden_layers": HIDDEN, "M": M, "device": torch.cuda.get_device_name(0), "build_ms": {}, "fit_predict_ms": {}}

    klib = _lib.load(knobs=True)  # the same sources with the timing knobs (knob 5 = 63: the per-layer ReLU recursion)
    arch = _lib.make_arch(w, b)

    def relu_build():
        _lib.check(klib.nngp_kernel_build(_lib.ptr(xd), N, None, N, D, ctypes.byref(arch), _lib.DTYPE_F64, _lib.ptr(out), None, N,
                                          0, N, _lib.stream_ptr()), klib)
    res["build_ms"]["relu_composite"] = timed(relu_build)
    _lib.check(klib.nngp_debug_set(5, 63), klib)
    res["build_ms"]["relu_per_layer"] = timed(relu_build)
    _lib.check(klib.nngp_debug_set(5, 0), klib)

    lib = _lib.load()
    for name in ("leaky_relu", "abs", "erf"):
        aa = _lib.make_arch_act(w, b, [ACTS[name]] * HIDDEN)

        def build(aa=aa):
            _lib.check(lib.nngp_kernel_build_act(_lib.ptr(xd), N, None, N, D, ctypes.byref(aa), _lib.DTYPE_F64, _lib.ptr(out), None,
                                                 N, 0, N, _lib.stream_ptr()))
        res["build_ms"][name] = timed(build)
    del out
    torch.cuda.empty_cache()

    for name in ("relu", "leaky_relu", "abs", "erf"):
        model = GPModel(N, D, w, b, get="nngp", diag_reg=1e-3, m_cap=M, activations=[ACTS[name]] * HIDDEN)

        def step():
            model.fit(xd, yd)
            model.predict(xt, cov="diag", as_numpy=False)
        res["fit_predict_ms"][name] = timed(step, reps=3)
        res.setdefault("refine_iters", {})[name] = model.info()["refine_iters"]
        model.close()
        torch.cuda.empty_cache()

    print(json.dumps(res, indent=1))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "activation_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
