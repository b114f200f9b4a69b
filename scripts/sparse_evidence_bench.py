"""Cost of one value-and-gradient evaluation of the sparse NNGP evidence (include/nngp_sparse_evidence.h) on synthetic encodings:
d = 128, three hidden ReLU layers, N in {65 536, 262 144} training rows, m in {1024, 4096} random inducing rows, chunks of 8192 rows,
bound vfe.

Per (N, m), HIP-event medians unless marked:
    fit_ms            set_kernel + set_inducing + add_rows (device-resident X, one call) + finish: the pass every evaluation starts with
    value_ms          nngp_sparse_evidence (no pass over the data)
    grad_ms           nngp_sparse_evidence_grad, everything
Per m, the pieces of one chunk of 8192 rows, timed alone on the chunk's shape:
    build_ms          nngp_kernel_build_act of K(X_c, U) into a [c, mp] buffer
    gemm_ms           nngp_gemm_nt_f64, D_c = K_cu M'  (c x mp x mp), and its TF/s
    adjoint_ms        the rectangular adjoint pass alone (nngp_sparse_adjoint_rect, wall clock: it allocates its partials and
                      synchronises), and the entries of K_cu it sweeps per second
    once_ms_derived   grad_ms minus chunks * (grad_ms(262 144) - grad_ms(65 536)) / 24: what does not grow with N -- the two
                      triangular solves of the identity, the m^3 products, the symmetric pass over K_uu
    per_chunk_ms_derived   that slope
Next to it, the exact evidence: nngp_mll_evaluate with its gradient at the largest N of {65 536, 32 768, 16 384} that fits.
Prints one JSON line and writes it to profiles/sparse_evidence_bench.json (or the path given as the argument)."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nngp_src_amd import _lib, mll, synth  # noqa: E402
from nngp_src_amd.kernel_spec import KernelSpec  # noqa: E402
from nngp_src_amd.sparse import SparseGPModel  # noqa: E402

D, N_HIDDEN, CHUNK = 128, 3, 8192
NS = [65536, 262144]
MS = [1024, 4096]
W, B = [1.0] * (N_HIDDEN + 1), [0.05] * (N_HIDDEN + 1)
ACTS = [("relu",)] * N_HIDDEN
LAM, BOUND = 1e-3, "vfe"


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


def chunk_pieces(lib, xs, u, m):
    mp = -(-m // 128) * 128
    spec = KernelSpec(W, B, ACTS)
    xc = xs[:CHUNK].contiguous()
    k = torch.zeros((CHUNK, mp), dtype=torch.float64, device="cuda")
    mm = torch.randn((mp, mp), dtype=torch.float64, device="cuda")
    dm = torch.empty((CHUNK, mp), dtype=torch.float64, device="cuda")
    beta = torch.randn(CHUNK, dtype=torch.float64, device="cuda")
    gamma = torch.randn(m, dtype=torch.float64, device="cuda")
    out = (ctypes.c_double * (4 * len(W)))()
    arch = spec.arch_act()

    def build():
        _lib.check(spec.kernel_build(lib, _lib.ptr(xc), CHUNK, _lib.ptr(u), m, D, _lib.GET_NNGP, _lib.ptr(k), None, mp, 0, CHUNK,
                                     _lib.stream_ptr()), lib)

    def gemm():
        _lib.check(lib.nngp_gemm_nt_f64(_lib.ptr(dm), mp, None, 0, _lib.ptr(k), mp, _lib.ptr(mm), mp, CHUNK, mp, mp, 1.0, 0.0,
                                        _lib.stream_ptr()), lib)

    def adjoint():
        _lib.check(lib.nngp_sparse_adjoint_rect(_lib.ptr(xc), CHUNK, _lib.ptr(u), m, D, ctypes.byref(arch), _lib.ptr(dm), mp,
                                                _lib.ptr(beta), _lib.ptr(gamma), out, _lib.stream_ptr()), lib)

    row = {}
    row["build_ms"], _ = timed(build, 5)
    row["gemm_ms"], _ = timed(gemm, 5)
    row["gemm_tflops"] = 2.0 * CHUNK * mp * mp / (row["gemm_ms"] * 1e-3) / 1e12
    row["adjoint_ms"], row["adjoint_min_ms"] = wall(adjoint, 5)
    row["adjoint_gentries_per_s"] = CHUNK * m / (row["adjoint_ms"] * 1e-3) / 1e9
    return row


def exact_evidence(x, y):
    for n in (65536, 32768, 16384):
        handle = None
        try:
            handle = mll.NNGPMarginalLikelihood(n, D).set_train(x[:n], y[:n])
            ms, lo = wall(lambda: handle.evaluate((W, B, ACTS), LAM), 2)
            return {"n": n, "evaluate_ms": ms, "evaluate_min_ms": lo}
        except _lib.NngpError as e:
            print("exact evidence at N = %d: %s" % (n, e), file=sys.stderr)
        finally:
            if handle is not None:
                handle.close()
    return None


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_evidence_bench.json")
    lib = _lib.load()
    x, y = synth.synthetic_queries(max(NS), D, seed=0)
    xs = torch.from_numpy(np.ascontiguousarray(x / 1000.0)).to("cuda")
    ys = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64).reshape(-1)).to("cuda")
    result = {"d": D, "n_dense": len(W), "chunk_rows": CHUNK, "bound": BOUND, "device": torch.cuda.get_device_name(0), "cases": [],
              "chunk": {}}
    grad_ms = {}
    for m in MS:
        idx = np.sort(np.random.RandomState(10).choice(NS[0], size=m, replace=False))
        u = xs[torch.from_numpy(idx).to("cuda")].contiguous()
        result["chunk"][str(m)] = chunk_pieces(lib, xs, u, m)
        model = SparseGPModel(m, D, W, B, activations=ACTS, diag_reg=LAM, chunk_rows=CHUNK, jitter=1e-6, test_cap=128).reserve_evidence()
        for n in NS:
            xn, yn = xs[:n], ys[:n]

            def fit():
                model.set_kernel((W, B, ACTS), LAM).set_inducing(u).add_rows(xn, yn).finish()

            row = {"n": n, "m": m, "chunks": -(-n // CHUNK)}
            row["fit_ms"], row["fit_min_ms"] = wall(fit, 3)
            row["value_ms"], _ = timed(lambda: model.evidence(BOUND), 5)
            row["grad_ms"], row["grad_min_ms"] = timed(lambda: model.evidence_grad(xn, yn, BOUND), 3)
            row["nlml"], g = model.evidence_grad(xn, yn, BOUND)
            row["grad"] = [float(v) for v in g]
            grad_ms[(n, m)] = row["grad_ms"]
            result["cases"].append(row)
            print(json.dumps(row), file=sys.stderr)
        model.close()
        slope = (grad_ms[(NS[1], m)] - grad_ms[(NS[0], m)]) / ((NS[1] - NS[0]) // CHUNK)
        result["chunk"][str(m)]["per_chunk_ms_derived"] = slope
        result["chunk"][str(m)]["once_ms_derived"] = grad_ms[(NS[0], m)] - slope * (NS[0] // CHUNK)
    del xs, ys
    torch.cuda.empty_cache()
    result["exact"] = exact_evidence(x / 1000.0, np.asarray(y, dtype=np.float64).reshape(-1))
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
