"""Cost of the relevance gradient of the sparse NNGP evidence (include/nngp_sparse_ard.h) on synthetic encodings: three hidden ReLU
layers, N = 65 536 training rows in chunks of 8192, bound vfe, at (m, d) in {(1024, 128), (4096, 128), (1024, 20)} with random
inducing rows and log-normal relevances.

Per (N, m, d), HIP-event medians unless marked:
    grad_ms           nngp_sparse_evidence_grad on the handle with relevances (it scales the rows, nothing more)
    grad_ard_ms       nngp_sparse_evidence_grad_ard on the same handle, and ard_over_grad = their ratio
    plain_grad_ms     nngp_sparse_evidence_grad on a handle that never reserved relevances, at the same sizes: the figure
                      scripts/sparse_evidence_bench.py records as grad_ms, for comparison across commits
Per (m, d), the pieces of one chunk of 8192 rows, timed alone on the chunk's shape (wall clock: both allocate their buffers on the
stream and synchronise):
    adjoint_ms        the rectangular adjoint pass alone (nngp_sparse_adjoint_rect)
    ard_rect_ms       the pass with ARD set plus the contraction (nngp_sparse_ard_rect: it also scales both row sets and copies the seed)
    contraction_share_derived   (ard_rect_ms - adjoint_ms) / ard_rect_ms: what the contraction and the extra stores add to the pass
    pass_share_of_grad_ard, extra_share_of_grad_ard   chunks * adjoint_ms and chunks * (ard_rect_ms - adjoint_ms) over grad_ard_ms
Prints one JSON line and writes it to profiles/sparse_ard_bench.json (or the path given as the argument)."""
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
from nngp_src_amd.kernel_spec import KernelSpec  # noqa: E402
from nngp_src_amd.sparse import SparseGPModel  # noqa: E402

N, N_HIDDEN, CHUNK = 65536, 3, 8192
SHAPES = [(1024, 128), (4096, 128), (1024, 20)]  # m, d
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


def chunk_pieces(lib, xs, u, m, d, rel):
    mp = -(-m // 128) * 128
    arch = KernelSpec(W, B, ACTS).arch_act()
    xc = xs[:CHUNK].contiguous()
    dm = torch.randn((CHUNK, mp), dtype=torch.float64, device="cuda")
    beta = torch.randn(CHUNK, dtype=torch.float64, device="cuda")
    gamma = torch.randn(m, dtype=torch.float64, device="cuda")
    out = (ctypes.c_double * (4 * len(W)))()
    out_s = (ctypes.c_double * (2 * d))()
    sh = (ctypes.c_double * d)(*rel)

    def adjoint():
        _lib.check(lib.nngp_sparse_adjoint_rect(_lib.ptr(xc), CHUNK, _lib.ptr(u), m, d, ctypes.byref(arch), _lib.ptr(dm), mp,
                                                _lib.ptr(beta), _lib.ptr(gamma), out, _lib.stream_ptr()), lib)

    def ard_rect():
        _lib.check(lib.nngp_sparse_ard_rect(_lib.ptr(xc), CHUNK, _lib.ptr(u), m, d, ctypes.byref(arch), sh, _lib.ptr(dm), mp,
                                            _lib.ptr(beta), _lib.ptr(gamma), out_s, _lib.stream_ptr()), lib)

    row = {}
    row["adjoint_ms"], row["adjoint_min_ms"] = wall(adjoint, 5)
    row["ard_rect_ms"], row["ard_rect_min_ms"] = wall(ard_rect, 5)
    row["contraction_share_derived"] = (row["ard_rect_ms"] - row["adjoint_ms"]) / row["ard_rect_ms"]
    return row


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_ard_bench.json")
    lib = _lib.load()
    result = {"n": N, "n_dense": len(W), "chunk_rows": CHUNK, "bound": BOUND, "device": torch.cuda.get_device_name(0), "cases": []}
    chunks = N // CHUNK
    for m, d in SHAPES:
        x, y = synth.synthetic_queries(N, d, seed=0)
        xs = torch.from_numpy(np.ascontiguousarray(x / 1000.0)).to("cuda")
        ys = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64).reshape(-1)).to("cuda")
        rel = np.exp(0.3 * np.random.default_rng(11).standard_normal(d))
        idx = np.sort(np.random.RandomState(10).choice(N, size=m, replace=False))
        u = xs[torch.from_numpy(idx).to("cuda")].contiguous()
        row = {"n": N, "m": m, "d": d, "chunks": chunks}
        row.update(chunk_pieces(lib, xs, u, m, d, rel))
        plain = SparseGPModel(m, d, W, B, activations=ACTS, diag_reg=LAM, chunk_rows=CHUNK, jitter=1e-6, test_cap=128).reserve_evidence()
        plain.set_inducing(u).add_rows(xs, ys).finish()
        row["plain_grad_ms"], row["plain_grad_min_ms"] = timed(lambda: plain.evidence_grad(xs, ys, BOUND), 3)
        plain.close()
        model = SparseGPModel(m, d, W, B, activations=ACTS, diag_reg=LAM, chunk_rows=CHUNK, jitter=1e-6, test_cap=128).reserve_evidence_ard()
        model.set_relevance(rel).set_inducing(u).add_rows(xs, ys).finish()
        row["grad_ms"], row["grad_min_ms"] = timed(lambda: model.evidence_grad(xs, ys, BOUND), 3)
        row["grad_ard_ms"], row["grad_ard_min_ms"] = timed(lambda: model.evidence_grad(xs, ys, BOUND, ard=True), 3)
        row["ard_over_grad"] = row["grad_ard_ms"] / row["grad_ms"]
        row["pass_share_of_grad_ard"] = chunks * row["adjoint_ms"] / row["grad_ard_ms"]
        row["extra_share_of_grad_ard"] = chunks * (row["ard_rect_ms"] - row["adjoint_ms"]) / row["grad_ard_ms"]
        nlml, _, gs = model.evidence_grad(xs, ys, BOUND, ard=True)
        row["nlml"], row["grad_s_finite"] = nlml, bool(np.all(np.isfinite(gs)))
        model.close()
        result["cases"].append(row)
        print(json.dumps(row), file=sys.stderr)
        del xs, ys, u
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
