"""The adjoint passes entry by entry over the whole angle range on the MI355X (-m gpu): rect_tile (csrc/sparse_evidence.hip)
through nngp_sparse_adjoint_rect with one-hot seeds, adjoint_tile (csrc/nngp_adjoint.h) through the marginal likelihood at
n = 2, embedded in a 130-row problem, and with relevances -- every component of dK_ij / dtheta held to the per-entry gate of
tests/adjoint_reference.py (mpmath forward-mode referee; the gate comes from the referee alone, no device result took part in
its constants).  Coverage of the pairs (all 65 table entries, both sides of every seam) is asserted in
tests/test_adjoint_angles_host.py.

How the constants of adjoint_reference.CONSTANTS were measured (CPU; printed by tests/test_adjoint_angles_host.py; "beyond" = the
largest error beyond the carried allowance, in units of the entry's unit; float64 reference = sparse_evidence_reference.kernel_rect
/ nngp_mll_reference.kernel_block / nngp_ard_reference.feature_tangent held to extra = 1, restatement = adjoint_reference.device_adjoint):

  family   kind   float64 reference   restatement   C1d = max(4 x the larger, 4 u)
  relu     v      9.76e-17            1.07e-16      4.5e-16   (the exact diagonal, relu2_bias; off the diagonal 0 for both)
  relu     c      3.87e-16            3.82e-16      1.6e-15   (relu2_bias, d2 few)
  relu     s      1.24e-16            1.30e-16      5.2e-16   (relu1, the symmetric d2 block)
  abrelu   v      2.45e-16            2.30e-16      9.9e-16   (Abs, d16 / d2 few)
  abrelu   c      3.47e-16            2.92e-16      1.4e-15   (LeakyRelu, d16 few)
  plain error of the unit, next to theta = 0 and pi: 3.2e-7 / 4.9e-8 (kernel_rect / restatement, relu1 d16), 4.1e-6 / 2.7e-6 (Abs, d2):
  carried, not C1d.
  calpha: float64 NumPy solve of the 2 x 2 systems on the float64 kernel, contracted with the referee's dK, against the referee:
  3.01 (relu1), 3.15 (relu2_bias), 2.59 (relu3), 4.74 (LeakyRelu), 8.69 (Abs) u sum |S dK|  ->  calpha = 4 x 8.69 = 35.
  Referee tangents against central differences of the referee's values (70 digits, h = 1e-18): 1.3e-37 of the unit.
  Restatement with the table index shifted by one: 19.6 x the gate; with t1 and t2 exchanged: 1e2 x the gate on the anchor of
  the sweep's radius, 1e23 .. 1e25 x on the anchors of radius 3 and 13.

Worst device error / gate on the MI355X (this file's printout): rectangular pass 0.79 (relu1: the "ends" blocks, next to 0 and pi;
0.63 on its "few" blocks, d = 64 the same bits as d = 16), relu2_bias 0.27, relu3 0.36, relu4_bias 0.28, LeakyRelu 0.28, Abs 0.47, relu5
(NLC = 8) 0.28, relu9 (NLC = 16) 0.29; symmetric pass at n = 2: relu1 0.16, relu2_bias 0.12, relu3 0.15, relu4_bias 0.13, LeakyRelu 0.14,
Abs 0.25, relu5 0.12, relu9 0.17; the pair in the 130-row problem 0.10 at each of the four placements (the same bits); relevance halves
0.19.  The restatement of the device arithmetic sits at the same levels (0.79 on the same "ends" entry).

Value-only mutations of the device code, each run once on scratch copies against this file and the existing gradient tests
(test_gpu_nngp_mll / _loo / _ard / test_gpu_sparse_evidence without their 4097-row, reference-size, tuning and command-line cases):
  adjoint_tile  4 pi (1 + 1e-12) in rq     the 9 n = 2 cases, the 4 placements, the relevances fail here; every existing test passes
  adjoint_tile  rq[l][ri] for t1 and t2    the same 14 fail here; 61 existing tests fail too (rows of unequal norm are everywhere)
  adjoint_tile  h (1 + 1e-12), reverse     the 5 n = 2 cases with >= 2 hidden layers and the 4 placements fail; every existing passes
  rect_tile     4 pi (1 + 1e-12) in rq     all 15 rectangular cases fail here; every existing test passes
  rect_tile     rq[l][ri] for t1 and t2    all 15 fail here; 24 existing sparse-evidence tests fail too
  rect_tile     h (1 + 1e-12), reverse     the 6 rectangular cases with >= 2 hidden layers fail here; every existing test passes
So the existing aggregate gates are blind to the four last-digit mutations and see the two operand swaps.

Cost on the MI355X host, one run: test_gpu_kernel_angles.py::test_kernel_build_meets_the_gate[relu1], that file's slowest case, 9.7 s;
the slowest test here 6.3 s (the rectangular relu9 case; its referee block is shared with the relu9 n = 2 test, 2.9 s: the
off-diagonal entry of pair j is entry (0, j) of the block "one"), every other test <= 2.4 s; the GPU work itself is 0.1 .. 1.2 s
per test, the rest is the referee.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as D  # noqa: E402
import gpu_util as G  # noqa: E402
from nngp_src_amd import _lib, mll  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = D.cases()


def _acts(net):
    return [tuple(a) for a in net.acts]


# ------------------------------------------------------------------------------------------------ the rectangular pass
class Rect:
    """nngp_sparse_adjoint_rect on fixed rows with one-hot seeds: call(dense entry, rank-one entry) -> the two halves [2, 2 nd]."""

    def __init__(self, x, u, net):
        self.lib = _lib.load()
        self.c, self.m, self.d, self.nd = x.shape[0], u.shape[0], x.shape[1], net.nd
        self.ld = self.m + 5
        self.xd, self.ud = _lib.to_device_f64(x, G.dev()), _lib.to_device_f64(u, G.dev())
        self.seed = torch.zeros((self.c, self.ld), dtype=torch.float64, device=G.dev())
        self.seed[:, self.m:] = float("nan")  # the padding columns are never read
        self.beta = torch.zeros(self.c, dtype=torch.float64, device=G.dev())
        self.gamma = torch.zeros(self.m, dtype=torch.float64, device=G.dev())
        self.arch = _lib.make_arch_act(net.w_std, net.b_std, _acts(net))
        self.out = (ctypes.c_double * (4 * self.nd))()

    def call(self, dense, rank1, value=1.0):
        (i, j), (i2, j2) = dense, rank1
        self.seed[i, j], self.beta[i2], self.gamma[j2] = value, value, 1.0
        _lib.check(self.lib.nngp_sparse_adjoint_rect(_lib.ptr(self.xd), self.c, _lib.ptr(self.ud), self.m, self.d, ctypes.byref(self.arch),
                                                     _lib.ptr(self.seed), self.ld, _lib.ptr(self.beta), _lib.ptr(self.gamma), self.out,
                                                     _lib.stream_ptr()), self.lib)
        got = np.array(self.out[:]).reshape(2, 2 * self.nd)
        self.seed[i, j], self.beta[i2], self.gamma[j2] = 0.0, 0.0, 0.0
        return got[::-1]  # [dense half, rank-one half]


def _calls(n1, n2):
    """[(entry of the dense seed, entry of the rank-one seed)]: entries with i + j even go to the dense seed, the others to the
    rank-one seed, so each path meets every anchor and every other sweep row -- one side of a seam on one path, the other side
    on the other, and the reverse at the next anchor.  The first two and the last two sweep rows (phi = 0 and its neighbour;
    in a full sweep the zero row and the exact duplicate) then go to both."""
    even = [(i, j) for j in range(n2) for i in range(n1) if (i + j) % 2 == 0]
    odd = [(i, j) for j in range(n2) for i in range(n1) if (i + j) % 2 == 1]
    odd += odd[: len(even) - len(odd)]
    even += even[: len(odd) - len(even)]
    return list(zip(even, odd)) + [((i, j), (i, j)) for j in (0, 1, n2 - 2, n2 - 1) for i in range(n1)]


@pytest.mark.parametrize("name,family,kind", [(n, f, k) for n, (_, blocks) in CASES.items() for f, k in blocks])
def test_rectangular_pass_meets_the_gate_entry_by_entry(name, family, kind):
    net = CASES[name][0]
    x1, x2, blk = D.block(family, kind, net)
    n1, n2 = blk.k.shape
    rect = Rect(x1, x2, net)
    calls = _calls(n1, n2)
    got = np.full((2,) + blk.unit.shape, np.nan)  # [path: dense, rank-one][i][j][p]
    for t, (e_dense, e_rank) in enumerate(calls):
        out = rect.call(e_dense, e_rank)
        assert np.all(np.isfinite(out))
        got[0][e_dense], got[1][e_rank] = out[0], out[1]
        if t % 97 == 0:
            assert rect.call(e_dense, e_rank).tobytes() == out.tobytes()  # the same bits
    seen = ~np.isnan(got[..., 0])
    assert np.all(seen[0] | seen[1])
    for a in range(n1):  # both paths see every anchor, the zero row and the duplicate
        for path in (0, 1):
            assert seen[path][a].sum() >= n2 // 2 and seen[path][a][[0, 1, n2 - 2, n2 - 1]].all()
    dead = blk.dead()
    zero_rows = int(np.sum(blk.q1 == 0.0)) * n2 + int(np.sum(blk.q2 == 0.0)) * n1
    bias_free = all(b == 0.0 for b in net.b2)
    assert int(dead.sum()) == (zero_rows * net.nd if bias_free else 0)  # a zero row without biases: the v components, and only they
    worst = 0.0
    for path, label in ((0, "dense"), (1, "rank-one")):
        g = np.where(seen[path][..., None], got[path], blk.hi)
        assert np.all(g[dead & seen[path][..., None]] == 0.0)  # exact zeros; nothing else is left out of the ratio
        ratio, at = blk.ratio(g)
        err, gate = blk.error_abs(g), blk.gate_abs()
        print("%s %s %s, %s seed: worst error / gate %.3f at %s (error %.3e, gate %.3e, unit %.3e)"
              % (name, family, kind, label, ratio, at, err[at], gate[at], blk.unit[at]))
        worst = max(worst, ratio)
    assert worst <= 1.0, (name, family, kind, worst)


def test_seed_values_scale_the_rectangular_pass_exactly():
    """A one-hot seed of 2^-7 gives the one-hot result scaled: the other entries add exact zeros."""
    net = CASES["relu2_bias"][0]
    x1, x2, _ = D.block("d16", "few", net)
    rect = Rect(x1, x2, net)
    for e in ((0, 100), (1, 333), (2, 640)):
        np.testing.assert_array_equal(rect.call(e, e, 2.0 ** -7), rect.call(e, e) * 2.0 ** -7)


# ------------------------------------------------------------------------------------------- the symmetric pass at n = 2
def _hold(pr, key, got, label, worst):
    err, gate = pr.error(key, got), pr.gate[key]
    r = np.where(err > 0, err / np.where(gate > 0, gate, 1.0), 0.0)
    r = np.where((err > 0) & (gate == 0), np.inf, r)
    p = int(np.argmax(r))
    if r[p] > worst[0]:
        worst[:] = [float(r[p]), label, p, float(err[p]), float(gate[p])]


def _run_pairs(handle, net, prs, place=None, n=2, relevance=None):
    """quad_p (both right-hand sides) and trace_p of every pair against the referee; returns the worst error / gate."""
    worst = [0.0, None, None, 0.0, 0.0]
    nc = 2 * net.nd
    d = prs[0].x.shape[1]
    params = (net.w_std, net.b_std, _acts(net))
    for t, pr in enumerate(prs):
        assert pr.cond <= 3.0  # in the referee: equal norms, lambda = K_00
        rows = (0, 1) if place is None else place
        x = np.zeros((n, d))
        x[rows[0]], x[rows[1]] = pr.x[0], pr.x[1]
        for y in pr.RHS:
            yy = np.zeros(n)
            yy[rows[0]], yy[rows[1]] = y
            handle.set_train(x, yy)
            if relevance is None:
                handle.evaluate(params, pr.lam, True)
                tm = handle.terms()
                quad, trace = tm["quad"][:nc], tm["trace"][:nc]
            else:
                handle.evaluate(params, pr.lam, True, relevance=relevance)
                tm = handle.ard_terms()
                quad, trace = tm["half1"], tm["half2"]
                pr_s = _Sub(pr, nc)
                assert np.all(np.isfinite(quad)) and np.all(np.isfinite(trace))
                _hold(pr_s, y, quad, (t, y, "quad"), worst)
                _hold(pr_s, "trace", trace, (t, y, "trace"), worst)
                continue
            assert np.all(np.isfinite(quad)) and np.all(np.isfinite(trace))
            _hold(pr, y, quad, (t, y, "quad"), worst)
            _hold(pr, "trace", trace, (t, y, "trace"), worst)
    return worst


class _Sub:
    """The relevance components of a Pair (those behind the 2 n_dense of the Dense layers)."""

    def __init__(self, pr, nc):
        self.want = {k: v[nc:] for k, v in pr.want.items()}
        self.gate = {k: v[nc:] for k, v in pr.gate.items()}

    error = D.Pair.error


SYM_CASES = [("relu1", "d2"), ("relu1", "d16"), ("relu2_bias", "d2"), ("relu3", "d2"), ("relu4_bias", "d2"), ("leaky", "d16"),
             ("abs", "d2"), ("relu5", "d2"), ("relu9", "d2")]


@pytest.mark.parametrize("name,family", SYM_CASES)
def test_symmetric_pass_at_n_2_meets_the_gate(name, family):
    """The anchor (R, 0) with every sweep row: equal norms, lambda = K_00 (absolute), y = (1, 1) and (1, -1)."""
    net = CASES[name][0]
    prs = D.pairs(family, net)
    m = mll.NNGPMarginalLikelihood(2, prs[0].x.shape[1])
    worst = _run_pairs(m, net, prs)
    m.close()
    print("%s %s n = 2, %d pairs: worst error / gate %.3f at %s component %s (error %.3e, gate %.3e)" % ((name, family, len(prs)) + tuple(worst)))
    assert worst[0] <= 1.0, worst


PLACES = [(1, 0), (63, 5), (64, 63), (129, 64)]
PLACED = [5, 88, 130, 299, 452, 603, 690, 703, 706, 709, 710]  # sweep rows: the grid, seams from both sides, next to 0 and pi, the zero row, the duplicate


@pytest.mark.parametrize("place", PLACES)
def test_the_pair_placed_in_a_130_row_problem(place):
    """A diagonal tile, an off-diagonal tile and the ragged last tile: the other 128 rows are zero rows with y = 0 (bias-free
    network: they decouple exactly; their diagonal entries add 128 dK_zz,p / lambda to the trace of the bias components)."""
    net = CASES["relu3"][0]
    x0, xs = D.pair_rows("d2")
    prs = [D.Pair(x0, xs[j], net, n_zero=128) for j in PLACED]
    m = mll.NNGPMarginalLikelihood(130, 2)
    worst = _run_pairs(m, net, prs, place=place, n=130)
    m.close()
    print("relu3 d2 pair at rows %s of 130: worst error / gate %.3f at %s component %s (error %.3e, gate %.3e)" % ((place,) + tuple(worst)))
    assert worst[0] <= 1.0, worst


def test_relevance_halves_at_n_2_meet_the_gate():
    """nngp_mll_evaluate_ard at unit relevances (family d2, relu1): both halves of d / ds_k from nngp_mll_ard_terms against the
    referee's s_k tangents."""
    net = CASES["relu1"][0]
    prs = D.pairs("d2", net, ard=True)
    m = mll.NNGPMarginalLikelihood(2, 2, ard=True)
    worst = _run_pairs(m, net, prs, relevance=np.ones(2))
    m.close()
    print("relu1 d2 relevances, %d pairs: worst error / gate %.3f at %s component %s (error %.3e, gate %.3e)" % ((len(prs),) + tuple(worst)))
    assert worst[0] <= 1.0, worst
