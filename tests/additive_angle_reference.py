"""Inputs, referee, gate and host restatement for the ADDITIVE kernel build (csrc/kernel_build_additive.hip: k_build_add,
k_diag_add) over the whole angle range, entry by entry (test infrastructure, no tests).  It builds on tests/angle_reference.py
(A below): the families "d2" / "d16", the sweeps, entry() and its angle allowances, CONSTANTS, the restated device arithmetic.

Inputs.  Rows of d = 40 integer columns, every squared norm < 2^51 (every Gram sum in any order is exact).  Three groups carry a
sweep each: G2 = [3, 5) the "d2" family, G16 = [8, 24) the "d16" family with its sweep index permuted against G2's (at one entry the
two groups see different angles), G1 = [30, 31) a width-1 group of integers of magnitude <= 2^12 (k k exact: the angle is exactly 0
or pi) or, in the "big" row sets, odd integers >= 2^20 (k k rounds).  Every other column holds integers of magnitude 2^17 .. 2^19
that differ from row to row and alternate in sign: a group walked one column too far or too short moves its entries by orders of
magnitude more than any gate.  The sweep rows of a rectangular block end in rows whose G2 (G16) slice is bit-identical to an
anchor's while everything else differs -- the `same` rule of group_map off the diagonal; the symmetric rows hold such a pair too.
TABLES holds the group tables on these rows: the three groups, chunk boundaries (widths 8, 9, 17 from odd offsets: one staged
chunk exactly, one feature past it, two chunks and one), two overlapping groups, a group equal to the whole input, widths 3 and 7
(1.0 / width is not exact), a weight of 0, full_weight 0 and 1, and a negative weight (the C ABI refuses that one -- weights must be
>= 0 -- so it is held on the host only, against the float64 reference and the restatement).

Referee.  Per term (a group, or the whole input) A.entry on that slice's exact (k, q, q') = (S, S1, S2) / width, with
exact_diag where the device takes act_diag: a GROUP term whose two slices are bit-identical (k == q == q' bit for bit on the device,
theta = 0 by construction), the whole-input term on the diagonal of a symmetric build only (kernel_build.hip).  Power-of-two
widths: (k, q, q') are float64 numbers and the device has them exactly (initial = 0).  Other widths (3, 7, 9, 17, and the whole
input at d = 40, which is why that term is not taken from A.Block -- its gram() asserts a power of two): the referee starts from
the rationals and entry() counts initial = 2 roundings in each of k, q, q' -- 1.0 / width and the product with it in k_build_add; the
plain build's k likewise, its q = S / d has one.  Every term is taken with kk_exact: where k k is a float64 number behind an exact
Dense layer the term u k^2 of E stands for no rounding and is left out, so exactly collinear small-integer slices get E = 0 and
_ds(0, E) adds nothing, while at |x| >= 2^20 the same formula widens the gate by itself.  The value of an entry is the weighted
sum of the terms in mpmath.

Gate (per entry and output, from the referee alone; u = 2^-53, terms t = the groups of non-zero weight and the whole input):
    gate = sum_t |w_t| (C1 scale_t + carry_t + CD same_t scale_t) + T u sum_t |w_t K_t|
scale_t = sqrt(K_t,ii K_t,jj) of that term, carry_t the angle allowance of A.entry carried to the output (0 for an exact-diagonal
entry: the symmetric build's diagonal carries none), C1 = A.CONSTANTS of the network's family, T the number of terms: one fma per
term of the running sum.  Nothing is added for the widths that are no power of two: entry()'s initial count carries them.
CD is the one constant this module adds, for Theta of an Erf term on identical slices (act_diag) only; it is 0 for every other
family and output.  The composed gate gives such an entry C1 scale alone, but act_diag's kdot = ap3 fast_rcp(w) keeps the relative
error of one Newton step from the reciprocal's seed, and Theta ~ kdot k there.  Measured beyond the composed gate, in units of
same_t scale_t, over every Erf block of tests/test_additive_angles_host.py: the float64 reference < 0 (inside: -2.4e-16), the
restatement 1.891e-15 (erf_abc, the width-1 group at |x| >= 2^20; 7.9e-16 on the symmetric block of erf; its seed is the exact
reciprocal rounded to 24 bits, so one step leaves up to 2^-48 = 3.6e-15).  CD = 4 x 1.891e-15 = 7.6e-15, set as A.CONSTANTS were;
no device result took part.  The diagonal test of tests/test_gpu_kernel_angles.py allows the same entries 1.1e-14.

Host restatement (a diagnostic; no device result is ever accepted against it): the Gram entries by fma chain in feature order
(k-chunks of GKC = 8 are consumed in order into one accumulator per entry, so chunking does not change the order), the multiply by
1.0 / width, the `same` rule, group_map's layer loop through act_diag / act_cross on A.pi_minus_atan2 / A.fast_sqrt_pos / A.fast_rcp
(for an all-ReLU network it is A.device_relu with diag = same, asserted in the host test), affine_lo and erf_cross_comp, the fma
sum in table order, the whole-input term last.
"""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

import angle_reference as A

D = 40
G2, G16, G1 = (3, 5), (8, 24), (30, 31)
FILL = [c for c in range(D) if not any(b <= c < e for b, e in (G2, G16, G1))]
U = A.U
CD = {"erf": {"ntk": 7.6e-15}}
GKC = 8

# name -> (groups, weights, full_weight)
TABLES = {
    "base": ([G2, G16, G1], [1.0, 0.7, 1.3], 0.0),
    "base_full": ([G2, G16, G1], [1.0, 0.7, 1.3], 1.0),
    "chunks": ([(9, 17), (9, 18), (7, 24)], [1.0, 0.5, 2.0], 0.0),
    "overlap": ([G2, (4, 12)], [1.0, 1.0], 0.0),
    "whole": ([(0, D), G2], [0.5, 1.0], 0.0),
    "whole_full": ([(0, D)], [0.5], 1.0),
    "w37": ([(3, 6), (24, 31)], [1.0, 0.25], 0.0),
    "zero_w": ([G2, G16, G1], [1.0, 0.0, 1.3], 0.0),
    "neg_w": ([G2, G16], [1.0, -0.4], 0.0),
    "w1": ([G1], [1.0], 0.0),
    "pair": ([G2], [1.0], 0.0),
    "g16": ([G16], [1.0], 0.0),
}
DEVICE_TABLES = ["chunks", "overlap", "whole", "whole_full", "w37", "zero_w", "base_full"]  # neg_w: refused by the C ABI

# the networks of the GPU file: name -> (Net, table, outputs).  comp3: the whole-input term of an NNGP-only, bias-free build takes
# the composite map, the groups the per-layer map.
_C = A.cases()
NETS = {n: (_C[n][0], "base", ("nngp", "ntk")) for n in ("relu1", "relu2_bias", "relu3_ntk", "leaky", "abs", "erf", "erf_abc")}
NETS["comp3"] = (_C["comp3"][0], "base_full", ("nngp",))

W1_SMALL = [3, -3, 1, 4096, -4096, 1000, 500, -500, 0, 17, -2047, 4095]
W1_BIG = [2 ** 20 + 1, -(2 ** 20 + 1), 2 ** 21 - 1, 3 * 2 ** 19 + 5, -(2 ** 20 + 12345), 2 ** 20 + 777]


# ------------------------------------------------------------------------------------------------------------------ inputs
def _rows(ab2, ab16, w1, phase):
    ab2, ab16 = np.asarray(ab2, np.float64), np.asarray(ab16, np.float64)
    n = ab2.shape[0]
    assert ab16.shape[0] == n and len(w1) == n
    x = np.zeros((n, D))
    i = np.arange(n)[:, None] + phase
    c = np.arange(len(FILL))[None, :]
    x[:, FILL] = (2 ** 17 + 131 * i + 7 * c) * np.where((i + c) % 2 == 0, 1.0, -1.0)
    x[:, G2[0]:G2[1]] = A.embed("d2", ab2)
    x[:, G16[0]:G16[1]] = A.embed("d16", ab16)
    x[:, G1[0]] = np.asarray(w1, np.float64)
    assert np.abs(x[:, FILL]).max() < 2 ** 19 and np.sum(x * x, axis=1).max() < 2.0 ** 51
    return x


def _cycle(vals, n, shift=0):
    return [vals[(i + shift) % len(vals)] for i in range(n)]


def anchor_rows(big=False):
    """Three anchors: per group the `few` anchors of its family (G16's in another order), G1 = 3, -4096, 1000."""
    a2, a16 = anchor_ab_pairs()
    return _rows(a2, a16, W1_BIG[:3] if big else [3, -4096, 1000], 800)


def sweep_ab_pairs():
    """The (a, b) pairs of the sweep rows' G2 and G16 slices (see sweep_rows)."""
    s2, s16 = A.sweep_ab("d2", medium=True), A.sweep_ab("d16", medium=True)
    n = s2.shape[0]
    assert s16.shape[0] == n and math.gcd(331, n) == 1
    s16 = s16[(np.arange(n) * 331 + 17) % n]
    a2, a16 = A.anchors_ab("d2", few=True), np.roll(A.anchors_ab("d16", few=True), 1, axis=0)
    ab2 = np.concatenate([s2, a2, s2[100:103]])
    ab16 = np.concatenate([s16, s16[200:203], a16])
    return ab2, ab16


def anchor_ab_pairs():
    return A.anchors_ab("d2", few=True), np.roll(A.anchors_ab("d16", few=True), 1, axis=0)


def sweep_rows(big=False):
    """The medium sweep in G2, the same sweep permuted in G16, G1 cycling through its values; then six rows whose G2 (G16) slice
    is an anchor's, bit for bit, while every other column differs from that anchor's row."""
    ab2, ab16 = sweep_ab_pairs()
    return _rows(ab2, ab16, _cycle(W1_BIG if big else W1_SMALL, ab2.shape[0]), 0)


def sym_rows():
    """75 rows (a full 64-tile and a ragged one a side: two diagonal tiles, an off-diagonal tile and its mirror image): every
    other direction of A.symmetric_ab, a zero slice, a pair of rows with bit-identical G2 slices."""
    sel = np.concatenate([np.arange(0, 97, 2), np.arange(1, 97, 4), [97, 98]])
    s2, s16 = A.symmetric_ab("d2")[sel], A.symmetric_ab("d16")[sel]
    n = len(sel)
    assert math.gcd(7, n) == 1
    return _rows(s2, s16[(np.arange(n) * 7 + 3) % n], _cycle(W1_SMALL, n, 2), 1600)


def block_rows(kind):
    """kind: "few" (3 anchors x sweep), "big" (the same with G1 >= 2^20), "sym" (x2 None)."""
    if kind == "sym":
        return sym_rows(), None
    return anchor_rows(kind == "big"), sweep_rows(kind == "big")


def same_slices(a, c):
    return np.all(a[:, None, :] == c[None, :, :], axis=2)


# ------------------------------------------------------------------------------------------------------------------ referee
def _ints(x):
    out = x.astype(np.int64).astype(object)
    assert np.all(out.astype(np.float64) == x)
    return out


class Term:
    """One term (a group [b, e), or the whole input: full) of a block, from the referee: val[g] (mpmath, object arrays),
    scale[g], carry[(g, extra)] (absolute), same (where the device takes act_diag), initial."""

    def __init__(self, x1, x2, b, e, net, sym, full, extras):
        a, c = x1[:, b:e], (x1 if sym else x2)[:, b:e]
        width = e - b
        pow2 = width & (width - 1) == 0
        self.initial = 0 if pow2 else 2
        ia, ic = _ints(a), _ints(c)
        s, s1, s2 = ia @ ic.T, (ia * ia).sum(axis=1), (ic * ic).sum(axis=1)
        n1, n2 = s.shape
        if full:
            self.same = np.eye(n1, dtype=bool) if sym else np.zeros((n1, n2), dtype=bool)
        else:
            self.same = same_slices(a, c)
            if sym:
                assert self.same.diagonal().all()
        self.mask = np.tril(np.ones((n1, n2), dtype=bool)) if sym else np.ones((n1, n2), dtype=bool)
        c0 = A.CONSTANTS["c0"]

        def num(v):  # a float64 number where the device has it exactly, the rational otherwise
            return float(v) / width if pow2 else mp.mpf(int(v)) / width

        if pow2:
            assert max(int(s1.max()), int(s2.max())) < 2 ** 51
        diag = {}
        for v in set(s1.tolist()) | set(s2.tolist()):
            q = num(v)
            diag[v] = A.entry(q, q, q, net, c0, exact_diag=True)[:2]
        self.val = {g: np.empty((n1, n2), dtype=object) for g in ("nngp", "ntk")}
        self.carry = {(g, x): np.zeros((n1, n2)) for g in ("nngp", "ntk") for x in extras}
        self.scale = {g: np.array([[float(mp.sqrt(diag[s1[i]][o] * diag[s2[j]][o])) for j in range(n2)] for i in range(n1)])
                      for o, g in enumerate(("nngp", "ntk"))}
        memo = {}
        for i, j in zip(*np.nonzero(self.mask)):
            key = (s[i, j], s1[i], s2[j], bool(self.same[i, j]))
            hit = memo.get(key)
            if hit is None:
                hit = memo[key] = A.entry(num(key[0]), num(key[1]), num(key[2]), net, c0, exact_diag=key[3], extras=extras,
                                          initial=self.initial, kk_exact=True)
            self.val["nngp"][i, j], self.val["ntk"][i, j] = hit[0], hit[1]
            for g, v in (("nngp", hit[2]), ("ntk", hit[3])):
                for x, vx in zip(extras, v):
                    self.carry[(g, x)][i, j] = float(vx)


_TERMS = {}


def term(x1, x2, b, e, net, sym, full, extras):
    c = x1 if sym else x2
    key = (x1[:, b:e].tobytes(), c[:, b:e].tobytes(), x1.shape[0], b - e, net.key(), sym, bool(full) and sym)
    hit = _TERMS.get(key)
    if hit is None or not set(extras) <= {x for _, x in hit.carry}:
        hit = _TERMS[key] = Term(x1, x2, b, e, net, sym, full, tuple(extras))
    return hit


def live_terms(table):
    """[(b, e, weight, full)] in the device's order: the groups of non-zero weight, then the whole input."""
    groups, weights, w0 = table
    out = [(b, e, w, False) for (b, e), w in zip(groups, weights) if w != 0.0]
    return out + ([(0, D, w0, True)] if w0 != 0.0 else [])


class AddBlock:
    """Referee and gate of the additive kernel on a block (sym: x2 = x1, the lower triangle)."""

    def __init__(self, x1, x2, net, table, sym=False, extras=(0.0,)):
        self.net, self.sym, self.table, self.extras = net, sym, table, tuple(extras)
        self.terms = [(w, term(x1, x2, b, e, net, sym, full, self.extras), (b, e), full) for b, e, w, full in live_terms(table)]
        self.mask = self.terms[0][1].mask
        self.shape = self.mask.shape
        self.val, self.absum = {}, {}
        for g in ("nngp", "ntk"):
            v, a = np.zeros(self.shape, dtype=object), np.zeros(self.shape, dtype=object)
            for w, t, _, _ in self.terms:
                wm = mp.mpf(w)
                tv = np.where(self.mask, t.val[g], mp.mpf(0))
                v, a = v + wm * tv, a + abs(wm) * np.abs(tv)
            self.val[g], self.absum[g] = v, a
        # sqrt(K_ii K_jj) of the summed kernel, for printing errors in units of scale
        self.scale = {g: sum(abs(w) * t.scale[g] for w, t, _, _ in self.terms) for g in ("nngp", "ntk")}

    def value(self, which):
        return np.where(self.mask, self.val[which], mp.mpf(0)).astype(np.float64)

    def gate_abs(self, which, extra=0.0, c1=None):
        c1 = A.CONSTANTS[self.net.family][which] if c1 is None else c1
        out = len(self.terms) * U * self.absum[which].astype(np.float64)
        cd = CD.get(self.net.family, {}).get(which, 0.0)
        for w, t, _, _ in self.terms:
            out = out + abs(w) * (c1 * t.scale[which] + t.carry[(which, extra)] + cd * t.same * t.scale[which])
        return np.where(self.mask, out, 0.0)

    def error_abs(self, got, which):
        got = np.asarray(got, dtype=np.float64)
        out = np.zeros(self.shape)
        for i, j in zip(*np.nonzero(self.mask)):
            out[i, j] = float(abs(mp.mpf(float(got[i, j])) - self.val[which][i, j]))
        return out

    def ratio(self, got, which, extra=0.0, where=None):
        """Worst error / gate (over `where`, default every entry of the mask), where, the error over scale there."""
        err, gate = self.error_abs(got, which), self.gate_abs(which, extra)
        sel = self.mask if where is None else (self.mask & where)
        r = np.where(err > 0, err / np.where(gate > 0, gate, 1.0), 0.0)
        r = np.where(sel, np.where((err > 0) & (gate == 0), np.inf, r), 0.0)
        at = np.unravel_index(int(np.argmax(r)), r.shape)
        sc = self.scale[which][at]
        return float(r[at]), (int(at[0]), int(at[1])), float(err[at] / sc) if sc > 0 else 0.0


_BLOCKS = {}


def block(kind, net, table_name, extras=(0.0,)):
    """Cached (x1, x2, AddBlock)."""
    key = (kind, net.key(), table_name)
    hit = _BLOCKS.get(key)
    if hit is None or not set(extras) <= set(hit[2].extras):
        x1, x2 = block_rows(kind)
        hit = _BLOCKS[key] = (x1, x2, AddBlock(x1, x2, net, TABLES[table_name], sym=kind == "sym", extras=extras))
    return hit


def diag_referee(x, net, table):
    """K(x, x), Theta(x, x) per row of the summed kernel in mpmath, and sum_t |w_t K_t| (the unit of its allowance)."""
    out = []
    for i in range(x.shape[0]):
        kn = kt = an = at = mp.mpf(0)
        for b, e, w, _ in live_terms(table):
            width = e - b
            s = int((_ints(x[i:i + 1, b:e]) ** 2).sum())
            q = float(s) / width if width & (width - 1) == 0 else mp.mpf(s) / width
            k, t = A.entry(q, q, q, net, A.CONSTANTS["c0"], exact_diag=True)[:2]
            kn, kt, an, at = kn + mp.mpf(w) * k, kt + mp.mpf(w) * t, an + abs(w) * abs(k), at + abs(w) * abs(t)
        out.append((kn, kt, an, at))
    return out


# ------------------------------------------------------------------------------------------------------- host restatement
def act_params(spec):
    """ArchDev::ap of a hidden layer (api.hip)."""
    if spec[0] == "erf":
        a, b, c = spec[1:]
        p0, p1 = a * a * (2.0 / math.pi), 2.0 * b * b
        return (p0, p1, c * c, p0 * p1)
    if spec[0] == "abrelu":
        a, b = spec[1:]
        return (a * b, (b - a) * (b - a), 0.5 * (a * a + b * b), 0.0)
    return (0.0, 0.0, 0.0, 0.0)


def act_diag(spec, ap, q, tab):
    if spec[0] == "erf":
        w = A.fast_sqrt_pos(A.fma(2.0 * ap[1], q, 1.0))
        return A.fma(ap[0], A.pi_minus_atan2(w, ap[1] * q, tab)[0] - 0.5 * math.pi, ap[2]), ap[3] * A.fast_rcp(w)
    if spec[0] == "abrelu":
        return ap[2] * q, np.full(np.shape(q), ap[2])
    return 0.5 * q, np.full(np.shape(q), 0.5)


def act_cross(spec, ap, k, q1, q2, tab, lo=None):
    """act_cross of act_map.h; lo: erf_cross_comp's first-order term of the lo parts (None: the plain build's bracket)."""
    if spec[0] == "erf":
        kk = k * k
        br = A.fma(q1, q2, -kk) + A.fma(-k, k, kk)
        br = np.maximum(br if lo is None else br + lo, 0.0)
        w = A.fast_sqrt_pos(A.fma(ap[1] * ap[1], br, A.fma(ap[1], q1 + q2, 1.0)))
        return A.fma(ap[0], A.pi_minus_atan2(w, ap[1] * k, tab)[0] - 0.5 * math.pi, ap[2]), ap[3] * A.fast_rcp(w)
    rr = A.fma(q1, q2, -(k * k))
    s = A._sqrt_or_zero(rr)
    kr = A.pi_minus_atan2(s, k, tab)[0] * (0.5 / math.pi)
    kk = A.fma(kr, k, s * (0.5 / math.pi))
    if spec[0] == "abrelu":
        return A.fma(ap[0], k, ap[1] * kk), A.fma(ap[1], kr, ap[0])
    return kk, kr


def affine_lo(w2, x, b2, hi):
    p = w2 * x
    ep = A.fma(w2, x, -p)
    s = p + b2
    bb = s - p
    es = (p - (s - bb)) + (b2 - bb)
    return (s - hi) + (ep + es)


def group_map(k, q1, q2, net, tab, same, comp=True):
    """group_map<NTK> of kernel_build_additive.hip on arrays k [n1, n2], q1 [n1], q2 [n2]; comp False: layer_map_act of
    kernel_build.hip (no compensated Erf bracket; same = its exact diagonal, where k is q1).  Returns (K, T)."""
    k = np.array(k, dtype=np.float64)
    q1, q2 = np.array(q1, dtype=np.float64), np.array(q2, dtype=np.float64)
    t = np.zeros_like(k)
    for l in range(net.nd):
        w2, b2 = net.w2[l], net.b2[l]
        hidden = l < net.nd - 1
        spec = net.acts[l] if hidden else ("relu",)
        erf = hidden and spec[0] == "erf" and comp
        a1, a2 = q1, q2
        q1, q2 = A.fma(w2, a1, b2), A.fma(w2, a2, b2)
        kk = A.fma(w2, k, b2)
        tt = A.fma(w2, t, kk)
        if hidden:
            ap = act_params(spec)
            qq1, qq2 = np.broadcast_to(q1[:, None], k.shape), np.broadcast_to(q2[None, :], k.shape)
            lo = None
            if erf:
                q1l, q2l = affine_lo(w2, a1, b2, q1), affine_lo(w2, a2, b2, q2)
                kl = affine_lo(w2, k, b2, kk)
                lo = A.fma(qq1, np.broadcast_to(q2l[None, :], k.shape), A.fma(qq2, np.broadcast_to(q1l[:, None], k.shape), -2.0 * (kk * kl)))
            kc, kdc = act_cross(spec, ap, kk, qq1, qq2, tab, lo)
            kdg, kdd = act_diag(spec, ap, kk, tab)
            kk, kd = np.where(same, kdg, kc), np.where(same, kdd, kdc)
            tt = tt * kd
            q1, q2 = act_diag(spec, ap, q1, tab)[0], act_diag(spec, ap, q2, tab)[0]
        k, t = kk, tt
    return k, t


def device_group(x1, x2, b, e, net, tab):
    """One group's term as k_build_add forms it: (K, T, same)."""
    a, c = x1[:, b:e], x2[:, b:e]
    acc = np.zeros((a.shape[0], c.shape[0]))
    qa, qb = np.zeros(a.shape[0]), np.zeros(c.shape[0])
    for k0 in range(0, e - b, GKC):
        for f in range(k0, min(k0 + GKC, e - b)):
            qa, qb = A.fma(a[:, f], a[:, f], qa), A.fma(c[:, f], c[:, f], qb)
            acc = A.fma(a[:, f][:, None], c[:, f][None, :], acc)
    inv = 1.0 / float(e - b)
    k, q1, q2 = acc * inv, qa * inv, qb * inv
    same = (q1[:, None] == k) & (q2[None, :] == k)
    kk, tt = group_map(k, q1, q2, net, tab, same)
    return kk, tt, same


def device_full(x1, x2, net, tab, sym, composite=False):
    """The whole-input term as kernel_build.hip forms it (q = S / d, k = S (1.0 / d); the exact diagonal of a symmetric build)."""
    d = x1.shape[1]
    s = x1 @ x2.T  # integers below 2^51: exact in any order
    q1, q2 = np.sum(x1 * x1, axis=1) / d, np.sum(x2 * x2, axis=1) / d
    k = s * (1.0 / d)
    dg = np.eye(x1.shape[0], dtype=bool) if sym else np.zeros(k.shape, dtype=bool)
    if composite:
        return A.device_composite(k, q1, q2, net, tab, dg if sym else None)[0], None
    k = np.where(dg, np.broadcast_to(q1[:, None], k.shape), k)
    return group_map(k, q1, q2, net, tab, dg, comp=False)


def device_additive(x1, x2, net, table, sym=False, composite=False):
    """The restated additive build: {"nngp", "ntk"} and the `same` masks per live group."""
    tab, _ = A.parse_trig_tab()
    x2 = x1 if sym else x2
    sn, st = np.zeros((x1.shape[0], x2.shape[0])), np.zeros((x1.shape[0], x2.shape[0]))
    sames = []
    for b, e, w, full in live_terms(table):
        if full:
            kk, tt = device_full(x1, x2, net, tab, sym, composite)
        else:
            kk, tt, same = device_group(x1, x2, b, e, net, tab)
            sames.append(same)
        sn = A.fma(w, kk, sn)
        st = A.fma(w, tt, st) if tt is not None else st
    return {"nngp": sn, "ntk": st}, sames
