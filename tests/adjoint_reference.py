"""Referee, unit, gate and host restatement for the adjoint passes entry by entry over the whole angle range (test
infrastructure, no tests).

The device differentiates the layer recursion by a reverse sweep per entry (adjoint_tile in csrc/nngp_adjoint.h, its copy
rect_tile in csrc/sparse_evidence.hip): with a one-hot seed the pass returns dK_ij / dtheta_p of ONE entry for every component
p (v_l = w_std_l^2 at 2 l, c_l = b_std_l^2 at 2 l + 1, the order of include/nngp_mll.h).  This module gives that number a
referee, a unit and a gate, on the exact-input rows of tests/angle_reference.py (whose sweep, anchors, block kinds, table
restatement and coverage counter it reuses).

Referee.  mpmath at 40 digits from the float64 (k, q, q'): FORWARD-mode tangents of the recursion, all components in one pass
(a different method from the device's reverse sweep).  Dense l: dk <- v dk (+ k for p = 2 l, + 1 for p = 2 l + 1), likewise
dq, dq'.  Activation (ReLU: a = 0, b = 1): dk <- ck dk + t1 dq + t2 dq', ck = a b + (b - a)^2 kdot, t1 = (b - a)^2 s / (4 pi q1)
with q1 the layer's input norm AFTER its Dense layer, dq <- h dq, h = (a^2 + b^2) / 2.  Rules: t1 = 0 where q1 = 0 (the q = 0
rule of nngp_mll.h); exact_diag (the symmetric pass's diagonal): theta = 0, dk <- h dk; the rectangular pass has no diagonal
rule.  A relevance s_k at unit relevances enters as a further component with dk = x_ik x_jk / d, dq = x_ik^2 / d,
dq' = x_jk^2 / d before Dense 0 (kind "s").

Unit of an entry's error: the same recursion with every term taken by absolute value -- |ck|, and for the k that Dense layer l
injects into dK / dv_l the value recursion with |.| on its terms as well (ka' = |a b| ka + (b - a)^2 (s / 2 pi + kdot ka)): next
to theta = pi K' = s / 2 pi + kdot k is a difference of two terms 1e4 .. 1e13 times its size, and |K'| would be no unit.
sqrt(|dK_ii,p| |dK_jj,p|) is no unit either: where a row of radius 3 meets one of radius 2^20, t1 = s / (4 pi q1) is of order
1e5 while the diagonal's derivative with respect to a bias is of order 1, and honest float64 code is off by 1e-11 .. 1e-9 of it.

Gate (per entry and component, from the referee alone):  C1d[family][kind] unit + sum over hidden layers l of
|T(theta_l +- d_theta_l) - T|, the tangent re-evaluated through the remaining layers with layer l's angle moved by the
d_theta_l of angle_reference.py (C0 + |k| ds(E_l) / rho^2 with its counted roundings, extra = 1 for code that rounds q q'
unfused; k = rho cos theta and s = rho sin theta move together).  The tangents are first order in theta like the NTK: next to
theta = 0 and pi the cancellation of q q' - k^2 costs up to 1e-7 of the unit, and the carried allowance is what admits that, not
C1d.  Two things the value gate did not need are counted here, each because a measurement showed it missing:
 1. dK / dv_l = kbar_l k_in reads the k that went INTO Dense layer l, k = v k_in + c.  The rotation moves k, so it moves
    k_in = (k - c) / v with it; left unmoved, the first-order terms of dK / dv_0 = kdot k_in + s / 2 pi cancel (-k_in + k = 0)
    and its carried allowance came out as 2e-20 where the identical number dK / dv_1 = K' (w_std = 1) had 2e-7.
 2. C0 is the ABSOLUTE error of the arctangent (5.2e-16 rad measured for pi_minus_atan2, 3.4e-16 for pi - arctan2; x 4).  Applied
    as a rotation it cancels to first order in K' = kdot k + s / 2 pi (d / d theta = -kdot s), and for the values the remainder
    |k| C0 / 2 pi sits inside C1 scale, scale = rho / 2.  The unit here is smaller than scale by (pi - theta) / pi next to pi, so
    the remainder is carried: the sweep also moves kdot ALONE by C0 / 2 pi, k and s held (the tangent is affine in kdot_l up to
    what the later layers do with K': one side is taken).  Without it the restatement is 1.4e-15 of the unit beyond the
    allowance at theta = pi - 0.0225 (pi_minus_atan2's 6.5e-17 rad there are 2.9e-15 of pi - theta) and kernel_rect 8.1e-12 ..
    1.3e-11 at pi - 1e-5 (arctan2 rounds theta at the size of pi); with it both are inside on every case, and the v components
    need no C1d beyond 4 u.
Where unit and carried allowance are both 0 -- the v components of a zero row in a bias-free network -- the device must return
an exact 0.

Host restatement.  device_adjoint follows rect_tile / adjoint_tile per entry, step for step (forward recursion with kin, ck, cs,
the q chain with rq = 1 / (4 pi q'), the reverse loop, every fma as written) on angle_reference's fma, pi_minus_atan2 and
fast_sqrt_pos.  It is a diagnostic and the source of C1d; a device result is never accepted against it.
"""
from __future__ import annotations

import math
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import angle_reference as A  # noqa: E402

mp.mp.dps = 40
U = A.U
_PI = mp.pi

# C1d[family][component kind], in units of the entry's unit: 4 x the larger of the restatement's and the float64 reference's
# error beyond the carried allowance, not below 4 u.  calpha: 4 x the error of a float64 NumPy solve of the 2 x 2 systems of
# the symmetric tests, in units of u sum |S_ij dK_ij|.  tests/test_adjoint_angles_host.py prints every figure behind them; the
# figures are in the module docstring of tests/test_gpu_adjoint_angles.py.
CONSTANTS = {
    "relu": {"v": 4.5e-16, "c": 1.6e-15, "s": 5.2e-16},
    "abrelu": {"v": 9.9e-16, "c": 1.4e-15, "s": 4.5e-16},
    "calpha": 35.0,
}


def kinds(net, ns=0):
    """Component kinds in output order: v, c per Dense layer, then ns relevances."""
    return ["v", "c"] * net.nd + ["s"] * ns


def cases():
    """name -> (Net, [(family, block kind)]).  few: three anchors (one of radius 3, one of radius 13) x the medium sweep; one: the
    anchor at the sweep's radius alone (the deep networks); ends: angles next to 0 and pi; d64: d16 rows padded with 48 zero
    coordinates, so that the pass walks two 32-feature chunks."""
    few = [("d2", "few"), ("d16", "few")]
    one = [("d2", "one")]
    return {
        "relu1": (A.relu_net(1), few + [("d2", "ends"), ("d16", "ends"), ("d64", "few")]),
        "relu2_bias": (A.relu_net(2, 1.4, 0.25), few),
        "relu3": (A.relu_net(3), one),
        "relu4_bias": (A.relu_net(4, 1.4, 0.25), one),
        "leaky": (A.Net([1.1, 1.1], [0.3, 0.3], [A.ACTS["leaky"]]), few),
        "abs": (A.Net([1.1, 1.1], [0.0, 0.0], [A.ACTS["abs"]]), few),
        "relu5": (A.relu_net(4, 1.2, 0.1), one),    # 5 Dense layers: NLC = 8
        "relu9": (A.relu_net(8, 1.3, 0.0), one),    # 9 Dense layers: NLC = 16
    }


def block_rows(family, kind):
    if family == "d64":
        x1, x2 = A.block_rows("d16", kind)
        return np.pad(x1, ((0, 0), (0, 48))), np.pad(x2, ((0, 0), (0, 48)))
    return A.block_rows(family, kind)


# ------------------------------------------------------------------------------------------------------------------ referee
def _sweep(net, l0, k, q1, q2, dk, d1, d2, dth=None, dkd=None, diag=False, absolute=False, trace=None):
    """Dense layers l0 .. of the recursion with tangents from the state before Dense layer l0; dth moves hidden layer l0's angle.
    absolute: every term of the tangent recursion by absolute value (the unit).  Returns (K, [dK / dtheta_p])."""
    nd, n2 = net.nd, 2 * net.nd
    dk, d1, d2 = list(dk), list(d1), list(d2)
    act = [p for p in range(len(dk)) if p >= n2 or p < 2 * l0]
    ka = abs(k)  # the value recursion with every term by absolute value: what the unit injects for k
    for l in range(l0, nd):
        if trace is not None:
            trace.append([k, q1, q2, list(dk), list(d1), list(d2), None])
        v, c = net.mw2[l], net.mb2[l]
        for p in act:
            dk[p], d1[p], d2[p] = v * dk[p], v * d1[p], v * d2[p]
        dk[2 * l], d1[2 * l], d2[2 * l] = (ka if absolute else k), q1, q2
        dk[2 * l + 1] = d1[2 * l + 1] = d2[2 * l + 1] = mp.mpf(1)
        act = act + [2 * l, 2 * l + 1]
        k, q1, q2, ka = v * k + c, v * q1 + c, v * q2 + c, v * ka + c
        if l == nd - 1:
            break
        spec = net.acts[l]
        a, b = (mp.mpf(0), mp.mpf(1)) if spec[0] == "relu" else (mp.mpf(spec[1]), mp.mpf(spec[2]))
        assert spec[0] in ("relu", "abrelu")
        ab, bma2, h = a * b, (b - a) ** 2, (a * a + b * b) / 2
        if diag:
            k, q1, q2, ka = h * k, h * q1, h * q2, h * ka
            for p in act:
                dk[p], d1[p], d2[p] = h * dk[p], h * d1[p], h * d2[p]
            continue
        rho2 = q1 * q2
        rr = rho2 - k * k
        s = mp.sqrt(rr) if rr > 0 else mp.mpf(0)
        th = _PI / 2 if (s == 0 and k == 0) else mp.atan2(s, k)
        if trace is not None:
            trace[-1][6] = (k, s, rho2)
        if dth is not None and l == l0:
            th = min(max(th + dth, mp.mpf(0)), +_PI)
            rho = mp.sqrt(rho2)
            k, s = rho * mp.cos(th), rho * mp.sin(th)
            if v > 0:  # dk / dv_l = the k that went into Dense layer l: it moves with k
                dk[2 * l] = (k - c) / v
        kd = (_PI - th) / (2 * _PI)
        if dkd is not None and l == l0:
            kd = kd + dkd
        kr = s / (2 * _PI) + kd * k
        kn, ck, cs = ab * k + bma2 * kr, ab + bma2 * kd, bma2 * s
        t1 = cs / (4 * _PI * q1) if q1 > 0 else mp.mpf(0)
        t2 = cs / (4 * _PI * q2) if q2 > 0 else mp.mpf(0)
        if absolute:
            ck = abs(ck)
        for p in act:
            dk[p] = ck * dk[p] + t1 * d1[p] + t2 * d2[p]
            d1[p], d2[p] = h * d1[p], h * d2[p]
        k, q1, q2, ka = kn, h * q1, h * q2, abs(ab) * ka + bma2 * (s / (2 * _PI) + kd * ka)
    return k, dk


def _moved(net, l0, k, q1, q2, dk, d1, d2, dth=None, dkd=None):
    """The tangents of _sweep(net, l0, ..., dth / dkd) for the gate's perturbed re-evaluations, at a cost that does not grow with
    layers x components: the scalars of the layers l0 .. (forward), then the row vector (d K_out / d dk, / d dq, / d dq') pulled
    back through them, contracted once with every component's state before Dense layer l0 and with what the later Dense
    layers inject.  Only the differences to the forward-mode tangents enter the gate; test_adjoint_angles_host.py holds the two
    routes to each other."""
    nd, n2 = net.nd, 2 * net.nd
    steps = []  # per Dense layer: (v, (k, q1, q2) into it, (ck, t1, t2, h) of the activation after it or None)
    for l in range(l0, nd):
        v, c = net.mw2[l], net.mb2[l]
        kin = k
        k, a1, a2 = v * k + c, v * q1 + c, v * q2 + c
        if l == nd - 1:
            steps.append((v, (kin, q1, q2), None))
            break
        spec = net.acts[l]
        a, b = (mp.mpf(0), mp.mpf(1)) if spec[0] == "relu" else (mp.mpf(spec[1]), mp.mpf(spec[2]))
        ab, bma2, h = a * b, (b - a) ** 2, (a * a + b * b) / 2
        rho2 = a1 * a2
        rr = rho2 - k * k
        s = mp.sqrt(rr) if rr > 0 else mp.mpf(0)
        th = _PI / 2 if (s == 0 and k == 0) else mp.atan2(s, k)
        if dth is not None and l == l0:
            th = min(max(th + dth, mp.mpf(0)), +_PI)
            rho = mp.sqrt(rho2)
            k, s = rho * mp.cos(th), rho * mp.sin(th)
            if v > 0:
                kin = (k - c) / v
        kd = (_PI - th) / (2 * _PI)
        if dkd is not None and l == l0:
            kd = kd + dkd
        cs = bma2 * s
        t1 = cs / (4 * _PI * a1) if a1 > 0 else mp.mpf(0)
        t2 = cs / (4 * _PI * a2) if a2 > 0 else mp.mpf(0)
        steps.append((v, (kin, q1, q2), (ab + bma2 * kd, t1, t2, h)))
        k, q1, q2 = ab * k + bma2 * (s / (2 * _PI) + kd * k), h * a1, h * a2
    out = [None] * len(dk)
    rk, r1, r2 = mp.mpf(1), mp.mpf(0), mp.mpf(0)
    for l in range(nd - 1, l0 - 1, -1):
        v, (kin, x1, x2), act = steps[l - l0]
        if act is not None:
            ck, t1, t2, h = act
            rk, r1, r2 = rk * ck, rk * t1 + r1 * h, rk * t2 + r2 * h
        out[2 * l], out[2 * l + 1] = rk * kin + r1 * x1 + r2 * x2, rk + r1 + r2
        rk, r1, r2 = v * rk, v * r1, v * r2
    for p in range(len(dk)):
        if p >= n2 or p < 2 * l0:
            out[p] = rk * dk[p] + r1 * d1[p] + r2 * d2[p]
    return out


def d_thetas(net, infos, extra=0.0, c0=None):
    """The angle allowance per hidden layer: the d_theta_l of angle_reference.entry, with its counted roundings."""
    c0 = A.CONSTANTS["c0"] if c0 is None else c0
    ek = eq = 0
    out = []
    for l in range(net.nd - 1):
        dc = A._dense_count(net, l)
        ek, eq = ek + dc, eq + dc
        kl, sl, rho2 = infos[l]
        dth = mp.mpf(c0)
        if rho2 > 0:
            e = U * (kl * kl + 2 * ek * abs(kl) * mp.sqrt(rho2) + (2 * eq + extra) * rho2)
            dth = dth + abs(kl) * A._ds(sl, e) / rho2
        out.append(dth)
        ek += 5
    return out


def entry(k, q1, q2, net, exact_diag=False, s0=(), extras=(0.0,), gate=True):
    """One entry from float64 (k, q1, q2): (K, [T_p], [unit_p], {extra: [carried allowance_p]}), p over the 2 n_dense components
    and then one per triple of s0 = [(x_ik x_jk / d, x_ik^2 / d, x_jk^2 / d)].  T in mpmath, the rest float."""
    k, q1, q2 = mp.mpf(float(k)), mp.mpf(float(q1)), mp.mpf(float(q2))
    if exact_diag:
        k = q2 = q1
    nc = 2 * net.nd
    zero = [mp.mpf(0)] * nc
    dk = zero + [mp.mpf(float(t[0])) for t in s0]
    d1 = zero + [mp.mpf(float(t[1])) for t in s0]
    d2 = zero + [mp.mpf(float(t[2])) for t in s0]
    if exact_diag:
        d2 = d1 = dk = zero + [mp.mpf(float(t[1])) for t in s0]
    trace = []
    kk, tt = _sweep(net, 0, k, q1, q2, dk, d1, d2, diag=exact_diag, trace=trace)
    _, un = _sweep(net, 0, k, q1, q2, [abs(v) for v in dk], d1, d2, diag=exact_diag, absolute=True)
    carry = {e: [0.0] * len(tt) for e in extras}
    if gate and not exact_diag:
        nh = net.nd - 1
        dkd = mp.mpf(A.CONSTANTS["c0"]) / (2 * _PI)
        alone = [mp.mpf(0)] * len(tt)  # kdot alone moved by C0 / 2 pi, per layer, summed (affine in kdot: one side)
        for l in range(nh):
            t2 = _moved(net, l, *trace[l][:6], dkd=dkd)
            alone = [w + abs(x - y) for w, x, y in zip(alone, t2, tt)]
        for e in extras:
            g = alone
            for l, dth in enumerate(d_thetas(net, [t[6] for t in trace[:nh]], e)):
                worst = [mp.mpf(0)] * len(tt)
                for sg in (1, -1):
                    t2 = _moved(net, l, *trace[l][:6], dth=sg * dth)
                    worst = [max(w, abs(x - y)) for w, x, y in zip(worst, t2, tt)]
                g = [x + w for x, w in zip(g, worst)]
            carry[e] = [float(x) for x in g]
    return kk, tt, [float(x) for x in un], carry


def _split(t):
    """An mpmath value as (hi, lo) float64 with hi + lo = t to 32 digits: lets the error |got - t| be formed in NumPy."""
    hi = float(t)
    return hi, float(t - mp.mpf(hi))


class Block:
    """Referee, unit and gate of dK_ij / dtheta_p on a block x1 x x2^T (sym: x2 = x1 with the exact diagonal, lower triangle).
    ard: also the d relevance components of family d2 rows."""

    def __init__(self, x1, x2, net, sym=False, extras=(0.0,), ard=False):
        self.net, self.sym, self.extras = net, sym, tuple(extras)
        x2 = x1 if sym else x2
        self.k, self.q1, self.q2 = A.gram(x1, x2)
        n1, n2 = self.k.shape
        d = x1.shape[1]
        ns = d if ard else 0
        self.kinds = kinds(net, ns)
        nc = len(self.kinds)
        self.hi, self.lo, self.unit = (np.zeros((n1, n2, nc)) for _ in range(3))
        self.carry = {e: np.zeros((n1, n2, nc)) for e in self.extras}
        self.mask = np.tril(np.ones((n1, n2), dtype=bool)) if sym else np.ones((n1, n2), dtype=bool)
        self.khi = np.zeros((n1, n2))
        self.raw = {}  # (i, j) -> what entry() returned: the n = 2 problems reuse the off-diagonal entries of a block
        for i, j in zip(*np.nonzero(self.mask)):
            s0 = [(x1[i, f] * x2[j, f] / d, x1[i, f] ** 2 / d, x2[j, f] ** 2 / d) for f in range(ns)]
            kk, tt, un, carry = entry(self.k[i, j], self.q1[i], self.q2[j], net, exact_diag=sym and i == j, s0=s0, extras=self.extras)
            self.khi[i, j] = float(kk)
            self.raw[(int(i), int(j))] = (kk, tt, un, carry)
            for p, t in enumerate(tt):
                self.hi[i, j, p], self.lo[i, j, p] = _split(t)
            self.unit[i, j] = un
            for e in self.extras:
                self.carry[e][i, j] = carry[e]

    def c1(self):
        return np.array([CONSTANTS[self.net.family][kd] for kd in self.kinds])

    def error_abs(self, got):
        """|got - referee| [n1, n2, nc] (0 outside the mask)."""
        got = np.asarray(got, dtype=np.float64)
        return np.where(self.mask[:, :, None], np.abs((got - self.hi) - self.lo), 0.0)

    def gate_abs(self, extra=0.0, c1=None):
        return (self.c1() if c1 is None else c1) * self.unit + self.carry[extra]

    def over(self, got, extra=0.0):
        """(error - carried allowance) / unit per component kind: what C1d is 4 x the worst of."""
        ex = (self.error_abs(got) - self.carry[extra]) / np.where(self.unit > 0, self.unit, 1.0)
        ex = np.where((self.unit > 0) & self.mask[:, :, None], ex, 0.0)
        return {kd: float(max(0.0, ex[:, :, [p for p, q in enumerate(self.kinds) if q == kd]].max()))
                for kd in sorted(set(self.kinds))}

    def ratio(self, got, extra=0.0, c1=None):
        """Worst error / gate and where (i, j, p); an error where the gate is 0 counts as infinite."""
        err, gate = self.error_abs(got), self.gate_abs(extra, c1)
        r = np.where(err > 0, err / np.where(gate > 0, gate, 1.0), 0.0)
        r = np.where((err > 0) & (gate == 0), np.inf, r)
        at = np.unravel_index(int(np.argmax(r)), r.shape)
        return float(r[at]), tuple(int(v) for v in at)

    def dead(self):
        """[n1, n2, nc]: where the gate is 0 -- the unit and the carried allowance both: the v components of a zero row in a
        bias-free network, which must be exact zeros.  (Exactly antiparallel rows of a bias-free network have unit 0 too, K = 0
        there, but not gate 0: the arctangent's own allowance C0 |k| / 2 pi remains.)"""
        return self.mask[:, :, None] & (self.gate_abs() == 0.0)


_BLOCKS = {}


def block(family, kind, net, extras=(0.0,)):
    """Cached (x1, x2, Block) of a rectangular block kind of angle_reference (family d64: d16 padded to 64 features)."""
    key = (family, kind, net.key())
    hit = _BLOCKS.get(key)
    if hit is None or not set(extras) <= set(hit[2].extras):
        x1, x2 = block_rows(family, kind)
        hit = _BLOCKS[key] = (x1, x2, Block(x1, x2, net, extras=extras))
    return hit


# ------------------------------------------------------------------------------------- the symmetric pass at n = 2 (referee)
def pair_rows(family, medium=True):
    """(anchor row (R, 0), the sweep's rows) for the n = 2 problems: equal norms up to the rounding of the integer rows, so the
    off-diagonal entry weighs like the diagonal ones in both halves."""
    anchor = A.embed(family, A.anchors_ab(family, True)[:1])
    return anchor[0], A.embed(family, A.sweep_ab(family, medium))


class Pair:
    """Referee of quad_p = alpha^T dK_p alpha (per right-hand side) and trace_p = tr(A^-1 dK_p) of A = K + lambda I on the rows
    (x0, x1), lambda = K_00 rounded to float64 (absolute), with their gates
        sum_ij |S_ij| gate_ij + calpha u sum_ij |S_ij dK_ij|,      gate_ii = C1d unit_ii  (the exact diagonal),
    and cond(A).  off: the off-diagonal entry as entry() returned it for (x0, x1), where a block already holds it.  n_zero: the pair stands in a larger problem whose other n_zero rows are zero rows with y = 0 -- they decouple
    exactly (alpha_z = 0, A^-1_zz = 1 / lambda, every other seed an exact 0), so the trace gains n_zero dK_zz,p / lambda (not 0
    for the bias components, even of a bias-free network)."""

    RHS = ((1.0, 1.0), (1.0, -1.0))

    def __init__(self, x0, x1, net, ard=False, n_zero=0, off=None):
        x = np.stack([np.asarray(x0, np.float64), np.asarray(x1, np.float64)])
        self.x, self.net = x, net
        d = x.shape[1]
        k, q, _ = A.gram(x, x)
        self.kinds = kinds(net, d if ard else 0)
        nc = len(self.kinds)
        c1 = np.array([CONSTANTS[net.family][kd] for kd in self.kinds])
        kf, dk = [[None, None], [None, None]], [[None, None], [None, None]]
        gate = np.zeros((2, 2, nc))
        for i, j in ((0, 0), (1, 0), (1, 1)):
            s0 = [(x[i, f] * x[j, f] / d, x[i, f] ** 2 / d, x[j, f] ** 2 / d) for f in range(d if ard else 0)]
            kk, tt, un, carry = off if (off is not None and i != j) else entry(k[i, j], q[i], q[j], net, exact_diag=i == j, s0=s0)
            kf[i][j] = kf[j][i] = kk
            dk[i][j] = dk[j][i] = tt
            gate[i, j] = gate[j, i] = c1 * np.array(un) + np.array(carry[0.0])
        self.lam = float(kf[0][0])
        lam = mp.mpf(self.lam)
        a, b, c = kf[0][0] + lam, kf[0][1], kf[1][1] + lam
        det = a * c - b * b
        self.ainv = [[c / det, -b / det], [-b / det, a / det]]
        half = mp.sqrt((a - c) ** 2 / 4 + b * b)
        self.cond = float(((a + c) / 2 + half) / ((a + c) / 2 - half))
        self.kf, self.dk = kf, dk
        seeds = {"trace": self.ainv}
        for y in self.RHS:
            al = [self.ainv[0][0] * y[0] + self.ainv[0][1] * y[1], self.ainv[1][0] * y[0] + self.ainv[1][1] * y[1]]
            seeds[y] = [[al[i] * al[j] for j in range(2)] for i in range(2)]
        self.seeds = seeds
        zz = None
        if n_zero:
            s0 = [(0.0, 0.0, 0.0)] * (d if ard else 0)
            _, tz, uz, _ = entry(0.0, 0.0, 0.0, net, exact_diag=True, s0=s0)
            zz = (n_zero / lam, tz, c1 * np.array(uz))
        ij = [(0, 0), (0, 1), (1, 0), (1, 1)]
        self.want, self.gate, self.mass = {}, {}, {}
        for key, s in seeds.items():
            want = [sum(s[i][j] * dk[i][j][p] for i, j in ij) for p in range(nc)]
            mass = [sum(abs(s[i][j] * dk[i][j][p]) for i, j in ij) for p in range(nc)]
            g = np.array([float(sum(abs(s[i][j]) * gate[i, j, p] for i, j in ij)) for p in range(nc)])
            if zz is not None and key == "trace":
                want = [w + zz[0] * t for w, t in zip(want, zz[1])]
                mass = [m + abs(zz[0] * t) for m, t in zip(mass, zz[1])]
                g = g + float(zz[0]) * zz[2]
            self.want[key], self.mass[key] = want, np.array([float(m) for m in mass])
            self.gate[key] = g + CONSTANTS["calpha"] * U * self.mass[key]

    def error(self, key, got):
        """|got_p - referee| per component for key = "trace" or a right-hand side."""
        return np.array([float(abs(mp.mpf(float(g)) - w)) for g, w in zip(got, self.want[key])])


_PAIRS = {}


def pairs(family, net, ard=False, every=1):
    """Cached [Pair] of the anchor (R, 0) with every sweep row of the family (every: thinning of the sweep)."""
    key = (family, net.key(), ard, every)
    if key not in _PAIRS:
        x0, xs = pair_rows(family)
        raw = {}
        if not ard:  # the off-diagonal entry of pair j is entry (0, j) of the block "one" (K and its tangents are symmetric)
            x1, x2, blk = block(family, "one", net)
            assert np.array_equal(x1[0], x0) and np.array_equal(x2, xs)
            raw = blk.raw
        _PAIRS[key] = [Pair(x0, xs[j], net, ard=ard, off=raw.get((0, j))) for j in range(0, len(xs), every)]
    return _PAIRS[key]


def numpy_pair(pair, kf64):
    """The float64 NumPy solve of a Pair's systems on the float64 kernel kf64 [2, 2], contracted with the referee's own dK: the
    error of the solve alone, in units of u sum |S_ij dK_ij| (what calpha is 4 x of)."""
    a = np.array(kf64, dtype=np.float64) + pair.lam * np.eye(2)
    ainv = np.linalg.solve(a, np.eye(2))
    worst = 0.0
    for key in pair.want:
        if key == "trace":
            s = ainv
        else:
            al = np.linalg.solve(a, np.array(key))
            s = np.outer(al, al)
        for p, w in enumerate(pair.want[key]):
            got = sum(mp.mpf(float(s[i, j])) * pair.dk[i][j][p] for i in range(2) for j in range(2))
            if pair.mass[key][p] > 0:
                worst = max(worst, float(abs(got - w)) / (U * pair.mass[key][p]))
    return worst


# ------------------------------------------------------------------------------------------------------- host restatement
def _ap(spec):
    """(a b, (b - a)^2, (a^2 + b^2) / 2) as float64, formed as csrc/api.hip forms them."""
    if spec[0] == "relu":
        return 0.0, 1.0, 0.5
    a, b = float(spec[1]), float(spec[2])
    return a * b, (b - a) * (b - a), 0.5 * (a * a + b * b)


def device_adjoint(k, q1, q2, net, tab, diag=None, shift=0, swap=False):
    """rect_tile (diag None) / adjoint_tile (diag: mask of the exact diagonal) per entry with seed 1: (dK / dtheta_p [n1, n2, 2 nd],
    (kbar, q1bar, q2bar) at the input of Dense layer 0, table indices per hidden layer).  shift: added to the table index;
    swap: t1 and t2 exchanged in the qbar updates (the two mutations the host test shows to be noticed)."""
    fma = A.fma
    k = np.array(k, dtype=np.float64)
    shape = k.shape
    nd = net.nd
    relu = [sp[0] == "relu" for sp in net.acts]
    ap = [_ap(sp) for sp in net.acts]
    # the q chain of the rows and the columns
    qs, rq = [], []
    for q in (np.asarray(q1, np.float64), np.asarray(q2, np.float64)):
        q = q.copy()
        qs_l, rq_l = [], []
        for l in range(nd):
            qs_l.append(q)
            qp = fma(net.w2[l], q, net.b2[l])
            with np.errstate(divide="ignore"):
                rq_l.append(np.where(qp > 0.0, 1.0 / ((4.0 * math.pi) * np.where(qp > 0.0, qp, 1.0)), 0.0))
            if l < nd - 1:
                q = (0.5 if relu[l] else ap[l][2]) * qp
        qs.append(qs_l)
        rq.append(rq_l)
    row = lambda a: np.broadcast_to(a[:, None], shape)  # noqa: E731
    col = lambda a: np.broadcast_to(a[None, :], shape)  # noqa: E731
    dg = np.zeros(shape, dtype=bool) if diag is None else diag
    k = np.where(dg, row(qs[0][0]), k)
    kin, ck, cs, idxs = [], [], [], []
    for l in range(nd):
        kin.append(k)
        if l < nd - 1:
            v, c = net.w2[l], net.b2[l]
            k = fma(v, k, c)
            hh = 0.5 if relu[l] else ap[l][2]
            qa, qb = fma(v, row(qs[0][l]), c), fma(v, col(qs[1][l]), c)
            rr = np.where(dg, 0.0, fma(qa, qb, -k * k))
            s = A._sqrt_or_zero(rr)
            pmt, idx, _ = A.pi_minus_atan2(s, k, tab, shift)
            kr = pmt * (0.5 / math.pi)
            kk = fma(kr, k, s * (0.5 / math.pi))
            if relu[l]:
                kn, ckl, csl = kk, kr, s
            else:
                kn, ckl, csl = fma(ap[l][0], k, ap[l][1] * kk), fma(ap[l][1], kr, ap[l][0]), ap[l][1] * s
            k = np.where(dg, k * hh, kn)
            ck.append(np.where(dg, hh, ckl))
            cs.append(np.where(dg, 0.0, csl))
            idxs.append(idx)
    kb = np.ones(shape)
    qa1, qa2 = np.zeros(shape), np.zeros(shape)
    out = np.zeros(shape + (2 * nd,))
    for l in range(nd - 1, -1, -1):
        if l < nd - 1:
            hh = 0.5 if relu[l] else ap[l][2]
            t1, t2 = cs[l] * row(rq[0][l]), cs[l] * col(rq[1][l])
            if swap:
                t1, t2 = t2, t1
            qa1 = fma(kb, t1, hh * qa1)
            qa2 = fma(kb, t2, hh * qa2)
            kb = kb * ck[l]
        x1, x2 = row(qs[0][l]), col(qs[1][l])
        out[..., 2 * l] = fma(kb, kin[l], fma(qa1, x1, qa2 * x2))
        out[..., 2 * l + 1] = (kb + qa1) + qa2
        v = net.w2[l]
        kb, qa1, qa2 = kb * v, qa1 * v, qa2 * v
    return out, (kb, qa1, qa2), idxs


def float64_tangents(x1, x2, net, sym=False):
    """The suite's float64 forward-mode references on a block, all components [n1, n2, 2 nd]: sparse_evidence_reference.kernel_rect
    (rectangular, no diagonal rule) or nngp_mll_reference.kernel_block (symmetric, exact diagonal)."""
    import nngp_mll_reference as MR
    import sparse_evidence_reference as SE
    acts = [tuple(a) for a in net.acts]
    out = []
    for p in range(2 * net.nd):
        if sym:
            out.append(MR.kernel_block(x1, slice(None), net.w2, net.b2, acts, param=p)[1])
        else:
            out.append(SE.kernel_rect(x1, x2, net.w2, net.b2, acts, param=p)[1])
    return np.stack(out, axis=2)
