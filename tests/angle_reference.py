"""Inputs, referee, gate and host restatement for the kernel build over the whole angle range (test infrastructure, no tests).

Everything a kernel-matrix entry goes through on the device -- pi_minus_atan2 with its 65-entry rotation table (csrc/f64_math.h,
csrc/trig_tab.h), fast_sqrt_pos / fast_rcp, the composite ReLU map of kernel_build.hip -- is a function of the ANGLE of a pair of
rows.  This module makes rows whose pair angles are known and cover [0, pi] with every table seam and every interval boundary
approached from both sides, evaluates the layer recursion on them in mpmath (the referee), derives a per-entry gate from the
referee alone, and restates the device arithmetic in NumPy as a diagnostic and a coverage counter.

Inputs.  Integer coordinates, rows of squared norm < 2^51 and d a power of two: every product, every partial Gram sum in any
order (|sum| <= |x| |x'| < 2^51 by Cauchy-Schwarz) and the division by d are exact in float64, so the referee and the device start
from the same k, q, q'.  Family "d2": x = (rint(R cos phi), rint(R sin phi)), R = 2^20.  Family "d16": the same sweep
(R = 2^18) in the plane of E1 = 7 (3, -4, 12) and E2 = 13 (-2, 3, 6) on disjoint coordinates of R^16 (|E1| = |E2| = 91,
E1 . E2 = 0), so the angle of two rows is the angle of their (a, b) pairs while the Gram walks sign-mixed columns.

Referee.  mpmath at 40 digits from the float64 inputs (and the float64 w_std^2, b_std^2 the library forms) taken as exact
rationals: theta = atan2(sqrt(q q' - k^2), k) per ReLU / ABRelu layer, atan2(u, w) per Erf layer, the formulas of
tests/activation_reference.py.

Gate (per entry, from the referee alone; u = 2^-53).  A ReLU-like layer forms rr = q q' - k^2 and s = sqrt(rr); an error E in
rr moves s by ds(E) = max(sqrt(s^2 + E) - s, s - sqrt(max(s^2 - E, 0)))  (E / 2s to first order, sqrt(E) at s = 0: exact duplicates
need no rule of their own) and the angle by |k| ds / rho^2, rho^2 = q q'.  Layer l has the angle allowance
    d_theta_l = C0 + |k| ds(E_l) / rho^2,      E_l = u (k^2 + 2 ek_l |k| rho + (eq_l + eq'_l) rho^2)
from that layer's k, s, rho in the referee.  u k^2 is the one rounding of k k in the kernel's rr = fma(q, q', -(k k)): on exact
inputs (the first layer behind an exact Dense layer: ek = eq = 0) that is d_theta = C0 + u |k|^3 / (2 s rho^2) to first order.
ek_l (in units of u rho) and eq_l (relative) count the roundings an unfused float64 evaluation has put into k and into q, q'
before layer l: per Dense layer 2 with a bias, 1 without, 0 when also w_std^2 is a power of two (the layer is exact); per
ReLU-like layer 5 on k ((pi - theta) / 2 pi: two roundings of a factor <= 1/2 times |k| <= rho = 2 rho_out; s / 2 pi: two
roundings of <= rho / 2 pi; the product and the sum).  Without the counts the allowance does not hold beyond the first layer:
there k, q, q' are computed numbers whose last-digit errors are divided by s exactly as the rounding of k k is, and after every
ReLU the angles are smaller.  Measured with E_l = u k^2 at every layer: the restatement of the device arithmetic below misses the
gate on the NTK of 3 bias-free ReLU layers by 2.2e-12 of scale (error 8.7e-12, allowance 6.5e-12, nearly parallel rows), and with
biases on 2 and 4 layers by up to 5e-14; with the counts it and the float64 oracle are inside everywhere.
The float64 oracle also rounds the product q q' (numpy.outer), so IT is held to E_l + u rho^2 ("extra = 1"): against the
kernel's own E the oracle's first-layer angle is off by up to 2.3e-11 rad on these inputs, against its own by 3.4e-16.  A device
result is only ever held to extra = 0.
An Erf layer (first hidden layer only) has psi = atan2(u, w), u = 2 b^2 k, w^2 = r = 1 + 2 b^2 (q + q') + 4 b^4 (q q' - k^2).  Its
inputs are exact before the Dense layer, which puts dc roundings (2 with a bias, 1 without, 0 when also w_std^2 is a power of
two) into each of k, q, q': |d(q q' - k^2)| <= 4 dc u rho^2, the bracket and the sums add (dc + 3) u r, so
    dw / w = (4 b^4 4 dc u rho^2 + (dc + 3) u r) / 2 r,     d_psi = C0 + (|u| w / (u^2 + w^2)) ((dc + 2) u + dw / w),
and kdot = a^2 (4 / pi) b^2 / w moves by the same dw / w.  (At raw norms and nearly parallel rows 4 b^4 rho^2 / r is large: Erf
behind an inexact Dense layer is ill conditioned there and any float64 evaluation shows it; with w_std = 1, b_std = 0 it is not.)
The value allowance of an entry is then
    |dK| <= scale (C1 + sum over hidden layers l of |K(theta_l +- d_theta_l) - K| / scale),
each difference taken by re-evaluating the remaining layers in the referee at the perturbed angle (so the NTK and kdot, first
order in theta, get what they need and the NNGP value, second order, does not), scale = sqrt(K_ii K_jj) of the same output.
The exact diagonal of a symmetric build has theta = 0 by construction on the device and d_theta = 0 here.
C0 and C1 are in CONSTANTS below; how they were measured is in the module docstring of tests/test_gpu_kernel_angles.py.

Host restatement.  pi_minus_atan2, fast_rcp, fast_sqrt_pos, the per-layer ReLU recursion of k_build_mfma and the composite map
(comp_build_host / comp_exact on numpy.longdouble, Horner with the kernel's interval selection), step for step: float32 where
the device is float32, one rounding per fma (two_prod + two_sum: exact but for ties beyond 2^-100).  The hardware seeds
(v_rcp_f64, v_rsq_f64) are restated as the exact value rounded to 24 bits.  It is never what a device result is accepted against.
"""
from __future__ import annotations

import functools
import math
import os
import re

import mpmath as mp
import numpy as np

mp.mp.dps = 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIG_TAB_H = os.path.join(ROOT, "nngp-src_amd", "csrc", "trig_tab.h")
U = 2.0 ** -53
NT = 64          # rotation table: entries 0..NT, a_i = i pi / NT
COMP_NI, COMP_DEG = 16, 10
COMP_LIMIT = 4e-16

# C0: angle allowance (rad); C1[family][output]: value allowance in units of scale.  C0 = 4 x the larger of the restatement's
# (5.2e-16) and the oracle's (3.4e-16) first-layer angle error beyond the cancellation term.  C1 = 4 x the larger of the two's
# value error beyond the carried angle allowance, and not below 4 u (the last fma of the layer and the Dense layer round once
# each whatever the angle).  Both far below the 3e-14 of scale the suite already asks of NNGP entries.  The measured figures are
# in the module docstring of tests/test_gpu_kernel_angles.py; tests/test_angle_math_host.py prints them.
CONSTANTS = {
    "c0": 2.1e-15,
    "relu": {"nngp": 6.6e-16, "ntk": 4.4e-16},     # beyond the carried allowance: 1.64e-16, 1.04e-16
    "abrelu": {"nngp": 6.8e-16, "ntk": 4.4e-16},   # 1.69e-16, 8.5e-17
    "erf": {"nngp": 4.4e-16, "ntk": 4.4e-16},      # 0 (2.2e-16 before the allowance), 5e-21
}


ACTS = {"erf": ("erf", 1.0, 1.0, 0.0), "erf_abc": ("erf", 0.8, 1.7, 0.3), "leaky": ("abrelu", 0.1, 1.0), "abs": ("abrelu", -1.0, 1.0)}


def cases():
    """name -> (Net, [(family, block kind)], outputs): what the host file holds the oracle and the restatement to and the GPU
    file the device.  comp*: bias-free, NNGP only -- the composite map where its table is accepted."""
    both, few = ("nngp", "ntk"), [("d2", "few"), ("d16", "few")]
    out = {
        "relu1": (relu_net(1), [("d2", "anchors"), ("d2", "ends"), ("d16", "anchors"), ("d16", "ends"), ("d2", "sym"), ("d16", "sym")], both),
        "relu2_bias": (relu_net(2, 1.4, 0.25), few, both),
        "relu4_bias": (relu_net(4, 1.4, 0.25), few, both),
        "relu3_ntk": (relu_net(3), few, both),
        "comp2": (relu_net(2), [("d2", "few"), ("d2", "sym")], ("nngp",)),
        "comp3": (relu_net(3, 1.3), few, ("nngp",)),
        "comp4": (relu_net(4, 0.8), [("d2", "few")], ("nngp",)),
        "comp7": (relu_net(7), [("d2", "one")], ("nngp",)),
        "comp8": (relu_net(8), [("d2", "one")], ("nngp",)),
        "comp12": (relu_net(12), [("d2", "one")], ("nngp",)),
        "erf": (Net([1.0, 1.0], [0.0, 0.0], [ACTS["erf"]]), [("d2", "few")], both),
        "erf_abc": (Net([1.1, 1.1], [0.3, 0.3], [ACTS["erf_abc"]]), [("d2", "few")], both),
        "leaky": (Net([1.1, 1.1], [0.3, 0.3], [ACTS["leaky"]]), [("d2", "few")], both),
        "abs": (Net([1.1, 1.1], [0.0, 0.0], [ACTS["abs"]]), [("d16", "few")], both),
    }
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def _e16():
    e1, e2 = np.zeros(16), np.zeros(16)
    e1[[0, 5, 10]] = 7.0 * np.array([3.0, -4.0, 12.0])
    e2[[3, 7, 15]] = 13.0 * np.array([-2.0, 3.0, 6.0])
    return e1, e2


FAMILIES = {"d2": (2, 2 ** 20), "d16": (16, 2 ** 18)}


def embed(family, ab):
    """Integer (a, b) pairs [n, 2] -> rows of the family [n, d]."""
    ab = np.asarray(ab, dtype=np.float64).reshape(-1, 2)
    assert np.all(ab == np.rint(ab))
    if family == "d2":
        return ab.copy()
    e1, e2 = _e16()
    return ab[:, :1] * e1[None, :] + ab[:, 1:] * e2[None, :]


def plane_angle(ab1, ab2):
    """Exact-input pair angles [n1, n2] of (a, b) pairs in float64 through atan2(cross, dot) (no cancellation): the coverage
    counter's and the tags' notion of the angle (the referee computes its own)."""
    a1, a2 = np.asarray(ab1, np.float64).reshape(-1, 2), np.asarray(ab2, np.float64).reshape(-1, 2)
    dot = a1[:, None, 0] * a2[None, :, 0] + a1[:, None, 1] * a2[None, :, 1]
    crs = a1[:, None, 0] * a2[None, :, 1] - a1[:, None, 1] * a2[None, :, 0]
    return np.arctan2(np.abs(crs), dot)


def seam_angles():
    return [(i + 0.5) * math.pi / NT for i in range(NT)]


def boundary_angles():
    return [i * math.pi / COMP_NI for i in range(1, COMP_NI)]


def sweep_phis(family, medium=False):
    """The sweep's directions: a uniform grid over [0, pi], every table seam and every composite boundary from both sides
    (eps = 8 / R, the family's angular resolution; 2e-3 and, for the seams, 6e-3: the float32 estimate that picks the
    table entry is good to 5e-3, so the entry really changes somewhere within 5e-3 of a seam), the ends.  medium: every 8th grid point (the multi-layer
    and deep cases); seams, boundaries and ends stay."""
    r = FAMILIES[family][1]
    eps = 8.0 / r
    grid = np.linspace(0.0, math.pi, 2049)[:: 8 if medium else 1]
    seams = [s + o for s in seam_angles() for o in (-6e-3, -2e-3, -eps, eps, 2e-3, 6e-3)]
    bounds = [b + o for b in boundary_angles() for o in (-1e-3, -eps, eps, 1e-3)]
    ends = [e for v in (1e-6, 1e-5, 1e-4, 1e-3) for e in (v, math.pi - v)]
    return np.concatenate([grid, seams, bounds, ends])


def sweep_ab(family, medium=False):
    """(a, b) integer pairs of the sweep, plus a zero row and an exact duplicate of the first row (phi = 0) at the end."""
    r = FAMILIES[family][1]
    phi = sweep_phis(family, medium)
    ab = np.stack([np.rint(r * np.cos(phi)), np.rint(r * np.sin(phi))], axis=1)
    return np.concatenate([ab, [[0.0, 0.0]], ab[:1]])


def anchors_ab(family, few=False):
    """The other row of each pair: several directions, radii 3 .. 2^25, a zero row.  few: three anchors (the multi-layer and
    deep cases): direction 0 at the sweep's radius (theta = phi: every angle, an exact duplicate at phi = 0, exactly antiparallel
    at phi = pi), direction pi at radius 3, and (-5, 12)."""
    r = FAMILIES[family][1]
    if few:
        return np.array([[r, 0], [-3, 0], [-5, 12]], dtype=np.float64)
    if family == "d16":  # |row| = 91 |(a, b)|
        return np.array([[r, 0], [3, 0], [-r, 0], [0, r], [-5, 12], [3 * 2 ** 16, 4 * 2 ** 16], [0, 0]], dtype=np.float64)
    big = 2 ** 25
    return np.array([[3, 0], [2 ** 10, 0], [r, 0], [big, 0], [-3, 0], [-big, 0], [0, r], [3 * 2 ** 18, 4 * 2 ** 18], [-5, 12], [0, 0]],
                    dtype=np.float64)


def end_anchors_ab(family):
    """Rows 9e-8 .. 1e-3 rad off direction 0 and off direction pi, at the largest radius: against the ends of the sweep they make
    the angles next to 0 and next to pi that the sweep's own resolution (1 / R) cannot."""
    r = FAMILIES[family][1]
    if family == "d16":
        return np.array([[sg * r, m] for sg in (1, -1) for m in (3, 26, 262)], dtype=np.float64)  # 1e-5, 1e-4, 1e-3
    return np.array([[sg * 2 ** 25, m] for sg in (1, -1) for m in (3, 336, 33554)], dtype=np.float64)  # 9e-8, 1e-5, 1e-3


def symmetric_ab(family):
    """Rows of the symmetric build: every 32nd grid direction, both sides of every 4th seam, a zero row, a duplicate (99 rows,
    two tiles a side: diagonal tiles, an off-diagonal tile and its mirror image)."""
    r = FAMILIES[family][1]
    eps = 8.0 / r
    phi = np.concatenate([np.linspace(0.0, math.pi, 2049)[::32], [s + o for s in seam_angles()[::4] for o in (-eps, eps)]])
    ab = np.stack([np.rint(r * np.cos(phi)), np.rint(r * np.sin(phi))], axis=1)
    return np.concatenate([ab, [[0.0, 0.0]], ab[5:6]])


def gram(x1, x2):
    """(k [n1, n2], q1, q2) in float64, asserted exact against integer arithmetic."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    d = x1.shape[1]
    assert d & (d - 1) == 0
    k, q1, q2 = x1 @ x2.T / d, np.sum(x1 * x1, axis=1) / d, np.sum(x2 * x2, axis=1) / d
    i1, i2 = x1.astype(np.int64).astype(object), x2.astype(np.int64).astype(object)
    assert np.all(i1.astype(np.float64) == x1) and np.all(i2.astype(np.float64) == x2)
    assert max(np.sum(x1 * x1, axis=1).max(), np.sum(x2 * x2, axis=1).max()) < 2.0 ** 51  # any partial sum, in any order, is exact
    assert np.all((i1 @ i2.T) == (k * d).astype(np.int64).astype(object)) and np.all(k * d == np.rint(k * d))
    assert np.all((i1 * i1).sum(axis=1) == (q1 * d).astype(np.int64).astype(object))
    assert np.all((i2 * i2).sum(axis=1) == (q2 * d).astype(np.int64).astype(object))
    return k, q1, q2


# ------------------------------------------------------------------------------------------------------------------ referee
class Net:
    """Dense,(act,Dense)*: w2 / b2 as the float64 squares the library forms, acts per hidden layer as in activation_reference."""

    def __init__(self, w_std, b_std, acts=None):
        self.w_std, self.b_std = [float(v) for v in w_std], [float(v) for v in b_std]
        self.w2, self.b2 = [v * v for v in self.w_std], [v * v for v in self.b_std]
        self.nd = len(self.w2)
        self.mw2, self.mb2 = [mp.mpf(v) for v in self.w2], [mp.mpf(v) for v in self.b2]
        self.acts = [tuple(a) for a in (acts or [("relu",)] * (self.nd - 1))]
        assert len(self.b2) == self.nd and len(self.acts) == self.nd - 1
        kinds = {a[0] for a in self.acts}
        self.family = "erf" if "erf" in kinds else ("abrelu" if "abrelu" in kinds else "relu")

    def key(self):
        return (tuple(self.w_std), tuple(self.b_std), tuple(self.acts))


def relu_net(n_relu, w=1.0, b=0.0):
    return Net([w] * (n_relu + 1), [b] * (n_relu + 1))


_PI = mp.pi


def _act(spec, k, q1, q2, dth, dw=0):
    """One hidden layer in mpmath on (k, q1, q2) after its Dense layer, its angle moved by dth (None: not at all) and, for
    Erf, w scaled by 1 / (1 + dw) in kdot.  Returns (K', kdot, q1', q2', (kind, angle data for the gate))."""
    if spec[0] == "erf":
        a, b, c = (mp.mpf(v) for v in spec[1:])
        bb = 2 * b * b
        u = bb * k
        rho2 = q1 * q2
        r = 1 + bb * (q1 + q2) + bb * bb * (rho2 - k * k)
        w = mp.sqrt(r)
        psi = mp.atan2(u, w)
        info = ("erf", u, w, r, rho2, bb)
        amp = a * a * 2 / _PI
        kd = amp * bb / w
        if dth is not None:
            psi, kd = psi + dth, kd * (1 + dw)

        def qn(q):
            return amp * mp.asin(bb * q / (1 + bb * q)) + c * c
        return amp * psi + c * c, kd, qn(q1), qn(q2), info
    rho2 = q1 * q2
    rr = rho2 - k * k
    s = mp.sqrt(rr) if rr > 0 else mp.mpf(0)
    th = _PI / 2 if (s == 0 and k == 0) else mp.atan2(s, k)
    info = ("relu", k, s, rho2)
    if dth is not None:
        th = min(max(th + dth, mp.mpf(0)), +_PI)
        rho = mp.sqrt(rho2)
        k, s = rho * mp.cos(th), rho * mp.sin(th)
    kd = (_PI - th) / (2 * _PI)
    kr = s / (2 * _PI) + kd * k
    if spec[0] == "abrelu":
        a, b = mp.mpf(spec[1]), mp.mpf(spec[2])
        return a * b * k + (b - a) ** 2 * kr, a * b + (b - a) ** 2 * kd, (a * a + b * b) / 2 * q1, (a * a + b * b) / 2 * q2, info
    return kr, kd, q1 / 2, q2 / 2, info


def _run(state, net, l0, dth=None, dw=0, trace=None):
    """Layers l0 .. of the recursion from state = (k, q1, q2, t) before Dense layer l0; dth (dw) move hidden layer l0's angle."""
    k, q1, q2, t = state
    for l in range(l0, net.nd):
        if trace is not None:
            trace.append((k, q1, q2, t))
        w2, b2 = net.mw2[l], net.mb2[l]
        k, q1, q2 = w2 * k + b2, w2 * q1 + b2, w2 * q2 + b2
        t = w2 * t + k
        if l < net.nd - 1:
            k, kd, q1, q2, info = _act(net.acts[l], k, q1, q2, dth if l == l0 else None, dw)
            t = kd * t
            if trace is not None:
                trace[-1] = trace[-1] + (info,)
    return k, t


def _is_pow2(v):
    return v > 0.0 and math.frexp(v)[0] == 0.5


def _dense_count(net, l):
    """Roundings of an unfused Dense layer w2 v + b2 (0: the layer is exact)."""
    if net.b2[l] != 0.0:
        return 2
    return 0 if _is_pow2(net.w2[l]) else 1


def _ds(s, e):
    up = mp.sqrt(s * s + e) - s
    dn = s - mp.sqrt(max(s * s - e, mp.mpf(0)))
    return max(up, dn)


def _mpf(v):
    return v if isinstance(v, mp.mpf) else mp.mpf(float(v))


def entry(k, q1, q2, net, c0, exact_diag=False, extras=(0.0,), initial=0, kk_exact=False):
    """One entry from float64 (k, q1, q2): (K, T, [gK per extra], [gT per extra]) -- the referee's values and the carried
    angle allowances (absolute, without C1).  extras: further roundings of rr in units of u rho^2 (1: an unfused q q' product,
    the float64 oracle's; 0: the gate a device result is held to).
    For the additive build (tests/additive_angle_reference.py; the defaults leave every other caller's numbers as they were):
    k, q1, q2 may be mpmath numbers -- the exact rationals S / width of a slice whose width is no power of two -- and initial
    counts the roundings the device has put into each of them before the first Dense layer (2: the rounded reciprocal and the
    product with it; a count of operations in the code, not a measurement).  kk_exact: leave the term u k^2 out of E where it
    stands for nothing -- the first layer behind an exact Dense layer on exact inputs, when k k is a float64 number, so that
    fma(q, q', -(k k)) rounds once, the exact bracket (exactly collinear small integers: E = 0, theta = 0 or pi exactly)."""
    state = (_mpf(k), _mpf(q1), _mpf(q2), mp.mpf(0))
    if exact_diag:
        state = (state[1], state[1], state[1], mp.mpf(0))
    trace = []
    kk, tt = _run(state, net, 0, trace=trace)
    gk, gt = [mp.mpf(0)] * len(extras), [mp.mpf(0)] * len(extras)
    if exact_diag:
        return kk, tt, gk, gt
    ek = eq = initial  # roundings carried by k (units of u rho) and by q, q' (relative) into layer l
    for l in range(net.nd - 1):
        info = trace[l][4]
        ek, eq = ek + _dense_count(net, l), eq + _dense_count(net, l)
        for x, extra in enumerate(extras):
            dw = 0
            if info[0] == "erf":
                assert l == 0, "the Erf allowance counts the roundings of one Dense layer on exact inputs"
                _, u, w, r, rho2, bb = info
                dc = _dense_count(net, l) + initial
                dw = (bb * bb * 4 * dc * U * rho2 + (dc + 3) * U * r) / (2 * r)
                dth = c0 + abs(u) * w / (u * u + w * w) * ((dc + 2) * U + dw)
                if x > 0:  # nothing of the extras applies to an Erf layer
                    gk[x], gt[x] = gk[x] + dk, gt[x] + dt
                    continue
            else:
                _, kl, sl, rho2 = info
                dth = mp.mpf(c0)
                if rho2 > 0:
                    k2r = kl * kl  # the rounding of k k
                    if kk_exact and ek == 0 and eq == 0 and mp.mpf(float(kl)) == kl and mp.mpf(float(kl) * float(kl)) == k2r:
                        k2r = 0
                    e = U * (k2r + 2 * ek * abs(kl) * mp.sqrt(rho2) + (2 * eq + extra) * rho2)
                    dth = dth + abs(kl) * _ds(sl, e) / rho2
            dk = dt = mp.mpf(0)
            for sg in (1, -1):
                k2, t2 = _run(trace[l][:4], net, l, sg * dth, sg * dw)
                dk, dt = max(dk, abs(k2 - kk)), max(dt, abs(t2 - tt))
            gk[x], gt[x] = gk[x] + dk, gt[x] + dt
        ek += 5
    return kk, tt, gk, gt


class Block:
    """Referee and gate of a block x1 x x2^T (sym: x2 = x1, the exact diagonal, the lower triangle only)."""

    def __init__(self, x1, x2, net, sym=False, extras=(0.0,)):
        self.net, self.sym, self.extras = net, sym, tuple(extras)
        x2 = x1 if sym else x2
        self.k, self.q1, self.q2 = gram(x1, x2)
        n1, n2 = self.k.shape
        c0 = CONSTANTS["c0"]
        self.val = {g: [[None] * n2 for _ in range(n1)] for g in ("nngp", "ntk")}
        self.carry = {(g, e): np.zeros((n1, n2)) for g in ("nngp", "ntk") for e in self.extras}  # absolute
        self.mask = np.tril(np.ones((n1, n2), dtype=bool)) if sym else np.ones((n1, n2), dtype=bool)
        d1 = [entry(q, q, q, net, c0, exact_diag=True)[:2] for q in self.q1]
        d2 = d1 if sym else [entry(q, q, q, net, c0, exact_diag=True)[:2] for q in self.q2]
        self.scale = {g: np.array([[float(mp.sqrt(d1[i][e] * d2[j][e])) for j in range(n2)] for i in range(n1)])
                      for e, g in enumerate(("nngp", "ntk"))}
        for i, j in zip(*np.nonzero(self.mask)):
            kk, tt, gk, gt = entry(self.k[i, j], self.q1[i], self.q2[j], net, c0, exact_diag=sym and i == j, extras=self.extras)
            self.val["nngp"][i][j], self.val["ntk"][i][j] = kk, tt
            for g, v in (("nngp", gk), ("ntk", gt)):
                for e, ve in zip(self.extras, v):
                    self.carry[(g, e)][i, j] = float(ve)

    def error_abs(self, got, which):
        """|got - referee| per entry (0 outside the mask)."""
        got = np.asarray(got, dtype=np.float64)
        out = np.zeros(self.k.shape)
        for i, j in zip(*np.nonzero(self.mask)):
            out[i, j] = float(abs(mp.mpf(float(got[i, j])) - self.val[which][i][j]))
        return out

    def of_scale(self, a, which):
        """An absolute per-entry figure in units of scale (entries of scale 0 -- a zero row without biases -- left out)."""
        sc = self.scale[which]
        return np.where(self.mask & (sc > 0), a / np.where(sc > 0, sc, 1.0), 0.0)

    def gate_abs(self, which, extra=0.0, c1=None):
        """C1 scale + the carried angle allowance.  Where scale = 0 this is the carried allowance alone: 0 for a ReLU network
        (a zero row gives exact zeros), the arctangent's own for Erf (whose entries do not scale with the rows)."""
        c1 = CONSTANTS[self.net.family][which] if c1 is None else c1
        return c1 * self.scale[which] + self.carry[(which, extra)]

    def ratio(self, got, which, extra=0.0, c1=None):
        """Worst error / gate, where, and the error there in units of scale."""
        err, gate = self.error_abs(got, which), self.gate_abs(which, extra, c1)
        r = np.where(err > 0, err / np.where(gate > 0, gate, 1.0), 0.0)
        r = np.where(self.mask, np.where((err > 0) & (gate == 0), np.inf, r), 0.0)
        at = np.unravel_index(int(np.argmax(r)), r.shape)
        return float(r[at]), (int(at[0]), int(at[1]))


_BLOCKS = {}


def block_ab(family, kind):
    """(anchor (a, b) pairs, sweep (a, b) pairs) of a rectangular block kind."""
    if kind == "ends":
        s = sweep_ab(family)
        phi = np.arctan2(s[:, 1], s[:, 0])
        return end_anchors_ab(family), s[(phi < 0.01) | (phi > math.pi - 0.01)]
    few = kind in ("few", "one")
    return anchors_ab(family, few)[: 1 if kind == "one" else None], sweep_ab(family, few)


def block_rows(family, kind):
    a, s = block_ab(family, kind)
    return embed(family, a), embed(family, s)


def block(family, kind, net, extras=(0.0,)):
    """Cached (x1, x2, Block): kind "anchors" (anchors x sweep), "ends" (the end anchors x the sweep's rows within 0.01 of 0 and pi),
    "few" (three anchors x the medium sweep), "one" (the first of them alone: the deep networks), "sym" (x2 None)."""
    key = (family, kind, net.key())
    hit = _BLOCKS.get(key)
    if hit is None or not set(extras) <= set(hit[2].extras):
        if kind == "sym":
            x1, x2 = embed(family, symmetric_ab(family)), None
        else:
            x1, x2 = block_rows(family, kind)
        hit = _BLOCKS[key] = (x1, x2, Block(x1, x2, net, sym=kind == "sym", extras=extras))
    return hit


# ------------------------------------------------------------------------------------------------------- host restatement
def parse_trig_tab(path=TRIG_TAB_H):
    """The 65 x 4 hex literals of trig_tab.h as float64 [65, 4] (and the literals themselves)."""
    text = open(path).read()
    lits = re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+", text)
    assert len(lits) == (NT + 1) * 4, len(lits)
    return np.array([float.fromhex(v) for v in lits]).reshape(NT + 1, 4), lits


def _two_prod(a, b):
    p = a * b  # Dekker's split; the inputs here stay below 2^110, far from overflow
    sp = 134217729.0
    ah = a * sp; ah = ah - (ah - a); al = a - ah
    bh = b * sp; bh = bh - (bh - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """a b + c with one rounding: two_prod, two_sum, one more sum (exact but for ties beyond 2^-100)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def _round24(x):
    m, ex = np.frexp(x)
    return np.ldexp(np.rint(m * 2.0 ** 24) / 2.0 ** 24, ex)


def seed_rcp(x):
    return _round24(1.0 / x)


def seed_rsq(x):
    return _round24(1.0 / np.sqrt(x))


def fast_rcp(x):
    r = seed_rcp(x)
    return fma(r, fma(-x, r, 1.0), r)


def fast_sqrt_pos(r):
    y = seed_rsq(r)
    g, h = r * y, 0.5 * y
    e = fma(-h, g, 0.5)
    g = fma(g, e, g)
    h = fma(h, e, h)
    return fma(fma(-g, g, r), h, g)


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def pi_minus_atan2(s, k, tab, shift=0):
    """pi - atan2(s, k) as f64_math.h computes it; returns (pmt, table index, residual u).  shift: added to the index (the
    tests use it to show that a shifted index is noticed)."""
    s, k = np.broadcast_arrays(np.asarray(s, np.float64), np.asarray(k, np.float64))
    ak = np.abs(k)
    mx, mn = np.maximum(s, ak), np.minimum(s, ak)
    pos = mx > 0.0
    mxs = np.where(pos, mx, 1.0)
    t = np.where(pos, _f32(mn * seed_rcp(mxs)), np.float32(0.0)).astype(np.float32)
    c1, c2 = np.float32(-0.1919), np.float32(0.9724)
    tt = t * t
    inner = _f32(c1.astype(np.float64) * tt.astype(np.float64) + c2.astype(np.float64))  # fmaf: one rounding
    at = t * inner
    at = np.where(s > ak, np.float32(1.57079637) - at, at).astype(np.float32)
    at = np.where(k < 0.0, np.float32(3.14159274) - at, at).astype(np.float32)
    i = np.rint(at * np.float32(20.3718327)).astype(np.int64)
    i = np.clip(i, 0, NT)
    i = np.clip(i + shift, 0, NT)
    cx, cy = tab[i, 0], tab[i, 1]
    xp = fma(k, cx, s * cy)
    yp = fma(s, cx, -(k * cy))
    u = yp * fast_rcp(np.where(pos, xp, 1.0))
    w = u * u
    p = fma(w, 1.0 / 9.0, -1.0 / 7.0)
    p = fma(p, w, 1.0 / 5.0)
    p = fma(p, w, -1.0 / 3.0)
    atu = fma(u, p * w, u)
    pmt = tab[i, 3] - atu
    return np.where(pos, pmt, 0.5 * math.pi), i, np.where(pos, u, 0.0)


def _sqrt_or_zero(rr):
    return np.where(rr > 0.0, fast_sqrt_pos(np.where(rr > 0.0, rr, 1.0)), 0.0)


def device_relu(k, q1, q2, net, tab, diag=None, shift=0):
    """The per-layer ReLU recursion of k_build_mfma on float64 Gram entries k [n1, n2] (q1 rows, q2 columns; diag: mask of
    the exact diagonal).  Returns (K, T, stats) with stats = per ReLU layer (table index, |residual u|)."""
    assert net.family == "relu"
    k = np.array(k, dtype=np.float64)
    q1 = np.broadcast_to(np.asarray(q1, np.float64)[:, None], k.shape).copy()
    q2 = np.broadcast_to(np.asarray(q2, np.float64)[None, :], k.shape).copy()
    dg = np.zeros(k.shape, dtype=bool) if diag is None else diag
    k = np.where(dg, q1, k)
    t = np.zeros_like(k)
    stats = []
    for l in range(net.nd):
        w2, b2 = net.w2[l], net.b2[l]
        q2 = fma(w2, q2, b2)
        q1 = fma(w2, q1, b2)
        k = fma(w2, k, b2)
        t = fma(w2, t, k)
        if l < net.nd - 1:
            rr = np.where(dg, 0.0, fma(q1, q2, -(k * k)))
            s = _sqrt_or_zero(rr)
            pmt, idx, u = pi_minus_atan2(s, k, tab, shift)
            kd = np.where(dg, 0.5, pmt * (0.5 / math.pi))
            k = fma(kd, k, s * (0.5 / math.pi))
            t = t * kd
            stats.append((idx, np.abs(u)))
            q1 = q1 * 0.5
            q2 = q2 * 0.5
    return k, t, stats


def comp_exact(t, n_relu):
    """G(t) = F(pi - t): n_relu arc-cosine maps of the cosine, on numpy.longdouble (kernel_build.hip: comp_exact)."""
    ld = np.longdouble
    pi = ld(mp.nstr(mp.pi, 30))
    t = np.asarray(t, dtype=ld)
    th, c = pi - t, np.zeros_like(t)
    for l in range(n_relu):
        if l > 0:
            th = np.arccos(np.clip(c, ld(-1), ld(1)))
        c = (np.sin(th) + (pi - th) * np.cos(th)) / pi
    return c


@functools.lru_cache(maxsize=None)
def comp_table(n_relu):
    """Port of comp_build_host: (coefficients [16, 11] float64, worst check error, accepted)."""
    ld = np.longdouble
    pi = ld(mp.nstr(mp.pi, 30))
    dg = COMP_DEG
    tm = np.zeros((dg + 1, dg + 1), dtype=ld)
    tm[0, 0] = 1
    tm[1, 1] = 1
    for n in range(2, dg + 1):
        for kk in range(n + 1):
            tm[n, kk] = (2 * tm[n - 1, kk - 1] if kk > 0 else 0) - tm[n - 2, kk]
    coef = np.zeros((COMP_NI, dg + 1))
    worst = 0.0
    a = pi / (2 * COMP_NI)
    nodes = pi * (np.arange(dg + 1, dtype=ld) + ld(0.5)) / (dg + 1)
    for i in range(COMP_NI):
        m = (2 * i + 1) * a
        f = comp_exact(m + a * np.cos(nodes), n_relu)
        cheb = np.array([np.sum(f * np.cos(j * nodes)) * 2 / (dg + 1) for j in range(dg + 1)], dtype=ld)
        cheb[0] *= ld(0.5)
        mono = np.zeros(dg + 1, dtype=ld)
        for j in range(dg + 1):
            mono[: j + 1] += cheb[j] * tm[j, : j + 1]
        coef[i] = mono.astype(np.float64)
        u = -1.0 + np.arange(65) / 32.0
        p = np.full(65, coef[i, dg])
        for kk in range(dg - 1, -1, -1):
            p = fma(p, u, coef[i, kk])
        err = np.abs((p.astype(ld) - comp_exact(m + a * u.astype(ld), n_relu)).astype(np.float64))
        worst = max(worst, float(err.max()))
    return coef, worst, worst <= COMP_LIMIT


def device_composite(k, q1, q2, net, tab, diag=None, shift=0, coef=None):
    """The composite ReLU map of k_build_mfma<COMP> (bias-free, NNGP only).  Returns (K, stats) with stats = (table index,
    |residual u|, interval, composite u)."""
    n_relu = net.nd - 1
    assert net.family == "relu" and n_relu >= 2 and all(b == 0.0 for b in net.b2)
    coef = comp_table(n_relu)[0] if coef is None else coef
    amp = 1.0
    for w2 in net.w2:
        amp *= w2
    amp = math.ldexp(amp, -n_relu)
    k = np.array(k, dtype=np.float64)
    q1 = np.broadcast_to(np.asarray(q1, np.float64)[:, None], k.shape)
    q2 = np.broadcast_to(np.asarray(q2, np.float64)[None, :], k.shape)
    qq = q1 * q2
    rr = fma(q1, q2, -(k * k))
    sn = _sqrt_or_zero(rr)
    pmt, idx, ur = pi_minus_atan2(sn, k, tab, shift)
    iv = np.clip((pmt * (COMP_NI / math.pi)).astype(np.int64), 0, COMP_NI - 1)
    u = fma(pmt, 2.0 * COMP_NI / math.pi, -(2.0 * iv + 1.0))
    p = coef[iv, COMP_DEG]
    for e in range(COMP_DEG - 1, -1, -1):
        p = fma(p, u, coef[iv, e])
    rho = _sqrt_or_zero(qq)
    out = rho * (amp * p)
    if diag is not None:
        kd = q1.copy()
        for l in range(net.nd):
            kd = net.w2[l] * kd
            if l < net.nd - 1:
                kd = kd * 0.5
        out = np.where(diag, kd, out)
    return out, (idx, np.abs(ur), iv, u)


def oracle_theta(k, q1, q2):
    """The float64 oracle's first-layer angle (oracle/nngp_oracle.py: outer product, sqrt, arctan2)."""
    s = np.sqrt(np.maximum(np.outer(q1, q2) - k * k, 0.0))
    return np.where((s == 0.0) & (k == 0.0), math.pi / 2, np.arctan2(s, k))


# ------------------------------------------------------------------------------------------------------------ coverage
def coverage(family, ab1, ab2, shift=0):
    """What the pairs ab1 x ab2 of a family reach, counted by the restatement: (problems, figures).  problems is empty when
    every rotation-table entry and every composite interval is selected, every seam (i + 1/2) pi / 64 and every interior interval
    boundary i pi / 16 has pairs within 2 eps (eps = 8 / R) on both sides -- the seam's two entries both selected around it, the
    boundary's pairs in the right intervals with |u| next to 1 -- and the residual of the arctangent stays within the 0.03 rad its
    series is sized for, the composite variable within [-1, 1]."""
    tab, _ = parse_trig_tab()
    eps = 8.0 / FAMILIES[family][1]
    k, q1, q2 = gram(embed(family, ab1), embed(family, ab2))
    th = plane_angle(ab1, ab2)
    live = (q1[:, None] > 0) & (q2[None, :] > 0)
    _, _, stats = device_relu(k, q1, q2, relu_net(1), tab, shift=shift)
    idx, res = stats[0]
    _, (_, _, iv, cu) = device_composite(k, q1, q2, relu_net(2), tab, shift=shift)
    problems = []
    missing = sorted(set(range(NT + 1)) - set(np.unique(idx[live]).tolist()))
    if missing:
        problems.append("table entries never selected: %s" % missing)
    missing = sorted(set(range(COMP_NI)) - set(np.unique(iv[live]).tolist()))
    if missing:
        problems.append("composite intervals never selected: %s" % missing)
    for i, sm in enumerate(seam_angles()):
        lo, hi = live & (th > sm - 2 * eps) & (th < sm), live & (th > sm) & (th < sm + 2 * eps)
        if not lo.any() or not hi.any():
            problems.append("seam %d + 1/2 not approached from %s" % (i, "below" if not lo.any() else "above"))
        near = set(np.unique(idx[live & (np.abs(th - sm) < 0.01)]).tolist())
        if not {i, i + 1} <= near:
            problems.append("seam %d + 1/2: entries selected around it are %s" % (i, sorted(near)))
    for i, b in enumerate(boundary_angles(), start=1):  # pmt = pi - theta crosses i pi / 16 at theta = pi - b
        tb = math.pi - b
        lo, hi = live & (th > tb - 2 * eps) & (th < tb), live & (th > tb) & (th < tb + 2 * eps)
        if not lo.any() or not hi.any():
            problems.append("interval boundary %d not approached from both sides" % i)
            continue
        if not (np.all(iv[lo] == i) and np.all(iv[hi] == i - 1)):
            problems.append("interval boundary %d: intervals %s below theta_b, %s above" % (i, np.unique(iv[lo]), np.unique(iv[hi])))
        if cu[lo].max() > -1 + 1e-3 or cu[hi].min() < 1 - 1e-3:
            problems.append("interval boundary %d: |u| stays away from 1" % i)
    figures = {"max_residual": float(res[live].max()), "max_comp_u": float(np.abs(cu[live]).max()),
               "entries": int(np.unique(idx[live]).size), "intervals": int(np.unique(iv[live]).size)}
    if figures["max_residual"] > 0.03:
        problems.append("arctangent residual %.4f > 0.03" % figures["max_residual"])
    if figures["max_comp_u"] > 1.0 + 1e-9:
        problems.append("composite |u| = %.12f > 1" % figures["max_comp_u"])
    return problems, figures
