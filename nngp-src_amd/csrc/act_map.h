// The closed-form maps of one hidden layer (include/nngp_activations.h), shared by the kernel build (kernel_build.hip) and the
// additive kernel build (kernel_build_additive.hip).  Device code only; include after f64_math.h.
#pragma once
#include "common.h"
#include "f64_math.h"

namespace nngp {

constexpr double kPi = 3.14159265358979323846;

// ap: ArchDev::ap.
// act_diag: a diagonal entry q through hidden layer `code` -- q' and kdot.  It is also what a row's q becomes, so the symmetric
// build's diagonal, the rows' q of its cross entries and k_diag_from_q_act all go through this one function (bit-identical).
// Erf: asin(u / sqrt(u^2 + w^2)) = atan2(u, w) = pi_minus_atan2(w, u) - pi / 2, with w = sqrt(1 + 4 b^2 q) on the diagonal.
__device__ __forceinline__ void act_diag(int code, const double* ap, double q, const double* __restrict__ tab, double& qo,
                                         double& kd) {
    if (code == NNGP_ACT_ERF) {
        const double w = fast_sqrt_pos(fma(2.0 * ap[1], q, 1.0));  // >= 1: q >= 0
        qo = fma(ap[0], pi_minus_atan2(w, ap[1] * q, tab) - 0.5 * kPi, ap[2]);
        kd = ap[3] * fast_rcp(w);
    } else if (code == NNGP_ACT_ABRELU) {
        qo = ap[2] * q;
        kd = ap[2];
    } else {
        qo = 0.5 * q;
        kd = 0.5;
    }
}

// act_cross: an off-diagonal entry k with diagonals q1, q2.  Erf: r = 1 + 2 b^2 (q1 + q2) + 4 b^4 (q1 q2 - k^2) -- r >= 1 and no term
// cancels, so w keeps its relative precision for near-duplicate rows (the product form (1 + 2 b^2 q1)(1 + 2 b^2 q2) - u^2 loses
// ~6 digits at raw forest norms, and the arcsine is first-order sensitive to w).  The bracket is fma(q1, q2, -k^2) plus the
// rounding error of k^2 (Kahan's difference of products, one more fma): without it that rounding alone is q ulp of r.
// ABRelu(a, b) = a b k + (b - a)^2 relu(k): the ReLU map's own arithmetic, then one fma.
__device__ __forceinline__ void act_cross(int code, const double* ap, double k, double q1, double q2,
                                          const double* __restrict__ tab, double& ko, double& kd) {
    if (code == NNGP_ACT_ERF) {
        const double kk = k * k;
        const double br = fmax(fma(q1, q2, -kk) + fma(-k, k, kk), 0.0);
        const double w = fast_sqrt_pos(fma(ap[1] * ap[1], br, fma(ap[1], q1 + q2, 1.0)));
        ko = fma(ap[0], pi_minus_atan2(w, ap[1] * k, tab) - 0.5 * kPi, ap[2]);
        kd = ap[3] * fast_rcp(w);
    } else {
        const double rr = fma(q1, q2, -k * k);
        const double s = rr > 0.0 ? fast_sqrt_pos(rr > 0.0 ? rr : 1.0) : 0.0;
        const double kr = pi_minus_atan2(s, k, tab) * (0.5 / kPi);
        const double kk = fma(kr, k, s * (0.5 / kPi));
        if (code == NNGP_ACT_ABRELU) {
            ko = fma(ap[0], k, ap[1] * kk);
            kd = fma(ap[1], kr, ap[0]);
        } else {
            ko = kk;
            kd = kr;
        }
    }
}

}  // namespace nngp
