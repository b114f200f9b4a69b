// float64 helpers of the kernel build's layer map (kernel_build.hip), shared with the marginal-likelihood gradient
// (nngp_mll.hip).  Device code only; include after hip_runtime.h.
#pragma once
#include <hip/hip_runtime.h>

namespace nngp {

// ---- float64 arithmetic of the ReLU map at ~1/2 of the libm cost (the epilogue is bound by the float64 ALUs) ---------------
// Measured on gfx950 (scripts/micro/f64_seed_accuracy.hip, 2^24 inputs over 2^-20 .. 2^21): v_rcp_f64 is good to 2^-24.4 and one
// Newton step brings it to 2.2e-15; v_rsq_f64 is good to 2^-24.2 and one coupled (Goldschmidt) iteration plus the residual
// correction reproduces the correctly rounded sqrt on every input tried.
__device__ __forceinline__ double fast_rcp(double x) {  // 1 / x to 2.2e-15, x > 0
    const double r = __builtin_amdgcn_rcp(x);
    return fma(r, fma(-x, r, 1.0), r);
}

__device__ __forceinline__ double fast_sqrt_pos(double r) {  // sqrt(r), r > 0
    const double y = __builtin_amdgcn_rsq(r);
    double g = r * y, h = 0.5 * y;
    const double e = fma(-h, g, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    return fma(fma(-g, g, r), h, g);
}

// pi - atan2(s, k) for s >= 0 (what the ReLU map needs; s = k = 0 gives pi / 2, the reference's fill value).
// A float32 estimate of the angle picks the nearest of 65 table angles a_i = i pi / 64; the pair (k, s) is rotated by -a_i in
// float64, which leaves a residual angle below 0.03 rad whose arctangent is u - u^3/3 + ... + u^9/9 (next term < 2e-18).
// tab[i] = {cos a_i, sin a_i, a_i, pi - a_i} in LDS.  Absolute error of the arctangent itself <= 5.2e-16 for the s, k it is given
// (NumPy restatement of these exact steps against mpmath over [0, pi], every seam (i + 1/2) pi / 64 from both sides, residual
// <= 0.0293: tests/angle_reference.py, tests/test_angle_math_host.py; on the device: tests/test_gpu_kernel_angles.py).  Next to
// 0 and pi the caller's s = sqrt(q q' - k^2) carries the rounding of k k, u |k|^3 / (2 s rho^2) of angle, on top of that.
__device__ __forceinline__ double pi_minus_atan2(double s, double k, const double* __restrict__ tab) {
    const double ak = fabs(k);
    const double mx = fmax(s, ak), mn = fmin(s, ak);
    float t = mx > 0.0 ? (float)(mn * __builtin_amdgcn_rcp(mx)) : 0.0f;
    float at = t * fmaf(-0.1919f, t * t, 0.9724f);  // atan on [0, 1] to 5e-3: only the table index depends on it
    at = s > ak ? 1.57079637f - at : at;
    at = k < 0.0 ? 3.14159274f - at : at;
    int i = (int)rintf(at * 20.3718327f);  // 64 / pi
    i = i < 0 ? 0 : (i > 64 ? 64 : i);
    const double2 cs = *reinterpret_cast<const double2*>(tab + 4 * i);
    const double xp = fma(k, cs.x, s * cs.y);      // rho cos(theta - a_i) > 0
    const double yp = fma(s, cs.x, -(k * cs.y));   // rho sin(theta - a_i)
    const double u = yp * fast_rcp(xp);
    const double w = u * u;
    double p = fma(w, 1.0 / 9.0, -1.0 / 7.0);
    p = fma(p, w, 1.0 / 5.0);
    p = fma(p, w, -1.0 / 3.0);
    const double atu = fma(u, p * w, u);
    const double pmt = tab[4 * i + 3] - atu;       // (pi - a_i) - (theta - a_i)
    return mx > 0.0 ? pmt : 0.5 * 3.14159265358979323846;
}

}  // namespace nngp
