// The int8 residual's decisions that need no device (residual_i8.hip): from which sizes on its products pay, and how far a fit's
// guard estimates let it be trusted.  Host code only -- no HIP header -- so that it also builds as a plain C++ program (tests/sanitize).
#pragma once
#include <stdint.h>

namespace nngp {

// Estimated |z . dr| / variance above which a fit is taken off the int8 residual: level 1 is itself 1e-6 .. 5e-6 from the converged
// variance; the bench fits sit at ~1e-7 (nngp_model_residual_floor)
constexpr double kI8FloorThr = 1e-5;

// From which size on the two grades of the product pay (np: padded training rows, mp: padded right-hand-side rows); the
// measurements are with use_i8s and use_i8s_fine.
inline bool i8_coarse_pays(int64_t np, int64_t mp) { return np >= 2048 && mp >= 256; }
inline bool i8_fine_pays(int64_t np, int64_t mp) { return np >= 4096 && mp >= 512; }

// What the guard has found out about the current kernel matrix.
struct I8Trust {
    bool checked = false;      // the first level-1 predict of the fit has seen its own estimate
    bool distrusted = false;   // an estimate was above the threshold: float64 pipe until K changes
    bool pending = false;      // a later batch's estimate is on its way to the host
    double floor_ratio = -1.0; // the largest estimate seen

    void new_kernel() { checked = distrusted = pending = false; }
    // a later batch's estimate has arrived
    void fold(double ratio, double threshold) {
        pending = false;
        if (ratio > floor_ratio) floor_ratio = ratio;
        if (!(ratio <= threshold)) distrusted = true;
    }
    // the first predict's own estimate; true: form the covariance again, on the float64 pipe
    bool first_verdict(double ratio, double threshold) {
        floor_ratio = ratio;
        checked = true;
        if (ratio <= threshold) return false;
        distrusted = true;
        return true;
    }
};

}  // namespace nngp
