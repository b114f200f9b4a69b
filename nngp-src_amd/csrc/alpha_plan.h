// The deferred alpha solve's decisions that need no device (alpha_solve.hip): what a request asks for, what the next caller has to
// run, when the CG may stop early, and what info() reports.  Host code only -- no HIP header -- so that it also builds as a plain
// C++ program (tests/sanitize).
#pragma once
#include <math.h>

namespace nngp {

// Stopping tolerance of the early-stopped solve.  Measured at N = 32768 (ms per step / error of the corrected mean): 1e-6:
// 150.0 / 8e-11, 1e-4: 147.5 / 4e-9, 1e-2: 145.9 / 2e-7.  1e-6 it is: the iteration count extrapolated from a solve stopped
// at 1e-4 underestimates slowly converging fits (two of the sweep's 72 cases then missed the adaptive covariance).
// (Round 2, level-1 variance: 1e-4 saves 2.2 of 113 ms; a two-staged stop -- 1e-4 only if reached within three iterations --
// kept the adaptive covariance right, but the corrected means at N = 8192 / 32768 then sit 1.3e-6 / 4.8e-6 (elementwise)
// from the oracle instead of 3e-9: not taken.)
constexpr double kPartialTol = 1e-6;

enum class AlphaNext {
    OrderOnly,  // alpha (or, for a caller that corrects the mean, the stopped solve's a_k) is there: only order the caller behind it
    Resume,     // the solve stopped early and alpha itself is needed: take it up where it was
    Fresh,      // a request is pending: solve from x = 0
};

struct AlphaPlan {
    bool solved = false;   // alpha was asked for (request) or handed in (installed): predict and alpha() may be called
    bool pending = false;  // asked for, not run yet
    // Early stop (ny == 1): a predict that also forms the covariance rows Z ~ K_td (K + reg I)^-1 stops the CG at kPartialTol and
    // corrects the mean through them: mu = K_td a_k + Z r_k (exact up to (K_td A^-1 - Z) r_k, the product of two small
    // errors).  partial: alpha holds a_k and the CG state is intact; anything that needs alpha itself resumes.
    bool partial = false;
    int iters_done = 0;  // ... iterations the stopped solve has run
    int max_iters = 60;
    double tol = 1e-10;
    int iters = 0;        // info(): iterations the solve needed (or would need) to reach tol
    double relres = 0.0;  // info(): relative residual it reached
    bool have_event = false;  // ev_solved has been recorded at least once

    // nngp_model_solve.  Default: 60 iterations; a factor with a raised shift preconditions worse by ~ sqrt(reg_fac / reg)
    void request(int max_iters_asked, double tol_asked, double reg, double reg_fac) {
        const double weak = (reg > 0.0 && reg_fac > reg) ? sqrt(reg_fac / reg) : 1.0;
        max_iters = max_iters_asked > 0 ? max_iters_asked : (int)fmin(2000.0, 60.0 * weak);
        tol = tol_asked > 0.0 ? tol_asked : 1e-10;
        partial = false;
        pending = true;
        solved = true;
    }
    // nngp_model_set_alpha: alpha was written on the caller's stream, in order
    void installed(int iters_given, double relres_given) {
        drop();
        solved = true; have_event = false;
        iters = iters_given; relres = relres_given;
    }
    void drop() { pending = partial = false; }     // what the solve reads, or its state, is about to change
    void invalidate() { drop(); solved = false; }  // ... and with it what alpha solves

    AlphaNext next(bool allow_partial) const {
        if (pending) return AlphaNext::Fresh;
        return (partial && !allow_partial) ? AlphaNext::Resume : AlphaNext::OrderOnly;
    }
    // allow_partial: the caller can correct the mean through the covariance rows.  never: a caller's switch
    bool may_stop_early(bool allow_partial, int ny, bool never) const { return allow_partial && ny == 1 && tol < 1e-3 && !never; }

    void begin_run() { pending = partial = false; iters = 0; relres = 0.0; }  // a solve, or the rest of one, is being enqueued
    // one column's solve ended after `it` iterations at `rr`: iterations it needs (or would need) to reach tol, from the rate it converged at
    void note(int it, double rr) {
        int est = it;
        if (rr > tol && rr > 0.0 && rr < 1.0 && it > 0) est = (int)ceil(it * log(tol) / log(rr));
        if (est > iters) iters = est;
        if (rr > relres) relres = rr;
    }
    void stopped_early(int it) { partial = true; iters_done = it; }
};

}  // namespace nngp
