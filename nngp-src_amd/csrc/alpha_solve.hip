// The deferred CG solve for alpha (nngp_model::alpha_solve): nngp_model_solve only asks for it, run_pending_solve runs what is
// left of it on the solve stream for whoever needs alpha first, nngp_model_set_alpha / nngp_model_alpha hand alpha in and out.
// The decisions are AlphaPlan's (alpha_plan.h); here are the launches, the events and the waits.
#include "model.h"

namespace nngp {

void open_gate_epoch(nngp_model* m) { m->alpha_solve.gate_recorded = false; }

int record_cg_gate(nngp_model* m, hipStream_t s) {
    AlphaSolve& a = m->alpha_solve;
    if (a.ev_gate == nullptr) NNGP_HIP_CHECK(hipEventCreateWithFlags(&a.ev_gate, hipEventDisableTiming));
    NNGP_HIP_CHECK(hipEventRecord(a.ev_gate, s));
    a.gate_recorded = true;
    return 0;
}

int record_predict_end(nngp_model* m, hipStream_t s) {
    NNGP_HIP_CHECK(hipEventRecord(m->alpha_solve.ev_predict, s));
    m->alpha_solve.have_predict_event = true;
    return 0;
}

namespace {

// the preconditioner's inverted blocks: behind the factor (ev_ready), built here if nobody has yet
int join_tri(nngp_model* m) {
    NNGP_HIP_CHECK(hipStreamWaitEvent(m->solve_stream, m->alpha_solve.ev_ready, 0));
    return tri_join(m, m->solve_stream);
}

// alpha was written on the solve stream: a caller on another stream than the one that triggered the solve still has to be
// ordered behind it (free once the event has completed)
int order_behind_alpha(nngp_model* m, hipStream_t user, bool order_user) {
    const AlphaSolve& a = m->alpha_solve;
    if (order_user && a.plan.solved && a.plan.have_event) NNGP_HIP_CHECK(hipStreamWaitEvent(user, a.ev_solved, 0));
    return 0;
}

// alpha itself is needed: the stopped solve goes on where it was (behind the last predict, whose mean correction may still be
// reading the residual this is about to update)
int resume_stopped_solve(nngp_model* m) {
    AlphaSolve& a = m->alpha_solve;
    hipStream_t s = m->solve_stream;
    if (a.have_predict_event) NNGP_HIP_CHECK(hipStreamWaitEvent(s, a.ev_predict, 0));
    int it = 0;
    double rr = 0.0;
    NNGP_TRY(join_tri(m));
    NNGP_TRY(pcg_finish(m->k64, m->ld, m->n, m->reg, m->a32, m->ld, m->tri, m->np, m->pcg.xcol, m->pcg, a.plan.iters_done,
                        a.plan.max_iters, a.plan.tol, &it, &rr, s));
    NNGP_TRY(launch_strided_copy_f64(m->pcg.xcol, 1, m->alpha, m->ny, m->n, s));
    a.plan.begin_run();
    a.plan.note(it, rr);
    return 0;
}

int solve_afresh(nngp_model* m, bool allow_partial) {
    AlphaSolve& a = m->alpha_solve;
    hipStream_t s = m->solve_stream;
    a.plan.begin_run();
    const bool early = a.plan.may_stop_early(allow_partial, m->ny, NNGP_KNOB(0) == 128);
    const double early_tol = (NNGP_KNOB(3) >= 41 && NNGP_KNOB(3) <= 52) ? pow(10.0, -(double)(NNGP_KNOB(3) - 40)) : kPartialTol;
    const double tol = early ? early_tol : a.plan.tol;
    NNGP_TRY(join_tri(m));
    if (a.gate_recorded) NNGP_HIP_CHECK(hipStreamWaitEvent(s, a.ev_gate, 0));  // see i8s_product_rows
    for (int c = 0; c < m->ny; ++c) {
        NNGP_TRY(launch_strided_copy_f64(m->y + c, m->ny, m->pcg.bcol, 1, m->n, s));
        int it = 0;
        double rr = 0.0;
        NNGP_TRY(pcg_solve(m->k64, m->ld, m->n, m->reg, m->a32, m->ld, m->tri, m->np, m->pcg.bcol, m->pcg.xcol, m->pcg,
                           a.plan.max_iters, tol, &it, &rr, s));
        NNGP_TRY(launch_strided_copy_f64(m->pcg.xcol, 1, m->alpha + c, m->ny, m->n, s));
        if (early && rr > a.plan.tol) a.plan.stopped_early(it);
        a.plan.note(it, rr);
    }
    return 0;
}

// alpha is on its way on the solve stream: the caller's stream goes behind it, or the host waits
int publish_alpha(nngp_model* m, hipStream_t user, bool order_user) {
    AlphaSolve& a = m->alpha_solve;
    NNGP_HIP_CHECK(hipEventRecord(a.ev_solved, m->solve_stream));
    a.plan.have_event = true;
    if (order_user) NNGP_HIP_CHECK(hipStreamWaitEvent(user, a.ev_solved, 0));
    else NNGP_HIP_CHECK(hipStreamSynchronize(m->solve_stream));
    return 0;
}

}  // namespace

int run_pending_solve(nngp_model* m, hipStream_t user, bool order_user, bool allow_partial) {
    switch (m->alpha_solve.plan.next(allow_partial)) {
    case AlphaNext::OrderOnly: return order_behind_alpha(m, user, order_user);
    case AlphaNext::Resume: NNGP_TRY(resume_stopped_solve(m)); break;
    case AlphaNext::Fresh: NNGP_TRY(solve_afresh(m, allow_partial)); break;
    }
    return publish_alpha(m, user, order_user);
}

}  // namespace nngp

using namespace nngp;

extern "C" {

int nngp_model_solve(nngp_model* m, int32_t max_iters, double tol, void* stream) {
    NNGP_REQUIRE(m != nullptr && m->factored, "solve: factor first");
    NNGP_REQUIRE(!m->k64_partial, "solve: this model holds only its own kernel rows (row-sharded layout): the caller drives the CG "
                                  "(nngp_model_precond, nngp_model_matvec_rows) and hands alpha back with nngp_model_set_alpha");
    NNGP_HIP_CHECK(hipEventRecord(m->alpha_solve.ev_ready, (hipStream_t)stream));  // everything the solve reads has been enqueued there
    // Deferred, all of it.  (Starting the first six iterations here, on the solve stream, was measured and dropped: N = 32768: 155.8 vs
    // 152.5 ms per step, N = 8192: 16.0 vs 15.3, N = 65536: 716 vs 706 -- scripts/archive/dropped/cg_first_iterations_ahead_of_the_gate.patch.)
    m->alpha_solve.plan.request(max_iters, tol, m->reg, m->reg_fac);
    return 0;
}

int nngp_model_set_alpha(nngp_model* m, const double* alpha, int32_t iters, double rel_residual, void* stream) {
    NNGP_REQUIRE(m != nullptr && m->factored && alpha != nullptr, "set_alpha: factor first");
    NNGP_HIP_CHECK(hipMemcpyAsync(m->alpha, alpha, sizeof(double) * m->n * m->ny, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    m->alpha_solve.plan.installed(iters, rel_residual);
    return 0;
}

int nngp_model_alpha(nngp_model* m, double* alpha_out, void* stream) {
    NNGP_REQUIRE(m != nullptr && m->alpha_solve.plan.solved && alpha_out != nullptr, "model_alpha: solve first");
    NNGP_TRY(run_pending_solve(m, (hipStream_t)stream, true));
    NNGP_HIP_CHECK(hipMemcpyAsync(alpha_out, m->alpha, sizeof(double) * m->n * m->ny, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream));
    return 0;
}

}  // extern "C"
