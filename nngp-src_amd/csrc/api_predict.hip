// The posterior half of the C ABI: workspaces of a predict, the consumers of the factor (blocked solves, refinement sweeps; their int8
// residual products: residual_i8.hip), nngp_model_prepare_serving / _predict / _apply_factor.  Reference: predict_fn(x_test, get, compute_cov),
// train.py:157-158, estimator.py:66-67.
#include "model.h"

namespace nngp {

int ensure_predict_capacity(nngp_model* m, int64_t mt, bool need_ktd) {
    if (mt > m->m_cap || m->b32 == nullptr) {
        const int64_t cap = mt > m->m_cap ? mt : m->m_cap;
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(m->xt_q); dev_free(m->tt_diag); dev_free(m->b32); dev_free(m->trsm_tmp);
        NNGP_TRY(dev_alloc(&m->xt_q, cap));
        NNGP_TRY(dev_alloc(&m->tt_diag, cap));
        NNGP_TRY(dev_alloc(&m->b32, round_up(cap, TB) * m->np_cap));
        NNGP_TRY(dev_alloc(&m->trsm_tmp, round_up(cap, TB) * triinv_block(m->np_cap)));
        if (m->split.planes != nullptr) {  // split copy of one right-hand-side block (float16 path of the blocked solves)
            dev_free(m->split.planes_b); dev_free(m->split.row_inv);
            m->split.planes_b = nullptr; m->split.row_inv = nullptr;
            m->split.mb_cap = round_up(cap, TB);
            // one panel per 1024 columns of a solve step, col_stride bytes apart (see SplitWork)
            m->split.b_panels = (int)((triinv_block(m->np_cap) + m->split.k_cap - 1) / m->split.k_cap);
            NNGP_TRY(dev_alloc(&m->split.planes_b, (int64_t)(m->split.b_panels - 1) * m->split.col_stride + (m->split.mb_cap + 256) * m->split.k_cap * 4));
            NNGP_TRY(dev_alloc(&m->split.row_inv, m->split.mb_cap));
            // ... and the persistent form of the blocked solves (no room for its workspace: the step-by-step form stays)
            tk_destroy(m->tk);
            m->tk = nullptr;
            if (m->split.k_cap == 1024 && triinv_block(m->np_cap) == 1024) NNGP_TRY(tk_create(&m->tk, m->np_cap, m->split.mb_cap) < 0 ? -1 : 0);
        }
        m->m_cap = cap;
    }
    if (need_ktd && mt > m->ktd_cap) {
        const int64_t cap = mt > m->m_cap ? mt : m->m_cap;
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(m->ktd64);
        NNGP_TRY(dev_alloc(&m->ktd64, round_up(cap, TB) * m->np_cap));
        m->ktd_cap = cap;
    }
    return 0;
}

int ensure_full_cov_capacity(nngp_model* m, int64_t mt) {
    if (mt > m->full_cap) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(m->ktt64); dev_free(m->vvt32);
        const int64_t mp = round_up(mt, TB);
        dev_free(m->covp64);
        NNGP_TRY(dev_alloc(&m->ktt64, mp * mp));
        NNGP_TRY(dev_alloc(&m->vvt32, mp * mp));
        NNGP_TRY(dev_alloc(&m->covp64, mp * mp));
        m->full_cap = mt;
    }
    return 0;
}

// |L_ij| <= sqrt(max_i A_ii): scale of the float16 split copies of the factor, largest entry below 2^15
void set_split_scale(nngp_model* m) {
    const double lmax = sqrt(fmax(m->diag_max, m->trace_mean) + m->reg_fac);
    int e = 0;
    (void)frexp(lmax, &e);  // lmax = f * 2^e, f in [0.5, 1)
    m->split.scale = (lmax > 0.0 && std::isfinite(lmax)) ? (float)ldexp(1.0, 15 - e) : 1.0f;
}

int ensure_refine_capacity(nngp_model* m, int64_t mp) {
    if (mp > m->refine_cap) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(m->z64); dev_free(m->r64);
        NNGP_TRY(dev_alloc(&m->z64, mp * m->np_cap));
        NNGP_TRY(dev_alloc(&m->r64, mp * m->np_cap));
        m->refine_cap = mp;
    }
    if (mp > m->rows.cap) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        RowsPcg& w = m->rows;
        dev_free(w.rho); dev_free(w.coef); dev_free(w.tol); dev_free(w.delta); dev_free(w.var); dev_free(w.state); dev_free(w.zstat);
        NNGP_TRY(dev_alloc(&w.rho, mp)); NNGP_TRY(dev_alloc(&w.coef, mp)); NNGP_TRY(dev_alloc(&w.tol, mp));
        NNGP_TRY(dev_alloc(&w.delta, mp)); NNGP_TRY(dev_alloc(&w.var, mp)); NNGP_TRY(dev_alloc(&w.state, mp));
        NNGP_TRY(dev_alloc(&w.zstat, 2 * mp));
        if (w.live == nullptr) {
            NNGP_TRY(dev_alloc(&w.live, 6));
            NNGP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&w.host), 6 * sizeof(int32_t), hipHostMallocDefault));
        }
        w.cap = mp;
    }
    return 0;
}

// L^T and the transposed inverted diagonal blocks: operands of the "B L^-1" half of (L L^T)^-1 on the float32 path.
int ensure_lt_alloc(nngp_model* m) {
    if (m->lt32 != nullptr) return 0;
    NNGP_HIP_CHECK(hipDeviceSynchronize());
    NNGP_TRY(dev_alloc(&m->lt32, m->np_cap * m->np_cap));
    NNGP_TRY(dev_alloc(&m->dinvt, (m->np_cap / TB) * TB * TB));
    return 0;
}
int ensure_lt(nngp_model* m, hipStream_t s) {
    if (m->lt_ready) return 0;
    NNGP_TRY(ensure_lt_alloc(m));
    NNGP_TRY(launch_transpose_f32(m->a32, m->ld, m->lt32, m->np, m->np, s));
    NNGP_TRY(launch_transpose_blocks_f32(m->dinv, m->dinvt, TB, m->np / TB, s));
    m->lt_ready = true;
    return 0;
}

// split copy of L^T by block row (operand of the "B L^-1" half on the float16 pipe); built once per fit
int ensure_lt_split(nngp_model* m, hipStream_t s) {
    if (m->split.lt_ready) return 0;
    if (m->split.planes_t == nullptr) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        const int64_t ncols = (m->np_cap + m->split.k_cap - 1) / m->split.k_cap;
        NNGP_TRY(dev_alloc(&m->split.planes_t, ncols * m->split.col_stride));
    }
    NNGP_TRY(launch_split_lower_t(m->a32, m->ld, m->np, m->split.k_cap, m->split.scale, m->split.planes_t,
                                  m->split.col_stride, s));
    m->split.lt_ready = true;
    return 0;
}


// every reader of m->tri calls this on the stream it reads from: builds the inverted blocks there if nobody has yet, else orders the
// stream behind whoever did
int tri_join(nngp_model* m, hipStream_t s) {
    if (m->tri_stale) {
        if (m->ev_tri == nullptr) NNGP_HIP_CHECK(hipEventCreateWithFlags(&m->ev_tri, hipEventDisableTiming));
        NNGP_TRY(triinv_build(m->a32, m->ld, m->dinv, m->np, m->tri, s));
        if (m->tk != nullptr && m->tri.bs == 1024) NNGP_TRY(tk_prepare_inverses(m->tk, m->tri, m->np, m->a32, m->ld, s));
        NNGP_HIP_CHECK(hipEventRecord(m->ev_tri, s));
        m->tri_stale = false;
        m->tri_pending = true;
        return 0;
    }
    if (m->tri_pending) NNGP_HIP_CHECK(hipStreamWaitEvent(s, m->ev_tri, 0));
    if (m->tk != nullptr && !tk_inverses_ready(m->tk) && m->tri.bs == 1024) {  // the workspace was rebuilt after the blocks were inverted
        NNGP_TRY(tk_prepare_inverses(m->tk, m->tri, m->np, m->a32, m->ld, s));
        if (m->ev_tri == nullptr) NNGP_HIP_CHECK(hipEventCreateWithFlags(&m->ev_tri, hipEventDisableTiming));
        NNGP_HIP_CHECK(hipEventRecord(m->ev_tri, s));
        m->tri_pending = true;
    }
    return 0;
}

// predict: the build goes to the panel stream (idle between factorisations) behind what `s` holds now; tri_join orders the readers
int tri_fork(nngp_model* m, hipStream_t s) {
    if (!m->tri_stale || m->la == nullptr || m->la->panel == nullptr || NNGP_KNOB(5) == 61) return 0;  // key 5 = 61: in line
    if (m->ev_tri == nullptr) NNGP_HIP_CHECK(hipEventCreateWithFlags(&m->ev_tri, hipEventDisableTiming));
    if (m->ev_tri_fork == nullptr) NNGP_HIP_CHECK(hipEventCreateWithFlags(&m->ev_tri_fork, hipEventDisableTiming));
    NNGP_HIP_CHECK(hipEventRecord(m->ev_tri_fork, s));
    NNGP_HIP_CHECK(hipStreamWaitEvent(m->la->panel, m->ev_tri_fork, 0));
    NNGP_TRY(triinv_build(m->a32, m->ld, m->dinv, m->np, m->tri, m->la->panel));
    if (m->tk != nullptr && m->tri.bs == 1024) NNGP_TRY(tk_prepare_inverses(m->tk, m->tri, m->np, m->a32, m->ld, m->la->panel));
    NNGP_HIP_CHECK(hipEventRecord(m->ev_tri, m->la->panel));
    m->tri_stale = false;
    m->tri_pending = true;
    return 0;
}

// the factor has float16-split copies (look-ahead factorisation) and the caller did not ask for the float32 path
// and the block of right-hand sides is large enough for the 256-row tiles of the float16 GEMM to pay (measured, ms per
// diag-variance call at level 2, float16 / float32 solves -- N = 10800: M = 128: 6.5 / 5.6, 512: 9.1 / 8.8, 1024: 11.5 / 12.9;
// N = 32768: M = 128: 21.8 / 20.1, 256: 29.3 / 30.6, 512: 40.6 / 51.5)
bool use_split_solves(const nngp_model* m, int64_t mp) {
    return m->split.l_ready && m->split.planes_b != nullptr && mp <= m->split.mb_cap && m->tri.bs % m->split.k_cap == 0 &&
           m->tri.bs / m->split.k_cap <= m->split.b_panels && m->tri.bs <= 2048 && NNGP_KNOB(7) == 0 && mp >= 256 && mp * m->np >= 7000000;
}

// one persistent, ticket-ordered launch per solve (trsm_tickets.hip) instead of np / 1024 steps of three launches (debug key 9 = 16: the steps)
bool use_tickets(const nngp_model* m, int64_t mp) {
    return !m->tk_failed && m->tri.bs == 1024 && tk_usable(m->tk, mp, m->np) && NNGP_KNOB(9) != 16;
}

// The one decision which triangular solve runs for mp right-hand sides: the 128-wide recursion (timing experiment, debug key 7 = 1), the
// 1024-block form in float32, the same on the split-float16 copies of the factor step by step, or that as one persistent launch per
// solve.  It reads the model as it is when asked: whoever needs the answer asks where it needs it.
SolvePath solve_path(const nngp_model* m, int64_t mp) {
    if (NNGP_KNOB(7) == 1) return SolvePath::Recursion128;
    if (!use_split_solves(m, mp)) return SolvePath::BlocksF32;
    return use_tickets(m, mp) ? SolvePath::Tickets : SolvePath::BlocksH3;
}

// Where a predict's side work goes beside the persistent solves (profiles/r5_posterior_schedule_ab.txt records the choice).  gate
// (NNGP_TK_GATE): 0 = the alpha CG waits for the plane products' start as on the other paths; reserve (NNGP_TK_RESERVE): compute
// units the solves leave free while K's planes are cut (measured 0 / 32 / 48 / 64: posterior 29.8-30.1 / 30.1 / 30.3 / 29.8 ms at cfg3);
// cutstream (NNGP_TK_CUTSTREAM): the early plane cut goes to the 0 solve, 1 panel, 2 update stream.  Constants in the product
// library; only the timing-knobs build still reads these three development aids from the environment.
struct TicketSchedule { int gate, reserve, cutstream; };
static const TicketSchedule& ticket_schedule() {
#ifdef NNGP_TIMING_KNOBS
    auto env = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    static const TicketSchedule t = {env("NNGP_TK_GATE", 1), env("NNGP_TK_RESERVE", 0), env("NNGP_TK_CUTSTREAM", 2)};
#else
    static const TicketSchedule t = {1, 0, 2};
#endif
    return t;
}

// With the blocked solves as persistent launches (224 registers, 128 KB of LDS: a 64-register kernel with a few KB of LDS fits beside
// their workgroups) the deferred alpha CG no longer waits for the plane products' start: it runs from the predict's start on.
bool cg_from_the_start(const nngp_model* m, int64_t mp) { return ticket_schedule().gate != 0 && solve_path(m, mp) == SolvePath::Tickets; }

// While the digit planes of K are being cut on the solve stream (one 132 KB workgroup per compute unit: it cannot share a unit with a
// persistent solve) the solves leave it some units; the alpha CG's light kernels fit beside the solve's workgroups as they are.
int tickets_reserve(const nngp_model* m) { return m->i8.k_pending ? ticket_schedule().reserve : 0; }

// The stream of a predict's early plane cut (cut_planes_early): the solve stream -- but with the alpha CG running from the predict's
// start (cg_from_the_start) the cut must not sit in front of it on the solve stream, nor in front of the inverted blocks on the
// panel stream
hipStream_t early_cut_stream(const nngp_model* m, int64_t mp) {
    const int cut_stream = ticket_schedule().cutstream;
    hipStream_t cs = m->solve_stream;
    if (cut_stream != 0 && cg_from_the_start(m, mp) && m->la != nullptr && m->la->panel != nullptr)
        cs = (cut_stream == 2 && m->la->update != nullptr) ? m->la->update : m->la->panel;
    return cs;
}

// a persistent solve that gave up waiting left its error word behind: report it once, and keep the model off that path
int tickets_check(nngp_model* m, bool wait) {
    const int e = tk_poll_error(m->tk, wait);
    if (e == 0) return 0;
    m->tk_failed = true;
    set_error("a persistent blocked solve gave up waiting for a dependency (error word 0x%x): its results are invalid; the model now uses the step-by-step solves", e);
    return -6;
}

// event pair around one blocked solve of mp right-hand sides (np^2 mp flops: a triangular matrix, multiply-add = 2)
static int trsm_timer_begin(nngp_model* m, int64_t mp, hipStream_t s, int* slot) {
    NNGP_TRY(m->trsm_t.begin(s, slot));
    if (*slot >= 0) m->trsm_flops[*slot] = (double)m->np * (double)m->np * (double)mp;
    return 0;
}

static int apply_forward_untimed(nngp_model* m, int64_t mp, hipStream_t s);

// b32 [mp, np] <- b32 L^-T   (rows are right-hand sides)
int apply_forward_f32(nngp_model* m, int64_t mp, hipStream_t s) {
    NNGP_TRY(tickets_check(m, false));
    NNGP_TRY(tri_join(m, s));
    int slot = -1;
    NNGP_TRY(trsm_timer_begin(m, mp, s, &slot));
    NNGP_TRY(apply_forward_untimed(m, mp, s));
    return m->trsm_t.end(slot);
}

static int apply_forward_untimed(nngp_model* m, int64_t mp, hipStream_t s) {
    // While the deferred alpha CG runs on its own stream (from the int8 residual's gate on), the solves' persistent update grids
    // leave it some compute units (debug key 13 = n: n units; default 0 = none -- see DESIGN_NOTES R4)
    m->split.solve_reserve = (m->alpha_solve.gate_recorded && NNGP_KNOB(13) > 0) ? NNGP_KNOB(13) : 0;
    switch (solve_path(m, mp)) {
    case SolvePath::Recursion128: return trsm_rlt_f32(m->b32, m->np, mp, m->a32, m->ld, m->dinv, m->np, s);
    case SolvePath::Tickets: return tk_solve(m->tk, m->b32, m->np, mp, m->np, m->split, false, s, tickets_reserve(m));
    case SolvePath::BlocksH3: return trsm_rlt_blocks_h3(m->b32, m->np, mp, m->a32, m->ld, m->tri, m->np, m->trsm_tmp, m->split, s);
    case SolvePath::BlocksF32: break;
    }
    return trsm_rlt_blocks_f32(m->b32, m->np, mp, m->a32, m->ld, m->tri, m->np, m->trsm_tmp, s);
}

// b32 [mp, np] <- b32 (L L^T)^-1
int apply_inverse_f32(nngp_model* m, int64_t mp, hipStream_t s) {
    // The split copy of L^T (first covariance predict after a fit) is only read by the second half: it is written on the
    // model's own stream (idle until the alpha CG is asked for) beside the forward solve.  (debug key 2 = 7: in stream order)
    const bool lt_aside = !needs_lt32(solve_path(m, mp)) && !m->split.lt_ready && m->split.planes_t != nullptr &&
                          m->ev_lt != nullptr && NNGP_KNOB(2) != 7;
    if (lt_aside) {
        NNGP_HIP_CHECK(hipEventRecord(m->ev_lt, s));
        NNGP_HIP_CHECK(hipStreamWaitEvent(m->solve_stream, m->ev_lt, 0));
        NNGP_TRY(ensure_lt_split(m, m->solve_stream));
        NNGP_HIP_CHECK(hipEventRecord(m->ev_lt, m->solve_stream));
    }
    NNGP_TRY(apply_forward_f32(m, mp, s));
    if (NNGP_KNOB(2) == 10 && !m->alpha_solve.gate_recorded && m->alpha_solve.plan.pending) {  // timing experiment: the deferred alpha CG starts with the backward solve
        NNGP_TRY(record_cg_gate(m, s));
    }
    if (lt_aside) NNGP_HIP_CHECK(hipStreamWaitEvent(s, m->ev_lt, 0));
    // (whoever gets here on the float32 path finds its operand built: round 4's null-pointer abort came from a caller that had not)
    const SolvePath path = solve_path(m, mp);
    if (needs_lt32(path)) NNGP_TRY(ensure_lt(m, s));
    else NNGP_TRY(ensure_lt_split(m, s));
    if (path == SolvePath::Recursion128) return trsm_rut_f32(m->b32, m->np, mp, m->lt32, m->np, m->dinvt, m->np, s);  // (untimed)
    int slot = -1;
    NNGP_TRY(trsm_timer_begin(m, mp, s, &slot));
    if (path == SolvePath::Tickets)
        NNGP_TRY(tk_solve(m->tk, m->b32, m->np, mp, m->np, m->split, true, s, tickets_reserve(m)));
    else if (path == SolvePath::BlocksH3)
        NNGP_TRY(trsm_rut_blocks_h3(m->b32, m->np, mp, m->lt_ready ? m->lt32 : nullptr, m->np, m->tri, m->np, m->trsm_tmp, m->split, s));
    else
        NNGP_TRY(trsm_rut_blocks_f32(m->b32, m->np, mp, m->lt32, m->np, m->tri, m->np, m->trsm_tmp, s));
    return m->trsm_t.end(slot);
}

// NTK covariance: the error of Z enters in first order (no cancellation as in the NNGP form), so what the sweeps leave is
// what the variance gets, ~ rho^(sweeps + 1) with rho the contraction of the float32 factor as a solver.  Measured at
// N = 16384, d = 256, join-block encoding, 4 CG iterations in the alpha solve (scripts/ntk_var_study.py, worst relative
// error over 1024 queries against 4 sweeps / ms per predict): 1 sweep 2.7e-5 / 24.8, 2 sweeps 3.6e-8 / 36.8, 3 sweeps
// 2.0e-8 / 49.0.  Levels <= 2: two sweeps; above: that many.
static int ntk_sweeps(const nngp_model* m) { return m->var_refine < 2 ? 2 : m->var_refine; }

// z64 <- rows of `rhs` [mp, np] times (K + reg I)^-1: float32 solves corrected by `sweeps` float64 residual sweeps.
// final_residual: also leave r64 = rhs - z64 (K + reg I) for the returned z64 (one more float64 product).
// measure (sweeps >= 2): the error energies r . M^-1 r that the first two corrections saw are kept in rows.var and
// rows.delta, and z . rhs in rows.tol, for k_sweep_estimate -- three passes over [mp, np].
// note (optional): handed to every residual (ResidualNote).
int refined_solve_rows(nngp_model* m, const double* rhs, int64_t mp, int sweeps, bool final_residual, hipStream_t s,
                       bool measure, ResidualNote* note) {
    const int64_t np = m->np;
    measure = measure && sweeps >= 2;
    NNGP_TRY(launch_convert_f64_f32(rhs, np, m->b32, np, mp, np, mp, np, s));
    NNGP_TRY(apply_inverse_f32(m, mp, s));
    NNGP_TRY(launch_f32_to_f64_mat(m->b32, np, m->z64, np, mp, np, false, s));
    for (int it = 0; it < sweeps + (final_residual ? 1 : 0); ++it) {
        NNGP_TRY(residual_rows(m, m->r64, rhs, m->z64, mp, s, it == 0, note));
        if (it == sweeps) break;
        NNGP_TRY(launch_convert_f64_f32(m->r64, np, m->b32, np, mp, np, mp, np, s));
        NNGP_TRY(apply_inverse_f32(m, mp, s));
        if (measure && it < 2) NNGP_TRY(launch_rows_energy(m->r64, m->b32, np, mp, np, it == 0 ? m->rows.var : m->rows.delta, s));
        NNGP_TRY(launch_f32_to_f64_mat(m->b32, np, m->z64, np, mp, np, true, s));
    }
    if (measure) NNGP_TRY(launch_rowdot_f64(m->z64, nullptr, 0.0, rhs, np, mp, np, nullptr, 1.0, m->rows.tol, s));
    return 0;
}

// Continues the correction of z64 (rows of rhs (K + reg I)^-1) by preconditioned CG, every row with its own scalars,
// until each row's step no longer lowers e^T A e by more than rows.tol[row] (twice in a row) or max_iters is reached.
// In: z64 and its residual r64 = rhs - z64 (K + reg I); out: both updated.  The stationary sweeps contract by the
// spectral radius of I - M^-1 A, which approaches 1 when cond(K + reg I) * eps32 does (small diag_reg, low-dimensional
// encodings: seen at cond 2.6e7, where four sweeps left 4e-2 in the variance); CG on the same operator needs ~the
// iteration count of the alpha solve.  One host read-back per iteration (the count of rows still iterating).
int rows_pcg_continue(nngp_model* m, int64_t mp, int max_iters, hipStream_t s) {
    const int64_t np = m->np;
    RowsPcg& w = m->rows;
    if (mp > m->rows_pq_cap) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(w.p); dev_free(w.q);
        w.p = w.q = nullptr;
        NNGP_TRY(dev_alloc(&w.p, mp * m->np_cap));
        NNGP_TRY(dev_alloc(&w.q, mp * m->np_cap));
        m->rows_pq_cap = mp;
    }
    m->cov_iters = 0;
    for (int it = 0; it < max_iters; ++it) {
        NNGP_TRY(launch_convert_f64_f32(m->r64, np, m->b32, np, mp, np, mp, np, s));
        NNGP_TRY(apply_inverse_f32(m, mp, s));
        NNGP_TRY(launch_rows_rho(m->r64, m->b32, np, mp, np, it == 0, w, s));
        NNGP_TRY(launch_rows_update_p(w.p, m->b32, np, mp, np, w, s));
        NNGP_TRY(launch_gemm_nt_f64(w.q, np, w.p, np, w.p, np, m->k64, m->ld, mp, np, np, 1.0, m->reg, s));
        NNGP_TRY(launch_rows_alpha(w.p, w.q, np, mp, np, w, s));
        NNGP_TRY(launch_rows_axpy2(m->z64, m->r64, w.p, w.q, np, mp, np, w, s));
        NNGP_HIP_CHECK(hipMemcpyAsync(w.host, w.live, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        NNGP_HIP_CHECK(hipStreamSynchronize(s));
        m->cov_iters = it + 1;
        if (w.host[0] == 0) break;
    }
    return 0;
}

int build_cross(nngp_model* m, const double* xt, const double* qt, int64_t mt, int64_t mp, bool nngp, double* out,
                hipStream_t s) {
    NNGP_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(double) * mp * m->np, s));
    BuildArgs a{};
    a.x1 = xt; a.x2 = m->x; a.q1 = qt; a.q2 = m->q;
    a.n1 = mt; a.n2 = m->n; a.d = m->d;
    a.row_begin = 0; a.row_end = mt; a.sym = 0;
    a.ld64 = a.ld32 = m->np;
    if (nngp) a.nngp64 = out; else a.ntk64 = out;
    return launch_kernel_build(a, m->arch, s);
}

// a model flag that is up for the length of a scope (and comes down on every way out of it)
struct ScopedFlag {
    bool& f;
    explicit ScopedFlag(bool& b) : f(b) { f = true; }
    ~ScopedFlag() { f = false; }
    ScopedFlag(const ScopedFlag&) = delete;
};

// Iterations a continuation by CG (rows_pcg_continue) may take: 80, times sqrt(reg_fac / reg) where the float32 factorisation had
// to raise the diagonal shift, 1000 at the most.
static int continuation_budget(const nngp_model* m) {
    const double shift = (m->reg > 0.0 && m->reg_fac > m->reg) ? sqrt(m->reg_fac / m->reg) : 1.0;
    return (int)fmin(1000.0, 80.0 * shift);
}

// ---- nngp_model_predict: its stages in the order predict_impl runs them (what one call knows and finds out: PredictCall, model.h) ----

// Row flag: a LOWER bound of the remaining relative variance error above this value (debug key 6 = e >= 2: 10^-e).
// The bound is loose -- measured 1e-10 where the error is 4e-7 (N = 32768, scripts/flag_study.py) -- so it is only the
// backstop for fits whose alpha solve says nothing about the conditioning (e.g. y = 0 converges at once).
static double row_flag_threshold() {
    return (NNGP_KNOB(6) >= 2 && NNGP_KNOB(6) <= 30) ? pow(10.0, -(double)NNGP_KNOB(6)) : 1e-8;
}
// NTK: predicted relative variance error after the two sweeps (k_sweep_estimate) above which the rows go on by CG.
// scripts/ntk_est_study.py, 54 fits (profiles/r2_ntk_est_study.jsonl): the estimate is within 0.4x .. 120x of the error
// wherever that exceeds 1e-8; every fit it passes is within 5e-7, the five it sends on had 7e-6 .. 6.5e-5; the
// bench-sized fits (N = 4096 .. 16384) sit at 3.5e-9 .. 8.2e-8.
constexpr double kSweepEstThr = 3e-7;

// Stage 1: argument checks, the call's facts, capacity.  (no rows: c.mt == 0 and nothing is allocated)
static int predict_open(nngp_model* m, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var_or_cov,
                        hipStream_t s, PredictCall& c) {
    NNGP_REQUIRE(m != nullptr && m->alpha_solve.plan.solved, "predict: fit the model first");
    NNGP_REQUIRE(cov_mode >= NNGP_COV_NONE && cov_mode <= NNGP_COV_FULL, "predict: bad cov_mode");
    NNGP_REQUIRE(mean != nullptr && (cov_mode == NNGP_COV_NONE || var_or_cov != nullptr), "predict: NULL output");
    c.on_train = (x_test == nullptr);
    if (c.on_train) mt = m->n;
    NNGP_REQUIRE(mt >= 0, "predict: negative row count");
    NNGP_REQUIRE(!m->k64_partial || (cov_mode == NNGP_COV_NONE && !c.on_train),
                 "predict: this model holds only its own kernel rows (row-sharded layout): it serves means of test rows; covariances are "
                 "formed by the caller from nngp_model_apply_factor and its row block (shard32.py)");
    c.s = s; c.mt = mt; c.mp = round_up(mt, TB); c.mean = mean; c.var_or_cov = var_or_cov;
    c.xt = c.on_train ? m->x : x_test; c.qt = m->q; c.ktd = m->k64;
    c.compact_train = c.on_train && m->ld != m->np;
    c.is_ntk = (m->get == NNGP_GET_NTK);
    c.want_cov = (cov_mode != NNGP_COV_NONE); c.full = (cov_mode == NNGP_COV_FULL);
    c.serving = m->serving_ready && !c.is_ntk;
    if (mt == 0) return 0;
    return ensure_predict_capacity(m, mt, !c.on_train || c.compact_train);
}

// Stage 4: the cross kernel of `get` (the mean is mu = K_td alpha, float64), or the compact copy of K_dd for x_test = None
static int build_cross_kernel(nngp_model* m, PredictCall& c) {
    const int64_t np = m->np;
    if (!c.on_train) {
        NNGP_TRY(launch_row_sqnorm(c.xt, c.mt, m->d, m->xt_q, c.s));
        c.qt = m->xt_q;
        NNGP_TRY(build_cross(m, c.xt, c.qt, c.mt, c.mp, !c.is_ntk, m->ktd64, c.s));
        c.ktd = m->ktd64;
    }
    if (c.compact_train) {
        NNGP_HIP_CHECK(hipMemsetAsync(m->ktd64, 0, sizeof(double) * c.mp * np, c.s));
        NNGP_HIP_CHECK(hipMemcpy2DAsync(m->ktd64, sizeof(double) * np, m->k64, sizeof(double) * m->ld, sizeof(double) * np, c.mt,
                                        hipMemcpyDeviceToDevice, c.s));
        c.ktd = m->ktd64;
    }
    return 0;
}

// ---- stage 6: the covariance, one function per case (form_covariance chooses) ----

static int build_ktt(nngp_model* m, const PredictCall& c) {  // NNGP K_tt [mt, mt] into ktt64 (ld = mp)
    BuildArgs a = symmetric_build_args(c.xt, c.qt, c.mt, m->d);
    a.ld64 = a.ld32 = c.mp;
    a.nngp64 = m->ktt64;
    return launch_kernel_build(a, m->arch, c.s);
}

// z64 ~ rows of K_td (K + reg I)^-1 [and r64 = their residual]: float32 solves + float64 sweeps, or -- serving mode --
// one product with the explicit inverse.  Either way z64 only has to be GOOD, not exact: the second-order formulas
// of the callers square its error.  (K_td X alone would not do: k^T X k cancels to the variance from terms 1e3..1e6 larger,
// and no float64 inverse is accurate to that.)
static int solve_cross_rows(nngp_model* m, const PredictCall& c, int sweeps, bool final_residual, ResidualNote* note = nullptr) {
    const int64_t np = m->np;
    if (!c.serving) return refined_solve_rows(m, c.ktd, c.mp, sweeps, final_residual, c.s, false, note);
    NNGP_TRY(launch_gemm_nt_f64(m->z64, np, nullptr, 0, c.ktd, np, m->ainv64, np, c.mp, np, np, 1.0, 0.0, c.s));
    if (m->serving_weak) {  // ill-conditioned fit: X is less accurate; one correction step with X as the solver
        NNGP_TRY(residual_rows(m, m->r64, c.ktd, m->z64, c.mp, c.s, false, note));
        NNGP_TRY(launch_gemm_nt_f64(m->z64, np, m->z64, np, m->r64, np, m->ainv64, np, c.mp, np, np, 1.0, 1.0, c.s));
    }
    if (final_residual) NNGP_TRY(residual_rows(m, m->r64, c.ktd, m->z64, c.mp, c.s, false, note));
    return 0;
}

// float32 only (level 0): V^T = K_td L^-T, cov = K_tt - V^T V  (fast; error ~ cond * eps32 relative to the prior)
static int cov_float32_only(nngp_model* m, PredictCall& c) {
    const int64_t np = m->np, mt = c.mt, mp = c.mp;
    NNGP_TRY(launch_convert_f64_f32(c.ktd, np, m->b32, np, mp, np, mp, np, c.s));
    NNGP_TRY(apply_forward_f32(m, mp, c.s));
    if (!c.full) return launch_row_sqsum_f32(m->b32, np, mt, np, m->tt_diag, c.var_or_cov, c.s);
    NNGP_TRY(build_ktt(m, c));
    NNGP_TRY(launch_gemm_nt_f32(m->vvt32, mp, m->b32, np, m->b32, np, mp, mp, np, 1.0f, 0.0f, false, c.s));
    return launch_cov_finish(m->ktt64, mp, m->vvt32, mp, mt, c.var_or_cov, c.s);
}

// NNGP diag at level 1: ONE float64 product and three triangular solves (the default).  With z0 = M^-1 k from the float32 factor
// M = L L^T and r0 = k - A z0:   k^T A^-1 k = z0.(k + r0) + e0^T A e0   exactly, for whatever z0 the solves
// returned, and   e0^T A e0 = r0^T A^-1 r0 ~ r0^T M^-1 r0 = |L^-1 r0|^2   -- a forward solve only, and only the
// correction term (<~ 1e-2 of the variance) depends on it.  Measured at N = 32768 against level 4: 2.1e-6 worst
// relative error (level 2: 4.2e-7 for one more solve pair and half a float64 product; the formula without the
// last term, z0.(k + r0) via the quadratic form alone: 4.7e-3 -- e0^T A e0 is NOT negligible).
// (an int8 residual's combination pass also leaves z.(k + r0), z.r0, the statistics of z and float32(r0): I8Fuse)
static int cov_nngp_diag_level1(nngp_model* m, PredictCall& c) {
    const int64_t np = m->np, mt = c.mt, mp = c.mp;
    ResidualNote note;
    note.want_fused_rows = true;
    NNGP_TRY(solve_cross_rows(m, c, 0, true, &note));
    if (note.used_int8) c.used_i8 = true;
    c.z_valid = true;
    if (note.fused) {
        NNGP_TRY(launch_i8s_rowstat_finish(m->i8.work.rowpart, np, mt, m->tt_diag, c.var_or_cov, m->rows.delta, m->rows.zstat, c.s));
    } else {
        NNGP_TRY(launch_rowdot_f64(m->z64, c.ktd, 1.0, m->r64, np, mt, np, m->tt_diag, -1.0, c.var_or_cov, c.s));
        NNGP_TRY(launch_rowdot_f64(m->z64, nullptr, 0.0, m->r64, np, mt, np, nullptr, 1.0, m->rows.delta, c.s,
                                   c.used_i8 ? m->rows.zstat : nullptr));
        NNGP_TRY(launch_convert_f64_f32(m->r64, np, m->b32, np, mp, np, mp, np, c.s));
    }
    NNGP_TRY(apply_forward_f32(m, mp, c.s));
    NNGP_TRY(launch_row_sqsum_f32(m->b32, np, mt, np, c.var_or_cov, c.var_or_cov, c.s));
    c.check = CovCheck::NngpDiagLevel1;
    if (c.used_i8) NNGP_TRY(record_i8_guard_estimate(m, c));
    return launch_rows_prepare(m->rows.delta, m->tt_diag, c.var_or_cov, nullptr, 0, row_flag_threshold(), mt, m->rows.tol,
                               m->rows.live + 1, c.s);
}

// NNGP diag, a handful of queries against the explicit inverse: two passes over N x N float64 matrices (X, then K) per
// group of 8 queries, both HBM-bound; var = K_tt - (2 z.k - z^T (K + reg I) z).  (Measured, ms per call,
// streamed groups / 128-row MFMA GEMM -- N = 10800: 8 queries 0.62 / 3.06; N = 32768: 4.07 / 9.29.)
static int cov_nngp_diag_few_queries(nngp_model* m, PredictCall& c) {
    const int64_t np = m->np, mt = c.mt;
    c.z_valid = true;
    for (int64_t g = 0; g < mt; g += 8) {
        const int64_t gm = (mt - g < 8) ? mt - g : 8;
        NNGP_TRY(launch_skinny_nt_f64(m->z64 + g * np, np, nullptr, 0, c.ktd + g * np, np, m->ainv64, np, gm, np, np, 1.0, 0.0, c.s));
        NNGP_TRY(launch_skinny_nt_f64(m->r64 + g * np, np, nullptr, 0, m->z64 + g * np, np, m->k64, m->ld, gm, np, np, 1.0, 0.0, c.s));
    }
    NNGP_TRY(launch_axpby_mat(m->r64, -1.0, m->z64, -m->reg, np, mt, np, c.s));
    return launch_rowdot_f64(m->z64, c.ktd, 2.0, m->r64, np, mt, np, m->tt_diag, -1.0, c.var_or_cov, c.s);
}

// NNGP diag, second order (level >= 2): z.(k + r) = 2 z.k - z^T (K + reg I) z, and the quadratic form needs only the lower triangle of
// the symmetric K: W = 2 Z strict_lower_blocks(K) + Z diag_blocks(K) -- HALF the float64 product that the
// full residual costs (kmode 1 / 2 of the float64 GEMM), then var = K_tt - z.(2 k - W - reg z)
static int cov_nngp_diag_second_order(nngp_model* m, PredictCall& c, int level) {
    const int64_t np = m->np, mt = c.mt, mp = c.mp;
    NNGP_TRY(solve_cross_rows(m, c, level - 1, false));
    c.z_valid = true;
    NNGP_TRY(launch_gemm_nt_f64(m->r64, np, nullptr, 0, m->z64, np, m->k64, m->ld, mp, np, np, 2.0, 0.0, c.s, 1));
    NNGP_TRY(launch_gemm_nt_f64(m->r64, np, m->r64, np, m->z64, np, m->k64, m->ld, mp, np, np, 1.0, 1.0, c.s, 2));
    NNGP_TRY(launch_axpby_mat(m->r64, -1.0, m->z64, -m->reg, np, mp, np, c.s));
    NNGP_TRY(launch_rowdot_f64(m->z64, c.ktd, 2.0, m->r64, np, mt, np, m->tt_diag, -1.0, c.var_or_cov, c.s));
    // delta = z.k - z^T A z: the first-order term that the formula above cancels (preconditioner_is_weak reads the flags)
    NNGP_TRY(launch_rowdot_f64(m->z64, c.ktd, 1.0, m->r64, np, mt, np, nullptr, 1.0, m->rows.delta, c.s));
    if (c.serving) return 0;  // the inverse was refined to convergence when it was built
    c.check = CovCheck::NngpDiag;
    return launch_rows_prepare(m->rows.delta, m->tt_diag, c.var_or_cov, nullptr, 0, row_flag_threshold(), mt, m->rows.tol,
                               m->rows.live + 1, c.s);
}

// The NNGP covariance from z64 and the residual r of its rows: issued by the general case, and again after a continuation.
// Variances: var_i = K_tt,ii - z_i . (k_i + r_i)   (r = NULL: first order, z_i . k_i alone)
static int nngp_diag_from_rows(nngp_model* m, const PredictCall& c, const double* r) {
    return launch_rowdot_f64(m->z64, c.ktd, 1.0, r, m->np, c.mt, m->np, m->tt_diag, -1.0, c.var_or_cov, c.s);
}
// Full: cov = K_tt - Z G^T, G = K_td + R formed in r64 (with_residual) or G = K_td.  The re-formation after a continuation differs
// in one thing: it does not rebuild K_tt, which ktt64 still holds.
static int nngp_full_from_rows(nngp_model* m, const PredictCall& c, bool with_residual, bool rebuild_ktt) {
    const int64_t np = m->np, mp = c.mp;
    const double* g = c.ktd;
    if (with_residual) {
        NNGP_TRY(launch_axpby_mat(m->r64, 1.0, c.ktd, 1.0, np, mp, np, c.s));  // G = K_td + R
        g = m->r64;
    }
    if (rebuild_ktt) NNGP_TRY(build_ktt(m, c));
    NNGP_TRY(launch_gemm_nt_f64(m->covp64, mp, m->ktt64, mp, m->z64, np, g, np, mp, mp, np, -1.0, 1.0, c.s));
    return launch_copy_mat_f64(m->covp64, mp, c.var_or_cov, c.mt, c.s);
}

// NNGP general: first-order diag, and the full covariance at either order
static int cov_nngp_general(nngp_model* m, PredictCall& c, int level) {
    const int64_t np = m->np, mt = c.mt;
    const bool second_order = level >= 2;
    NNGP_TRY(solve_cross_rows(m, c, second_order ? level - 1 : 1, second_order));
    c.z_valid = true;
    if (!c.full) return nngp_diag_from_rows(m, c, second_order ? m->r64 : nullptr);
    if (second_order) {
        NNGP_TRY(launch_rowdot_f64(m->z64, c.ktd, 1.0, m->r64, np, mt, np, m->tt_diag, -1.0, m->rows.var, c.s));
        NNGP_TRY(launch_rowdot_f64(m->z64, nullptr, 0.0, m->r64, np, mt, np, nullptr, 1.0, m->rows.delta, c.s));
        NNGP_TRY(launch_rows_prepare(m->rows.delta, m->tt_diag, m->rows.var, nullptr, 0, row_flag_threshold(), mt, m->rows.tol,
                                     m->rows.live + 1, c.s));
        c.check = c.serving ? CovCheck::None : CovCheck::NngpFull;
    }
    return nngp_full_from_rows(m, c, second_order, true);
}

// NTK: the covariance from z64 = Theta_td (Theta_dd + reg I)^-1; K_tt already in ktt64 (full).  Runs again after a continuation.
static int ntk_finish(nngp_model* m, const PredictCall& c) {
    const int64_t np = m->np, mt = c.mt, mp = c.mp;
    NNGP_TRY(kaux_product_rows(m, m->r64, m->z64, mp, c.s));  // W = Z K_dd
    if (!c.full)  // var_i = K_tt,ii + z_i . (w_i - 2 k_i)
        return launch_rowdot_f64(m->z64, c.ktd_nngp, -2.0, m->r64, np, mt, np, m->tt_diag, 1.0, c.var_or_cov, c.s);
    NNGP_TRY(launch_axpby_mat(m->r64, 1.0, c.ktd_nngp, -1.0, np, mp, np, c.s));  // G = W - K_td
    NNGP_TRY(launch_gemm_nt_f64(m->covp64, mp, m->ktt64, mp, m->r64, np, m->z64, np, mp, mp, np, 1.0, 1.0, c.s));
    NNGP_TRY(launch_gemm_nt_f64(m->covp64, mp, m->covp64, mp, m->z64, np, c.ktd_nngp, np, mp, mp, np, -1.0, 1.0, c.s));
    return launch_copy_mat_f64(m->covp64, mp, c.var_or_cov, mt, c.s);
}

// NTK (train.py --kernel_type ntk): with Z = Theta_td (Theta_dd + reg I)^-1,
//   cov = K_tt + Z K_dd Z^T - (K_td Z^T + h.c.),  K = NNGP kernels.
static int cov_ntk(nngp_model* m, PredictCall& c) {
    const int64_t n = m->n, np = m->np, mt = c.mt, mp = c.mp;
    if (!m->aux_ready) {  // the NNGP kernel of the training rows, unless the fit's own build has written it
        if (m->kaux64 == nullptr) {
            NNGP_HIP_CHECK(hipDeviceSynchronize());
            NNGP_TRY(dev_alloc(&m->kaux64, m->np_cap * m->np_cap));
        }
        BuildArgs a = symmetric_build_args(m->x, m->q, n, m->d);
        a.ld64 = a.ld32 = np;
        a.nngp64 = m->kaux64;
        a.no_comp = 1;  // the same bits as when the fit's own build writes it (nngp_model_build_rows)
        NNGP_TRY(launch_kernel_build(a, m->arch, c.s));
        NNGP_TRY(launch_zero_pad_f64(m->kaux64, np, n, np, c.s));
        m->aux_ready = true;
        m->i8.work.aux.ready = false;
    }
    const double* ktd_n = m->kaux64;  // NNGP cross kernel; x_test=None: K_dd itself
    if (!c.on_train) {
        if (mp > m->ktd_aux_cap) {
            NNGP_HIP_CHECK(hipDeviceSynchronize());
            dev_free(m->ktd_aux);
            NNGP_TRY(dev_alloc(&m->ktd_aux, mp * m->np_cap));
            m->ktd_aux_cap = mp;
        }
        NNGP_TRY(build_cross(m, c.xt, c.qt, mt, mp, true, m->ktd_aux, c.s));
        ktd_n = m->ktd_aux;
    }
    NNGP_TRY(refined_solve_rows(m, c.ktd, mp, ntk_sweeps(m), false, c.s, m->var_refine >= 1));
    c.ktd_nngp = ktd_n;
    c.z_valid = true;
    if (c.full) NNGP_TRY(build_ktt(m, c));
    if (m->var_refine >= 1) c.check = CovCheck::Ntk;
    NNGP_TRY(ntk_finish(m, c));
    if (c.check == CovCheck::Ntk) {
        // b32 still holds the second correction; r64 = Z K_dd (diag) or Z K_dd - K_td (full): see ntk_finish
        NNGP_TRY(launch_rows_dvar(m->b32, m->r64, c.full ? nullptr : c.ktd_nngp, -1.0, np, mt, np, m->rows.coef, c.s));
        NNGP_TRY(launch_sweep_estimate(m->rows.var, m->rows.delta, m->rows.tol, m->rows.coef, c.var_or_cov, c.full ? mt + 1 : 1,
                                       mt, reinterpret_cast<double*>(m->rows.live + 2), c.s));
    }
    return 0;
}

// Stage 6.  The covariance does not depend on alpha: it is enqueued first, then the deferred CG solve runs on its own stream
// (overlapping it), and the mean follows once alpha is there.  Levels >= 1 leave in c.check what is looked at afterwards: whether
// the fixed number of correction sweeps was enough (preconditioner_is_weak).  Runs a second time when the int8 guard distrusts
// the first result (first_guard_verdict).
static int form_covariance(nngp_model* m, PredictCall& c) {
    if (c.full) NNGP_TRY(ensure_full_cov_capacity(m, c.mt));
    NNGP_TRY(launch_kernel_diag(c.xt, c.qt, c.mt, m->d, m->arch, m->tt_diag, nullptr, c.s));  // NNGP K(x_t, x_t)
    if (!c.is_ntk && m->var_refine == 0) return cov_float32_only(m, c);
    if (!c.serving && needs_lt32(solve_path(m, c.mp))) NNGP_TRY(ensure_lt(m, c.s));  // float32 L^T: only the float32 solve path reads it
    NNGP_TRY(ensure_refine_capacity(m, c.mp));
    if (c.is_ntk) return cov_ntk(m, c);
    // NNGP: cov_ij = K_tt,ij - k_i^T A^-1 k_j with Z ~ K_td A^-1 (float32 solve + float64 correction sweeps).
    //   level 1: one sweep, cov = K_tt - sym(Z K_dt)  (error ~ rho * float32 error); diag only: cov_nngp_diag_level1
    //   level L >= 2: L-1 sweeps, then with R = K_td - Z A:  k_i^T A^-1 k_j = sym(z_i . (k_j + r_j)) + O(err^2)
    // the explicit inverse needs the second-order formula; the full covariance has no cheap remainder estimate: level >= 2
    const int level = ((c.serving || (c.full && m->var_refine == 1)) && m->var_refine < 2) ? 2 : m->var_refine;
    if (!c.full && level == 1) return cov_nngp_diag_level1(m, c);
    if (!c.full && c.serving && c.mt <= (m->np <= 16384 ? 32 : 16) && !m->serving_weak) return cov_nngp_diag_few_queries(m, c);
    if (!c.full && level >= 2) return cov_nngp_diag_second_order(m, c, level);
    return cov_nngp_general(m, c, level);
}

// Stage 9.  Were the fixed sweeps enough?  Two signs that the float32 factor is a weak preconditioner: the alpha solve needed
// many CG iterations, or a row's first-order term is too large for its second-order error to be small (k_rows_prepare).
// Then the rows go on by preconditioned CG until each has converged, and the covariance is formed again.
// (debug key 6 = 1: fixed sweeps only.)
//
// The iteration count from which a fit counts as weak.  Iterations of the alpha solve against the variance error of the fixed
// sweeps, 72 random fits of tests/test_gpu_parity.py (N <= 5200): <= 5: <= 1e-7, 6: <= 1e-5, 7: <= 5e-5, >= 9: up to 8e-2; the
// bench sizes need 5 (N = 32768) and 6 (N = 65536).
static int weak_iters_threshold(CovCheck check) {
    // NTK covariance has no second-order formula: stricter.
    // (NTK: two sweeps leave ~rho^3 where the NNGP formula leaves ~rho^4: 6 iterations ~ 2e-4, 5 ~ 6e-6, 4 ~ 4e-8 -- the
    // threshold was 4 until round 2, which sent the N = 16384 bench config (4 iterations, 3.6e-8 after the sweeps) through
    // three continuation steps, 78 ms per predict instead of 37)
    if (check == CovCheck::Ntk) return 6;
    // (round 3: the full covariance continues from 7 iterations too -- a 7-iteration fit of the large-N sweep, N = 5007, d = 3, left 2.1e-4 in
    // its diagonal where the diag path, which already continued from 7, was at 8e-9)
    return (check == CovCheck::NngpDiagLevel1 || check == CovCheck::NngpFull) ? 7 : 8;
}
static int preconditioner_is_weak(nngp_model* m, const PredictCall& c, bool* weak_out) {
    bool weak = m->alpha_solve.plan.iters >= weak_iters_threshold(c.check) || m->reg_fac > m->reg;
    if (!weak && c.check == CovCheck::Ntk) {
        // NTK below 6 iterations: the count alone does not separate 4e-8 (N = 16384, d = 256: 4 iterations) from 5e-5
        // (N = 907, d = 2, four layers, diag_reg 1e-4: also 4).  What the two sweeps removed does: 16-byte read-back.
        NNGP_HIP_CHECK(hipMemcpyAsync(m->rows.host + 2, m->rows.live + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, c.s));
        NNGP_HIP_CHECK(hipStreamSynchronize(c.s));
        memcpy(&m->sweep_est, m->rows.host + 2, sizeof(double));
        memcpy(&m->sweep_est_var, m->rows.host + 4, sizeof(double));
        weak = !(m->sweep_est_var <= kSweepEstThr);
    }
    // the row flag is the backstop for fits whose alpha solve says nothing (it converged in < 3 iterations, e.g.
    // y = 0); otherwise the iteration count decides and the call stays asynchronous
    if (!weak && c.check != CovCheck::Ntk && m->alpha_solve.plan.iters < 3) {
        NNGP_HIP_CHECK(hipMemcpyAsync(m->rows.host + 1, m->rows.live + 1, sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
        NNGP_HIP_CHECK(hipStreamSynchronize(c.s));
        weak = m->rows.host[1] > 0;
    }
    *weak_out = weak;
    return 0;
}

// ... and the continuation: r64 back to the float64 residual of z64, the rows on by CG, the covariance again from what they converged to
static int continue_rows_by_cg(nngp_model* m, PredictCall& c) {
    const int64_t np = m->np, mt = c.mt, mp = c.mp;
    if (c.check == CovCheck::NngpFull) {
        NNGP_TRY(launch_axpby_mat(m->r64, 1.0, c.ktd, -1.0, np, mp, np, c.s));  // back from G = K_td + R to R
    } else if (c.check == CovCheck::NngpDiagLevel1) {
        // level 1: r64 is the residual of z64 already -- but if it came from the int8 product, its error floor (~1e-3 of it)
        // would stay in the recursively updated residual and in the rows the CG converges to (seen in the parity sweep:
        // continued rows at 1e-6 .. 9e-6 instead of 1e-9): the continuation starts from the float64 residual proper
        if (use_i8s(m, mp)) NNGP_TRY(residual_rows(m, m->r64, c.ktd, m->z64, mp, c.s, false));
    } else {
        NNGP_TRY(residual_rows(m, m->r64, c.ktd, m->z64, mp, c.s, false));
    }
    if (c.check == CovCheck::Ntk)  // tolerance from what the second sweep did to the variance (rows.tol holds z . k)
        NNGP_TRY(launch_rows_prepare_ntk(m->rows.delta, m->rows.coef, m->rows.tol, c.var_or_cov, c.full ? mt + 1 : 1, mt,
                                         NNGP_KNOB(6) >= 2 ? pow(10.0, -(double)NNGP_KNOB(6)) : 1e-10, c.s));
    NNGP_TRY(rows_pcg_continue(m, mp, continuation_budget(m), c.s));
    if (c.check == CovCheck::Ntk) return ntk_finish(m, c);
    if (!c.full) return nngp_diag_from_rows(m, c, m->r64);
    return nngp_full_from_rows(m, c, true, false);
}

// Stage 10: mu = K_td alpha, and its correction when the alpha CG stopped early
static int write_mean(nngp_model* m, const PredictCall& c) {
    const int64_t n = m->n, np = m->np, mt = c.mt;
    for (int col = 0; col < m->ny; ++col)
        NNGP_TRY(launch_gemv_f64(c.ktd, np, mt, n, m->alpha + col, m->ny, c.mean + col, m->ny, 0.0, c.s));
    if (m->alpha_solve.plan.partial && c.z_valid) {
        // the CG stopped at a_k with residual r_k = y - A a_k (still in the CG workspace):
        //   K_td A^-1 y = K_td a_k + (K_td A^-1) r_k = K_td a_k + Z r_k + (K_td A^-1 - Z) r_k,
        // and the last term is the product of two small errors (rows: <= 1e-3 relative; r_k: <= 1e-6 |y|)
        NNGP_TRY(launch_gemv_f64(m->z64, np, mt, n, m->pcg.r, 1, m->rows.delta, 1, 0.0, c.s));
        NNGP_TRY(launch_axpby_mat(c.mean, 1.0, m->rows.delta, 1.0, mt, 1, mt, c.s));
    }
    return 0;
}

}  // namespace nngp

extern "C" {

// Serving mode (the reference's Estimator keeps its Cholesky factor and calls cho_solve per query
// batch, estimator.py:34-67).  Builds X = (K + reg I)^-1 explicitly in float64: rows of the identity, 1024 at a time,
// through the same float32-solve + float64-correction machinery as the covariance (two sweeps; by CG to convergence when
// the factor is a weak preconditioner), then X <- (X + X^T) / 2.  Cost ~ N/1024 covariance-sized solves, once per fit;
// afterwards predict forms Z = K_td X with ONE float64 product and no solves.
int nngp_model_prepare_serving(nngp_model* m, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->alpha_solve.plan.solved, "prepare_serving: fit the model first");
    NNGP_REQUIRE(!m->k64_partial, "prepare_serving: not with the row-sharded layout (the model holds only its own kernel rows)");
    if (m->get != NNGP_GET_NNGP) return 0;  // the NTK covariance has no second-order formula to absorb the inverse's error
    NNGP_TRY(run_pending_solve(m, s, true));  // its iteration count says how good the preconditioner is
    const int64_t n = m->n, np = m->np;
    const int64_t blk = np < 1024 ? np : 1024;
    NNGP_TRY(ensure_predict_capacity(m, blk, true));
    NNGP_TRY(ensure_refine_capacity(m, blk));
    if (needs_lt32(solve_path(m, blk))) NNGP_TRY(ensure_lt(m, s));
    if (m->ainv64 == nullptr) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        NNGP_TRY(dev_alloc(&m->ainv64, m->np_cap * m->np_cap));
    }
    const bool weak = m->alpha_solve.plan.iters >= 8 || m->reg_fac > m->reg;
    // The serving predictions SQUARE the inverse's error (second-order formula) on top of a cancellation of 1e3 .. 1e6: the
    // inverse has to converge to float64 accuracy proper, and the COARSE int8 residual's floor (2^-32 of the row maxima) stops the
    // sweeps four digits short of it -- measured: 4e-3 in the serving variances at N = 2500 against 1e-7 (scripts/i8s_hard_case.py).
    // Nor the FINE product: an inverse refined against it serves variances at 1e-9 .. 6e-9 of level 3 where the float64 pipe's
    // reaches 2e-11 .. 5e-11, for 10-20 % of the build time (scripts/i8s_serving_build.py).
    ScopedFlag suspend(m->i8.suspended);
    for (int64_t r0 = 0; r0 < n; r0 += blk) {
        const int64_t rows = (n - r0 < blk) ? n - r0 : blk, rp = round_up(rows, TB);
        NNGP_TRY(launch_identity_rows(m->ktd64, np, np, r0, rows, rp, s));
        // three sweeps: the rows' errors add up coherently in Z = K_td X (two left 1.4e-3 in the variance at N = 32768)
        NNGP_TRY(refined_solve_rows(m, m->ktd64, rp, 3, weak, s));
        if (weak) {  // tolerance relative to the row's energy z.e = X_ii
            NNGP_TRY(launch_rowdot_f64(m->z64, m->ktd64, 1.0, nullptr, np, rows, np, nullptr, 1.0, m->rows.delta, s));
            NNGP_TRY(launch_rows_prepare(nullptr, nullptr, nullptr, m->rows.delta, 1, 0.0, rows, m->rows.tol, m->rows.live + 1, s));
            NNGP_TRY(rows_pcg_continue(m, rp, continuation_budget(m), s));
        }
        NNGP_HIP_CHECK(hipMemcpyAsync(m->ainv64 + r0 * np, m->z64, sizeof(double) * rows * np, hipMemcpyDeviceToDevice, s));
    }
    if (np > n) NNGP_HIP_CHECK(hipMemsetAsync(m->ainv64 + n * np, 0, sizeof(double) * (np - n) * np, s));
    NNGP_TRY(launch_symmetrize_f64(m->ainv64, np, np, s));
    m->serving_ready = true;
    m->serving_weak = weak;
    return 0;
}

// The posterior of one batch of queries, stage by stage (the stages: above, in this order; 2, 5 and 8 -- the int8 residual's early
// plane cut and its guard -- in residual_i8.hip)
static int predict_impl(nngp_model* m, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var_or_cov,
                        void* stream) {
    PredictCall c;
    NNGP_TRY(predict_open(m, x_test, mt, cov_mode, mean, var_or_cov, (hipStream_t)stream, c));
    if (c.mt == 0) return 0;
    NNGP_TRY(cut_planes_early(m, c));
    NNGP_TRY(tri_fork(m, c.s));  // first predict of a fit: the factor's inverted blocks are built beside the cross-kernel build
    NNGP_TRY(build_cross_kernel(m, c));
    take_in_guard_word(m);
    c.used_i8 = false;
    open_gate_epoch(m);
    if (c.want_cov) NNGP_TRY(form_covariance(m, c));
    NNGP_TRY(run_pending_solve(m, c.s, true, c.z_valid));
    bool redo_cov = false;
    NNGP_TRY(first_guard_verdict(m, c, &redo_cov));
    if (redo_cov) NNGP_TRY(form_covariance(m, c));  // the int8 guard distrusts the first result
    m->cov_iters = 0;
    m->sweep_est = m->sweep_est_var = -1.0;
    if (c.check != CovCheck::None && NNGP_KNOB(6) != 1) {
        bool weak = false;
        NNGP_TRY(preconditioner_is_weak(m, c, &weak));
        if (weak) NNGP_TRY(continue_rows_by_cg(m, c));
    }
    NNGP_TRY(write_mean(m, c));
    return record_predict_end(m, c.s);
}

int nngp_model_predict(nngp_model* m, const double* x_test, int64_t mt, int32_t cov_mode, double* mean,
                       double* var_or_cov, void* stream) {
    const int rc = predict_impl(m, x_test, mt, cov_mode, mean, var_or_cov, stream);
    // whatever path the predict took, the caller's stream leaves behind the build of the inverted blocks it may have forked (tri_fork)
    if (m != nullptr && !m->tri_stale && m->tri_pending) (void)hipStreamWaitEvent((hipStream_t)stream, m->ev_tri, 0);
    return rc;
}

int nngp_model_apply_factor(nngp_model* m, float* b, int64_t rows, int32_t mode, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->factored, "apply_factor: fit the model first");
    NNGP_REQUIRE(b != nullptr && rows > 0 && (mode == 0 || mode == 1), "apply_factor: bad arguments");
    NNGP_TRY(ensure_predict_capacity(m, rows, false));
    const int64_t mp = round_up(rows, TB), np = m->np, n = m->n;
    NNGP_HIP_CHECK(hipMemsetAsync(m->b32, 0, sizeof(float) * mp * np, s));
    NNGP_HIP_CHECK(hipMemcpy2DAsync(m->b32, sizeof(float) * np, b, sizeof(float) * n, sizeof(float) * n, rows, hipMemcpyDeviceToDevice, s));
    if (mode == 0) {
        NNGP_TRY(apply_forward_f32(m, mp, s));
    } else {
        if (needs_lt32(solve_path(m, mp))) NNGP_TRY(ensure_lt(m, s));  // float32 L^T: only the float32 solve path reads it
        NNGP_TRY(apply_inverse_f32(m, mp, s));
    }
    NNGP_HIP_CHECK(hipMemcpy2DAsync(b, sizeof(float) * n, m->b32, sizeof(float) * np, sizeof(float) * n, rows, hipMemcpyDeviceToDevice, s));
    return 0;
}
}  // extern "C"
