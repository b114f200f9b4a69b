// Look-ahead schedules of the blocked Cholesky (host code only: the leaf kernels and the plain recursion are in potrf.hip).
//   potrf_lookahead_f32      picks the schedule: the grouped form (product), the grouped form with the panel solves off the update
//                            stream (knobs build, debug key 8), or its own one-column loop
//   potrf_panel_f32 / potrf_update_f32 / potrf_update_cols_f32   the same steps by block column, for the multi-GPU factorisation
// Every step that more than one of them takes -- the float32 lead pass, the update timer, the solve of the rows below a diagonal
// block, the workspace test, the far update's shares and regions, fork and join -- is a file-local function below, once.
#include <cstdio>
#include <new>

#include "common.h"

namespace nngp {

// ---- look-ahead driver -----------------------------------------------------------------------------------
// The recursion of potrf.hip runs ~2300 dependent launches; about a third of its wall time is spent in kernels too small
// to fill 256 CUs (leaves, 128-wide triangular solves).  The look-ahead form cuts the matrix into block columns of
// width nb and uses two HIP streams: the high-priority "panel" stream factors block column k+1 (small kernels) while
// the low-priority "update" stream applies block column k to the rest of the trailing matrix (large SYRKs), so the
// small kernels run in the shadow of the large ones instead of in sequence with them.
//   panel  : wait col[k-1]; potrf(A_kk) (recursive chain of small kernels); record panel[k]
//   update : wait panel[k]; trsm(rows below); update diagonal block k+1 first; record col[k]; update the rest
int lookahead_create(LookAhead** out) {
    LookAhead* la = new (std::nothrow) LookAhead();
    NNGP_REQUIRE(la != nullptr, "lookahead_create: out of memory");
    // Optional CU partition (timing experiment, NNGP debug key 5 = 2): the panel stream owns `panel_cus` compute units,
    // the update stream the rest.  Measured at N = 32768: 138.6 ms (32 CUs) / 202 ms (16) / 140 ms (64) against 124.2 ms
    // for plain priority streams and 126.1 ms for the single-stream recursion -- so the default is priority streams.
    int ncu = 256;
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
    const int panel_cus = NNGP_KNOB(4) > 0 ? NNGP_KNOB(4) : 32;
    bool masked = false;
    if (NNGP_KNOB(5) == 2 && ncu >= 64 && panel_cus < ncu) {
        const int words = (ncu + 31) / 32;
        uint32_t mp[16] = {0}, mu[16] = {0};
        // mask bit i addresses CU (i / 8) of XCD (i % 8) (measured: masks that thin out one XCD make it the straggler of
        // every GEMM), so the first 8*r bits take r CUs from every XCD
        for (int c = 0; c < ncu; ++c) (c < panel_cus ? mp : mu)[c / 32] |= (1u << (c % 32));
        if (words <= 16 && hipExtStreamCreateWithCUMask(&la->panel, words, mp) == hipSuccess) {
            if (hipExtStreamCreateWithCUMask(&la->update, words, mu) == hipSuccess) {
                masked = true;
            } else {
                (void)hipStreamDestroy(la->panel);
                la->panel = nullptr;
            }
        }
    }
    la->masked = masked;
    if (!masked) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
        // Priorities (numerically lower = higher).  With three levels or more: the diagonal-block chain and the bulk panel solves on
        // top, the trailing updates in the middle, and a lowest level for work that may only use what everything else leaves idle
        // (the `side` stream: inverted blocks, digit planes, split copies cut under the chain-bound last block columns).  The bulk
        // solves must outrank the update stream: their workgroups take the compute units a trailing-update launch gives back before
        // the next launch's persistent grid settles there.  With two levels there is no side stream.
        const bool three = least - greatest >= 2;
        const int prio_update = (three && (NNGP_KNOB(8) & 1)) ? least - 1 : least;
        if (hipStreamCreateWithPriority(&la->panel, hipStreamNonBlocking, greatest) != hipSuccess ||
            hipStreamCreateWithPriority(&la->update, hipStreamNonBlocking, prio_update) != hipSuccess) {
            set_error("lookahead_create: hipStreamCreateWithPriority failed");
            delete la;
            return -1;
        }
        // Every further stream costs: HIP multiplexes streams onto a few hardware queues, and a fifth look-ahead stream with work pending
        // on it stretched the whole factorisation by a third (measured: 40.7 -> 55 ms at N = 32768; not when profiled).  The streams of
        // the round-4 schedule only exist when that experiment is switched on.
        if (!(NNGP_KNOB(8) & 1) || hipStreamCreateWithPriority(&la->bulk, hipStreamNonBlocking, greatest) != hipSuccess) la->bulk = nullptr;
        if (!(NNGP_KNOB(8) & 1) || !three || hipStreamCreateWithPriority(&la->side, hipStreamNonBlocking, NNGP_KNOB(11) == 1 ? prio_update : NNGP_KNOB(11) == 2 ? greatest : least) != hipSuccess) la->side = nullptr;
        // (the stream of the early diagonal-block product, debug key 8 = 4, only exists when that experiment is on: every further stream
        // costs -- see the note on the side stream in DESIGN.md)
        if (!(NNGP_KNOB(8) & 4) || hipStreamCreateWithPriority(&la->aux, hipStreamNonBlocking, greatest) != hipSuccess) la->aux = nullptr;
        la->prio_levels = least - greatest + 1;
    }
    hipEvent_t* all[5] = {&la->ev_in, &la->ev_panel_done, &la->ev_update_done, &la->ev_bulk_done, &la->ev_side_done};
    for (auto e : all)
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return -1; }
    for (int i = 0; i < LookAhead::kMaxSteps; ++i) {
        // (the seven events per step of round 4's schedule with the panel solves off the update stream exist in the knobs build only:
        // that schedule never runs in the product library)
#ifdef NNGP_TIMING_KNOBS
        hipEvent_t* per[11] = {&la->ev_panel[i], &la->ev_col[i], &la->ev_chunk[i], &la->ev_helper[i], &la->ev_far[i],
                               &la->ev_near[i],  &la->ev_tc[i],  &la->ev_tb[i],    &la->ev_split[i],  &la->ev_gp[i], &la->ev_c1[i]};
#else
        hipEvent_t* per[4] = {&la->ev_panel[i], &la->ev_col[i], &la->ev_chunk[i], &la->ev_helper[i]};
#endif
        for (auto e : per)
            if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
                set_error("hipEventCreate failed");
                return -1;
            }
    }
    *out = la;
    return 0;
}

void lookahead_destroy(LookAhead* la) {
    if (!la) return;
    (void)hipStreamSynchronize(la->panel);
    (void)hipStreamSynchronize(la->update);
    if (la->bulk) (void)hipStreamSynchronize(la->bulk);
    (void)hipStreamDestroy(la->panel);
    (void)hipStreamDestroy(la->update);
    if (la->bulk) (void)hipStreamDestroy(la->bulk);
    if (la->aux) { (void)hipStreamSynchronize(la->aux); (void)hipStreamDestroy(la->aux); }
    if (la->side) { (void)hipStreamSynchronize(la->side); (void)hipStreamDestroy(la->side); }
    if (la->ev_side_done) (void)hipEventDestroy(la->ev_side_done);
    (void)hipEventDestroy(la->ev_in); (void)hipEventDestroy(la->ev_panel_done); (void)hipEventDestroy(la->ev_update_done);
    if (la->ev_bulk_done) (void)hipEventDestroy(la->ev_bulk_done);
    for (int i = 0; i < LookAhead::kMaxSteps; ++i) {
        hipEvent_t per[11] = {la->ev_panel[i], la->ev_col[i], la->ev_chunk[i], la->ev_helper[i], la->ev_far[i],
                              la->ev_near[i],  la->ev_tc[i],  la->ev_tb[i],    la->ev_split[i],  la->ev_gp[i], la->ev_c1[i]};
        for (auto e : per)
            if (e) (void)hipEventDestroy(e);
    }
    for (int i = 0; i < LookAhead::kMaxTimed; ++i) {
        if (la->tu0[i]) (void)hipEventDestroy(la->tu0[i]);
        if (la->tu1[i]) (void)hipEventDestroy(la->tu1[i]);
    }
    delete la;
}

// ---- steps the schedules share ------------------------------------------------------------------------------------------------
namespace {

// The leading columns of the factor are large and of one sign (K is a positive kernel); the float16 MFMA
// accumulator truncates toward zero, which biases long same-sign sums (-2.6e-8 relative at K = 1024 on
// positive data, nothing on mixed signs; float32 MFMA: 1e-10).  A coherent error of that size in the first
// trailing update costs two CG iterations and 40x in the refined variances, so the first `lead` columns
// of block column 0 go through the float32-MFMA kernels and the rest through the float16 pipe.  Measured at
// N = 32768 (Cholesky ms / CG iterations / level-2 variance error): lead 0: 59.8 / 7 / 1.6e-5, 128: 61.0 / 6 /
// 4.1e-7, 256: 61.9 / 5 / 4.0e-7, 512: 63.6 / 6, whole column: 63.6 / 5 / 4.0e-7.  Round 2 (scripts/lead_study.py;
// level-1 variance against level 3): 0: 47.1 / 7 / 7.5e-5, 32: 47.6 / 6 / 1.16e-6, 64: 47.8 / 5 / 1.13e-6, 128: 48.0 /
// 5 / 1.13e-6, 256: 48.8 / 6 / 1.17e-6 -- the bias sits in the first few (dominant, one-signed) columns: 64 it is.
// Every schedule and the block-column ABI take the width from here.
constexpr int64_t kLeadF32Cols = 64;

// May a factorisation of n rows with block columns (panels) of width kw use the split-float16 workspace?  (Debug key 2 = 2: the
// float32-MFMA updates, for A/B timing.)  What an entry point asks beyond this stands at its call site.
bool h3_workspace_ok(const SplitWork* sw, int64_t n, int64_t kw) {
    return sw != nullptr && sw->planes != nullptr && sw->k_cap == kw && sw->rows_cap >= n + 256 && NNGP_KNOB(2) != 2;
}

// Block-column ABI: the rows below panel [po, po + pw) are split into its planes (rows at their global index) when its first
// update arrives, unless the panel solve already left them there.
int ensure_panel_split(SplitWork* sw, const float* a, int64_t ld, int64_t n, int64_t po, int64_t pw, hipStream_t s) {
    if (sw->split_panel == po) return 0;
    const int64_t ldp = 4 * sw->k_cap;
    char* col = sw->planes + (po / pw) * sw->col_stride;
    NNGP_TRY(launch_split_rows(a + (po + pw) * ld + po, ld, n - po - pw, pw, sw->scale, col + (po + pw) * ldp, ldp, s));
    sw->split_panel = po;
    return 0;
}

// The schedule's streams start behind the caller's stream ...
int lookahead_fork(LookAhead* la, hipStream_t user, hipStream_t extra = nullptr) {
    NNGP_HIP_CHECK(hipEventRecord(la->ev_in, user));
    NNGP_HIP_CHECK(hipStreamWaitEvent(la->panel, la->ev_in, 0));
    NNGP_HIP_CHECK(hipStreamWaitEvent(la->update, la->ev_in, 0));
    if (extra != nullptr) NNGP_HIP_CHECK(hipStreamWaitEvent(extra, la->ev_in, 0));
    return 0;
}

// ... and the caller's stream goes on behind the panel and the update stream
int lookahead_join(LookAhead* la, hipStream_t user) {
    NNGP_HIP_CHECK(hipEventRecord(la->ev_panel_done, la->panel));
    NNGP_HIP_CHECK(hipEventRecord(la->ev_update_done, la->update));
    NNGP_HIP_CHECK(hipStreamWaitEvent(user, la->ev_panel_done, 0));
    NNGP_HIP_CHECK(hipStreamWaitEvent(user, la->ev_update_done, 0));
    return 0;
}

// Live timing of the split-float16 trailing updates (nngp_model_update_timer): an event pair around each launch on stream s,
// created on first use.  begin: 1 = this launch is timed and `end` has to follow it, 0 = not timed.
int update_timer_begin(LookAhead* la, hipStream_t s) {
    if (!la->time_updates || la->tu_count >= LookAhead::kMaxTimed) return 0;
    const int t = la->tu_count;
    if (la->tu0[t] == nullptr) NNGP_HIP_CHECK(hipEventCreate(&la->tu0[t]));
    if (la->tu1[t] == nullptr) NNGP_HIP_CHECK(hipEventCreate(&la->tu1[t]));
    NNGP_HIP_CHECK(hipEventRecord(la->tu0[t], s));
    return 1;
}

// entries: updated entries of C; rows_cols: rows of the two operands, summed over the launch's regions; kk: depth of the product
int update_timer_end(LookAhead* la, hipStream_t s, double entries, double rows_cols, double kk) {
    const int t = la->tu_count++;
    NNGP_HIP_CHECK(hipEventRecord(la->tu1[t], s));
    la->tu_flops[t] = 2.0 * entries * kk;
    la->tu_bytes[t] = 8.0 * entries + 4.0 * rows_cols * kk;
    return 0;
}

// entries of the region rows [0, m) x cols [0, n) with col <= row + shift
double trap_entries(int64_t m, int64_t n, int64_t shift) {
    double e = 0.0;
    // rows r < n - shift see r + shift + 1 columns, the others n
    const int64_t full_from = (n - shift - 1 > 0) ? n - shift - 1 : 0;  // first row that sees all n columns
    const int64_t rt = full_from < m ? full_from : m;
    e += (double)rt * (double)(shift + 1) + 0.5 * (double)rt * (double)(rt - 1);
    if (m > rt) e += (double)(m - rt) * (double)n;
    return e;
}

double region_entries(const H3RegionSpec* reg, int nreg) {
    double e = 0.0;
    for (int r = 0; r < nreg; ++r) e += trap_entries(reg[r].m, reg[r].n, reg[r].shift);
    return e;
}

double region_rows_cols(const H3RegionSpec* reg, int nreg) {
    double rc = 0.0;
    for (int r = 0; r < nreg; ++r) rc += (double)reg[r].m + (double)reg[r].n;
    return rc;
}

// One timed split-float16 launch on the update stream: the lower trapezoid rows [0, m) x cols [0, n), col <= row + diag_shift,
// of c receives np panels of depth k each (less the `lead` columns of the first)
int h3_update_timed(LookAhead* la, float* c, int64_t ldc, const char* a, const char* b, int64_t ldp, int64_t pstride, int np, int64_t lead,
                    int64_t m, int64_t n, int64_t k, float alpha, int64_t diag_shift, SplitWork* sw, int reserve) {
    if (m <= 0 || n <= 0) return 0;
    const int timed = update_timer_begin(la, la->update);
    if (timed < 0) return timed;
    NNGP_TRY(launch_gemm_nt_h3x(c, ldc, a, b, ldp, pstride, np, lead, m, n, k, alpha, 1.0f, true, diag_shift, sw->counters, reserve,
                                la->update));
    if (timed)
        NNGP_TRY(update_timer_end(la, la->update, trap_entries(m, n, diag_shift), (double)m + (double)n,
                                  (double)np * (double)k - (double)lead));
    return 0;
}

// float32-MFMA update of the lower trapezoid rows [0, m) x cols [0, n), n <= m (lower triangle inside the top n x n square):
// c -= pa pb^T over K columns; pa, pb: rows of the factor (row stride ld), pb = the rows of the trapezoid's columns
int f32_update_trap(float* c, int64_t ld, const float* pa, const float* pb, int64_t m, int64_t n, int64_t kk, hipStream_t s) {
    if (m <= 0 || n <= 0 || kk <= 0) return 0;
    NNGP_TRY(launch_gemm_nt_f32(c, ld, pa, ld, pb, ld, n, n, kk, -1.0f, 1.0f, true, s));
    if (m > n) NNGP_TRY(launch_gemm_nt_f32(c + n * ld, ld, pa + n * ld, ld, pb, ld, m - n, n, kk, -1.0f, 1.0f, false, s));
    return 0;
}

// The same for rows [nb2, m) x cols [0, wn) of the trailing matrix c (on or below its diagonal), m > nb2: kk columns of the
// panel rows p.  The rectangle under the next diagonal block first (the rows start below its columns), then the trapezoid beside it.
int f32_update_below(float* c, int64_t ld, const float* p, int64_t nb2, int64_t m, int64_t wn, int64_t kk, hipStream_t s) {
    NNGP_TRY(launch_gemm_nt_f32(c + nb2 * ld, ld, p + nb2 * ld, ld, p, ld, m - nb2, nb2, kk, -1.0f, 1.0f, false, s));
    return f32_update_trap(c + nb2 * ld + nb2, ld, p + nb2 * ld, p + nb2 * ld, m - nb2, wn - nb2, kk, s);
}

// The float32 pass that follows a split-float16 launch over `reg` which left out the first `lead` columns of a panel: lcols points
// at those columns of the factor's row 0 (a itself for block column 0)
int lead_pass_f32(float* a, int64_t ld, const float* lcols, const H3RegionSpec* reg, int nreg, int64_t lead, hipStream_t s) {
    for (int r = 0; r < nreg && lead > 0; ++r) {
        float* cr = a + reg[r].row0 * ld + reg[r].col0;
        const float* pa = lcols + reg[r].row0 * ld;
        const float* pb = lcols + reg[r].col0 * ld;
        if (reg[r].shift == 0) {
            NNGP_TRY(f32_update_trap(cr, ld, pa, pb, reg[r].m, reg[r].n, lead, s));
        } else {  // rows start `shift` below the columns: every entry of the columns is in
            NNGP_TRY(launch_gemm_nt_f32(cr, ld, pa, ld, pb, ld, reg[r].m, reg[r].n, lead, -1.0f, 1.0f, false, s));
        }
    }
    return 0;
}

// "Solve the rows below a diagonal block": b [m, w] <- b L_kk^-T in one fused launch (trsm_panel.hip) that also leaves the rows'
// split copy in `planes` (NULL: none).  From the second block column on the solve's left-looking products run on the float16 pipe
// (k_trsm_panel_h3): the diagonal block is split into a buffer of its own first, in the order the kernel's waves read it
// (k_split_diag_frag).  Block column 0 stays float32 (same-sign data, see kLeadF32Cols); debug key 2 = 5: float32 everywhere
// (the grouped schedules never run under it).
struct DiagSolve {
    bool h3 = false;  // solve against the split copy (ldiag, dfrag, dscale) instead of the float32 block (akk, dk)
    const float* akk = nullptr;
    const float* dk = nullptr;
    int64_t ld = 0, w = 0;
    char* ldiag = nullptr;
    float* dfrag = nullptr;
    float* dscale = nullptr;
};

// after_first: not block column 0, and the rows' split copy has a place (the callers' own conditions); buf: which of the
// workspace's two buffers takes the block's split copy
int diag_solve_begin(DiagSolve* d, bool after_first, const float* akk, int64_t ld, const float* dk, int64_t w, const SplitWork* sw, int buf,
                     hipStream_t s) {
    d->akk = akk; d->dk = dk; d->ld = ld; d->w = w;
    d->h3 = after_first && w == 1024 && sw->ldiag != nullptr && sw->dfrag != nullptr && NNGP_KNOB(2) != 5;
    if (!d->h3) return 0;
    d->ldiag = sw->ldiag + (int64_t)buf * 4 * sw->k_cap * sw->k_cap;
    d->dfrag = sw->dfrag + (int64_t)buf * sw->k_cap * 128;
    d->dscale = sw->dscale + (int64_t)buf * sw->k_cap;
    return launch_split_diag_frag(akk, ld, w, sw->scale, d->ldiag, dk, d->dfrag, d->dscale, s);
}

int diag_solve_rows(const DiagSolve& d, float* b, int64_t m, char* planes, int64_t ldp, float scale, hipStream_t s, char* planes_t = nullptr,
                    int64_t tstride = 0, int64_t row0 = 0, int64_t col0 = 0) {
    if (d.h3) return launch_trsm_panel_h3(b, d.ld, m, d.ldiag, d.dfrag, d.dscale, d.w, planes, ldp, scale, s, planes_t, tstride, row0, col0);
    return launch_trsm_panel_f32(b, d.ld, m, d.akk, d.ld, d.dk, d.w, planes, ldp, scale, s, planes_t, tstride, row0, col0);
}

// both in one: all rows in one launch
int solve_rows_below(bool after_first, const float* akk, int64_t ld, const float* dk, int64_t w, const SplitWork* sw, float* b, int64_t m,
                     char* planes, int64_t ldp, float scale, hipStream_t s, char* planes_t = nullptr, int64_t tstride = 0, int64_t row0 = 0,
                     int64_t col0 = 0) {
    DiagSolve d;
    NNGP_TRY(diag_solve_begin(&d, after_first, akk, ld, dk, w, sw, 0, s));
    return diag_solve_rows(d, b, m, planes, ldp, scale, s, planes_t, tstride, row0, col0);
}

// ---- grouped form (round 3): deep-K trailing updates -----------------------------------------------------------------------
// A 256 x 256 tile of the trailing update costs its workgroup ~60k cycles of C traffic and tile hand-over beside ~112k cycles
// of matrix work per 1024 columns of K (in-kernel stamps, profiles/r3_h3_stamps.txt) -- a compute unit reads and writes its
// 512 KB of C at ~25 GB/s while its matrix pipe idles, and with one workgroup per unit nothing else runs there meanwhile.
// So K is deepened instead: the block columns are taken in groups of D.  A finished block column k is applied at once only
// to the remaining columns of ITS group (a narrow update, K = 1024); the columns beyond the group receive the whole group in
// ONE pass over C (K = 1024 D: measured 459 TF/s at K = 4096 against 360 at K = 1024).  The far update of a group is issued in
// pieces, in stream order between the next group's panel steps, so that every diagonal-block factorisation on the panel
// stream still runs under a large update:
//   F0        next diagonal block (float32 GEMM, K = 1024 D)                    -> releases the panel stream
//   chunk i   (while diagonal block gend + i is factored)  column gend + i + 1 of the next group (i = 0: also the rows of column
//             gend below its diagonal block) and the i-th share of the columns beyond the next group
// Every C tile is read and written 1 + (columns of its group before it) times per group pass instead of once per block column.
struct FarWork {
    bool active = false;
    int g0 = 0, np = 0;        // first block column of the group, number of panels
    int64_t r0 = 0;            // global row / column where the far region starts (= first row below the group)
    int next = 0;              // next chunk to issue
    int nchunks = 0;
    int64_t share_lo[LookAhead::kMaxSteps + 1] = {};  // far-far shares: global column ranges [share_lo[i], share_lo[i + 1])

    // The group of np panels from block column g0 on is complete and the far region starts at r0: one chunk per block column
    // of the next group (dn of them), and the columns beyond the next group in shares of equal trapezoid area -- whole block
    // columns; few, large launches.
    void begin(int g0_, int np_, int64_t r0_, int dn, int64_t n, int64_t nb) {
        *this = FarWork();
        active = true;
        g0 = g0_;
        np = np_;
        r0 = r0_;
        nchunks = dn;
        const int64_t f0 = r0 + (int64_t)dn * nb;
        for (int i = 0; i <= dn; ++i) share_lo[i] = f0 < n ? f0 : n;
        if (f0 >= n) return;
        const int64_t mf = n - f0;
        const double total = 0.5 * (double)mf * (double)mf;
        const double tiles = total / (256.0 * 256.0);
        int ns = (int)(tiles / 700.0);  // >= ~3 tiles per compute unit and launch
        if (ns < 1) ns = 1;
        if (ns > dn) ns = dn;
        double acc_area = 0.0;
        int sidx = 1;
        for (int64_t col = f0; col < n; col += nb) {
            const int64_t w = (n - col < nb) ? n - col : nb;
            acc_area += (double)(n - col) * (double)w - 0.5 * (double)w * (double)w;
            if (sidx < ns && acc_area >= total * sidx / ns) share_lo[sidx++] = col + w;
        }
        for (int i = sidx; i <= dn; ++i) share_lo[i] = n;
    }

    // the next chunk to issue, or -1 when none is left
    int take() {
        if (!active || next >= nchunks) return -1;
        const int i = next++;
        if (next >= nchunks) active = false;
        return i;
    }

    // Appends the regions of chunk i that `parts` names to reg (room for all three): rows [row0, n) x cols [col0, col0 + w), lower
    // trapezoid (col <= row + shift relative to the region's origin).
    enum : int {
        kColRows = 1,  // chunk 0 only: the rows of the next group's first column below its diagonal block (the block itself was F0)
        kNextCol = 2,  // column gend + i + 1, if it belongs to the next group (D block columns a group)
        kShare = 4,    // the chunk's share of the columns beyond the next group
        kAll = 7
    };
    void chunk_regions(int i, int D, int64_t n, int64_t nb, int parts, H3RegionSpec* reg, int* nreg) const {
        auto width = [&](int64_t col0) { return (n - col0 < nb) ? n - col0 : nb; };
        auto add = [&](int64_t row0, int64_t col0, int64_t w, int64_t shift) {
            if (n - row0 > 0 && w > 0) reg[(*nreg)++] = H3RegionSpec{row0, col0, n - row0, w, shift};
        };
        if ((parts & kColRows) && i == 0) {
            const int64_t w0 = width(r0);
            add(r0 + w0, r0, w0, w0);
        }
        const int64_t c1 = r0 + (int64_t)(i + 1) * nb;
        if ((parts & kNextCol) && c1 < n && i + 1 < D) add(c1, c1, width(c1), 0);
        // shares are dealt from the LAST chunk backwards: the early chunks already carry the next group's own columns
        const int si = nchunks - 1 - i;
        if ((parts & kShare) && share_lo[si + 1] > share_lo[si]) add(share_lo[si], share_lo[si], share_lo[si + 1] - share_lo[si], 0);
    }
};

// What both grouped schedules derive from their arguments
struct Grouped {
    float* a;
    int64_t n, ld, nb;
    LookAhead* la;
    SplitWork* sw;
    int64_t ldp;    // bytes per row of the split planes
    float ascale;   // -1 / scale^2: undoes the scale of both split operands
    int reserve;    // compute units a persistent split-float16 grid leaves to the panel stream (debug key 4 overrides)
    Grouped(float* a_, int64_t n_, int64_t ld_, int64_t nb_, LookAhead* la_, SplitWork* sw_)
        : a(a_), n(n_), ld(ld_), nb(nb_), la(la_), sw(sw_), ldp(4 * sw_->k_cap), ascale(-1.0f / (sw_->scale * sw_->scale)),
          reserve(NNGP_KNOB(4) > 0 ? NNGP_KNOB(4) : 32) {}
    char* plane_rows(int col, int64_t row) const { return sw->planes + (int64_t)col * sw->col_stride + row * ldp; }
    int64_t width(int64_t col0) const { return (n - col0 < nb) ? n - col0 : nb; }
    int nblk() const { return (int)((n + nb - 1) / nb); }
    // one split-float16 grid of the pending far update over `reg`, all panels of the group in one pass over C
    // (helper: 0 = the only grid, 1 = a helper grid follows, 2 = the helper grid)
    int far_grid(const FarWork& far, const H3RegionSpec* reg, int nreg, int64_t lead, hipStream_t s, int helper) const {
        const char* rows = plane_rows(far.g0 + far.np - 1, 0);  // latest panel
        return launch_gemm_nt_h3r(a, ld, rows, rows, ldp, sw->col_stride, far.np, lead, reg, nreg, nb, ascale, 1.0f, true, sw->counters, reserve,
                                  s, nullptr, helper);
    }
    // inside a group: block column k (solved rows `below`, their split copy at pk_rows) goes to the rest of its group -- rows [nb2, m)
    // x the first wn columns of the trailing matrix c, on or below its diagonal (the next diagonal block above them is the caller's)
    int near_update(float* c, const float* below, const char* pk_rows, int64_t nb2, int64_t m, int64_t wn, int64_t nbk, int64_t lead) const {
        NNGP_TRY(h3_update_timed(la, c + nb2 * ld, ld, pk_rows + nb2 * ldp + lead * 4, pk_rows + lead * 4, ldp, 0, 1, 0, m - nb2, wn, nbk - lead,
                                 ascale, nb2, sw, reserve));
        if (lead > 0) NNGP_TRY(f32_update_below(c, ld, below, nb2, m, wn, lead, la->update));
        return 0;
    }
};

int potrf_lookahead_grouped(float* a, int64_t n, int64_t ld, float* dinv, int32_t* clamped, float pivot_floor, LookAhead* la,
                            SplitWork* sw, hipStream_t user, int64_t nb, int D) {
    la->tu_count = 0;
    NNGP_TRY(lookahead_fork(la, user));
    const Grouped g(a, n, ld, nb, la, sw);
    const int nblk = g.nblk();
    const bool use_helper = !(NNGP_KNOB(2) >= 31 && NNGP_KNOB(2) <= 46) && g.reserve >= 8 && g.reserve % 8 == 0;  // debug key 2 = 30 + D: no helper grids
    FarWork far;
    bool wrote_t = true;  // every panel solve also left the transposed split copy

    // One launch per chunk: up to three regions of the pending group's far update with all panels of the group in one pass over C;
    // the group's lead columns go through the float32 GEMM region by region.
    auto far_chunk = [&](int step) -> int {
        const int i = far.take();
        if (i < 0) return 0;
        H3RegionSpec reg[4];
        int nreg = 0;
        far.chunk_regions(i, D, n, nb, FarWork::kAll, reg, &nreg);
        if (nreg == 0) return 0;
        const int64_t lead = far.g0 == 0 ? kLeadF32Cols : 0;
        const double entries = region_entries(reg, nreg);
        const int timed = update_timer_begin(la, la->update);
        if (timed < 0) return timed;
        // The `reserve` compute units this launch leaves to the panel stream idle once the diagonal-block chain (0.5 ms) is done:
        // a helper grid of that many workgroups, enqueued on the PANEL stream behind the chain, then joins the pass through the
        // shared work counters.  It may not start before everything the pass depends on (the update stream up to here), and the
        // update stream may not go on before it has finished.  Only for passes long enough to outlive the chain.
        const bool helper = use_helper && step >= 0 && entries / 65536.0 * (double)far.np >= 4.0 * 3.0 * 224.0;  // >= ~3 rounds of K = 4096 tiles
        if (helper) NNGP_HIP_CHECK(hipEventRecord(la->ev_chunk[step], la->update));
        NNGP_TRY(g.far_grid(far, reg, nreg, lead, la->update, helper ? 1 : 0));
        if (helper) {
            NNGP_HIP_CHECK(hipStreamWaitEvent(la->panel, la->ev_chunk[step], 0));
            NNGP_TRY(g.far_grid(far, reg, nreg, lead, la->panel, 2));
            NNGP_HIP_CHECK(hipEventRecord(la->ev_helper[step], la->panel));
            NNGP_HIP_CHECK(hipStreamWaitEvent(la->update, la->ev_helper[step], 0));
        }
        if (timed) NNGP_TRY(update_timer_end(la, la->update, entries, region_rows_cols(reg, nreg), (double)far.np * (double)nb - (double)lead));
        return lead_pass_f32(a, ld, a, reg, nreg, lead, la->update);  // columns [0, lead) of block column 0
    };

    int rc = 0;
    for (int k = 0; k < nblk && rc == 0; ++k) {
        const int64_t o = (int64_t)k * nb;
        const int64_t nbk = g.width(o);
        const int64_t m = n - o - nbk;  // rows below this block column
        float* akk = a + o * ld + o;
        float* dk = dinv + (o / TB) * TB * TB;
        const int g0 = (k / D) * D;
        const int gend = (g0 + D < nblk) ? g0 + D : nblk;
        // panel stream: factor the diagonal block (chain of small kernels)
        if (k > 0) NNGP_HIP_CHECK(hipStreamWaitEvent(la->panel, la->ev_col[k - 1], 0));
        rc = potrf_rec(akk, nbk, ld, dk, clamped, pivot_floor, la->panel);
        NNGP_HIP_CHECK(hipEventRecord(la->ev_panel[k], la->panel));
        if (rc != 0) break;
        // update stream, while that factorisation runs: the next piece of the previous group's far update
        rc = far_chunk(k);
        if (rc != 0 || m == 0) break;
        NNGP_HIP_CHECK(hipStreamWaitEvent(la->update, la->ev_panel[k], 0));
        // solve all rows below in one fused launch; it leaves their float16 split copy in this block column's planes
        const int64_t nb2 = g.width(o + nbk);
        float* below = akk + nbk * ld;           // panel rows below the diagonal block: [m, nbk]
        float* c = below + nbk;                  // trailing matrix: [m, m]
        char* pk_rows = g.plane_rows(k, o + nbk);
        // (the same launch also leaves the rows' TRANSPOSED split copy -- the operand of the posterior's "B L^-1" solves -- so
        // that no pass over the finished factor has to write it beside the first solve of a predict; debug key 9 = 8: not here)
        char* pt = (sw->planes_t != nullptr && nb == sw->k_cap && NNGP_KNOB(9) != 8) ? sw->planes_t : nullptr;
        wrote_t = wrote_t && pt != nullptr;
        rc = solve_rows_below(k > 0, akk, ld, dk, nbk, sw, below, m, pk_rows, g.ldp, sw->scale, la->update, pt, sw->col_stride, o + nbk, o);
        if (rc != 0) break;
        if (k + 1 < gend) {
            // ---- inside the group: block column k goes to the group's remaining columns only (K = nbk) ----
            rc = launch_gemm_nt_f32(c, ld, below, ld, below, ld, nb2, nb2, nbk, -1.0f, 1.0f, true, la->update);  // next diagonal block
            NNGP_HIP_CHECK(hipEventRecord(la->ev_col[k], la->update));
            int64_t wn = (int64_t)(gend - 1 - k) * nb;  // columns of the group after block column k
            if (wn > m) wn = m;
            if (rc == 0 && m > nb2) rc = g.near_update(c, below, pk_rows, nb2, m, wn, nbk, k == 0 ? kLeadF32Cols : 0);
        } else {
            // ---- the group is complete: its far update starts with the next diagonal block (all panels, float32 GEMM) ----
            const int np = k + 1 - g0;
            const float* rows = a + (o + nbk) * ld + (int64_t)g0 * nb;  // rows below the group, columns of the group
            rc = launch_gemm_nt_f32(c, ld, rows, ld, rows, ld, nb2, nb2, (int64_t)np * nb, -1.0f, 1.0f, true, la->update);
            NNGP_HIP_CHECK(hipEventRecord(la->ev_col[k], la->update));
            far.begin(g0, np, o + nbk, (nblk - (k + 1) < D) ? nblk - (k + 1) : D, n, nb);
        }
    }
    while (rc == 0 && far.active) rc = far_chunk(-1);  // (nothing is left when the loop ran to the last block column)
    if (rc == 0) sw->l_ready = true;
    if (rc == 0 && wrote_t && sw->planes_t != nullptr) sw->lt_ready = true;
    NNGP_TRY(lookahead_join(la, user));
    return rc;
}

// ---- grouped form, round 4: the panel solves leave the update stream ---------------------------------------------------------------
// Round 3's timeline (profiles/r3_timeline_cfg3.csv) has 7.8 ms of panel solves, float32 diagonal-block updates and splits IN LINE
// with the 28.4 ms of split-float16 trailing updates on the update stream, most of the chip idle meanwhile.  Here the update stream
// carries the trailing updates only.  Per block column k:
//   panel stream   P_k  factor the diagonal block               (needs the update stream up to the far chunk issued at step k - 1)
//                  Tc_k solve the nb rows right below it        (needs the near update of block column k - 1)
//                  G_k  their product onto diagonal block k + 1 (float32 MFMA, K = nb)           -> P_{k+1}
//   bulk stream    Tb_k solve all other rows below              (same inputs as Tc_k; a priority above the update stream's: its
//                       workgroups run on the compute units the trailing updates leave free and take over whatever a finishing
//                       update launch gives back, before the next launch's persistent grid settles there)
//   update stream  the far chunk of step k (previous group's panels, K = nb D), then N_k = block column k onto the rest of its
//                       group (K = nb; needs Tc_k and Tb_k)
// In the product's schedule the next group's first diagonal block receives the whole finished group in one float32 GEMM (K = nb D)
// at the head of the chain; with debug key 8 = 4 the D - 1 earlier panels go there as soon as THEY are solved (a stream of its own,
// behind Tb of the group's last-but-one column) and only the last panel's K = nb product is left in the chain.  The split copy of a diagonal block and its inverted
// 128-blocks (operands of the fused solves) alternate between two buffers: Tb_k may still be reading one while the panel stream
// prepares block column k + 1.
int potrf_lookahead_grouped_v4(float* a, int64_t n, int64_t ld, float* dinv, int32_t* clamped, float pivot_floor, LookAhead* la,
                               SplitWork* sw, hipStream_t user, int64_t nb, int D, TriInv* ti) {
    la->tu_count = 0;
    hipStream_t SP = la->panel, SU = la->update, SB = (NNGP_KNOB(8) & 2) ? la->panel : la->bulk;
#ifdef NNGP_TIMING_KNOBS
    static hipEvent_t dbg_ev[8] = {};
    const bool dbg = NNGP_KNOB(12) != 0;
    if (dbg && dbg_ev[0] == nullptr)
        for (auto& e : dbg_ev) (void)hipEventCreate(&e);
    if (dbg) (void)hipEventRecord(dbg_ev[0], user);
#endif
    NNGP_TRY(lookahead_fork(la, user, SB));
    const Grouped g(a, n, ld, nb, la, sw);
    const int nblk = g.nblk();
    // Helper grids (the reserved compute units join a far chunk once the diagonal-block chain is done, see potrf_lookahead_grouped)
    // are OFF here: the chain runs ahead of the update stream and the bulk solves live on those units -- a persistent helper grid
    // starves both (measured: chains of 1.3 - 2.8 ms instead of 0.6, Cholesky 54.8 ms).  Debug key 8 = 8: on, behind Tb_k on the
    // bulk stream.
    const bool use_helper = (NNGP_KNOB(8) & 8) && g.reserve >= 8 && g.reserve % 8 == 0;
    const bool early_gp = (NNGP_KNOB(8) & 4) != 0;  // measured: one more CG iteration (6 instead of 5 at N = 32768) -- off
    FarWork far;
    // a far chunk's helper grid is enqueued BEHIND the step's chain work and bulk solve
    struct PendingHelper {
        bool on = false;
        H3RegionSpec reg[4];
        int nreg = 0, step = 0;
        int64_t lead = 0;
    } ph;

    // one split-float16 launch of the pending group's far update over `reg` (+ the float32 pass of the group's lead columns)
    auto far_launch = [&](const H3RegionSpec* reg, int nreg, int step, bool allow_helper) -> int {
        if (nreg == 0) return 0;
        const int64_t lead = far.g0 == 0 ? kLeadF32Cols : 0;
        const double entries = region_entries(reg, nreg);
        // (a pass with lead columns is followed by float32 launches over the same regions: no helper there)
        const bool helper = allow_helper && use_helper && lead == 0 && step >= 0 && entries / 65536.0 * (double)far.np >= 4.0 * 3.0 * 224.0;
        const int timed = update_timer_begin(la, SU);
        if (timed < 0) return timed;
        if (helper) NNGP_HIP_CHECK(hipEventRecord(la->ev_chunk[step], SU));
        NNGP_TRY(g.far_grid(far, reg, nreg, lead, SU, helper ? 1 : 0));
        if (timed) NNGP_TRY(update_timer_end(la, SU, entries, region_rows_cols(reg, nreg), (double)far.np * (double)nb - (double)lead));
        if (helper) {
            ph.on = true;
            ph.nreg = nreg;
            for (int r = 0; r < nreg; ++r) ph.reg[r] = reg[r];
            ph.step = step; ph.lead = lead;
        }
        return lead_pass_f32(a, ld, a, reg, nreg, lead, SU);  // columns [0, lead) of block column 0
    };
    // the pieces of the pending far update that belong to step `step` (block column gend + i of the next group is being factored)
    auto far_step = [&](int step, bool* colrows_event, bool* c1_event) -> int {
        const int i = far.take();
        if (i < 0) return 0;
        H3RegionSpec reg[4];
        int nreg = 0;
        // the rows of the next group's first column below its diagonal block: its panel solve waits for exactly these
        far.chunk_regions(i, D, n, nb, FarWork::kColRows, reg, &nreg);
        if (nreg > 0 && step >= 0) {
            NNGP_TRY(far_launch(reg, nreg, step, false));
            NNGP_HIP_CHECK(hipEventRecord(la->ev_col[step], SU));
            *colrows_event = true;
            nreg = 0;
        }
        // column gend + i + 1 of the next group in a launch of its own: the chain (G, P of that column) waits for this launch only,
        // not for the chunk's share of the columns beyond -- the diagonal-block chain then runs a whole step ahead of the update
        // stream and the bulk solve of a block column has the following far chunk to hide under (debug key 8 = 16 only)
        const bool split_c1 = (NNGP_KNOB(8) & 16) && step >= 0;  // measured: +0.6 ms (one more launch per step) -- off
        far.chunk_regions(i, D, n, nb, FarWork::kNextCol, reg, &nreg);
        if (split_c1 && nreg > 0) {
            NNGP_TRY(far_launch(reg, nreg, step, false));
            nreg = 0;
        }
        if (split_c1) {
            NNGP_HIP_CHECK(hipEventRecord(la->ev_c1[step], SU));
            *c1_event = true;
        }
        far.chunk_regions(i, D, n, nb, FarWork::kShare, reg, &nreg);
        return far_launch(reg, nreg, step, true);
    };

    int rc = 0;
    bool side_used = false;
    const int kTriInvTail = NNGP_KNOB(10) > 0 ? NNGP_KNOB(10) : 7;  // block columns from the end where the finished blocks' inverses are issued
    for (int k = 0; k < nblk && rc == 0; ++k) {
        const int64_t o = (int64_t)k * nb;
        const int64_t nbk = g.width(o);
        const int64_t m = n - o - nbk;  // rows below this block column
        float* akk = a + o * ld + o;
        float* dk = dinv + (o / TB) * TB * TB;
        const int g0 = (k / D) * D;
        const int gend = (g0 + D < nblk) ? g0 + D : nblk;
        // ---- panel stream: P_k ----
        if (k > 0) NNGP_HIP_CHECK(hipStreamWaitEvent(SP, la->ev_chain[k - 1], 0));
        rc = potrf_rec(akk, nbk, ld, dk, clamped, pivot_floor, SP);
        NNGP_HIP_CHECK(hipEventRecord(la->ev_panel[k], SP));
        if (rc != 0) break;
        // The inverted diagonal blocks of the blocked solves (solve.hip, triinv_build): from here on the chain of diagonal-block
        // factorisations bounds the factorisation and most of the chip idles -- the blocks of the block columns behind us are
        // inverted now, on the lowest-priority stream, instead of after the factorisation.  Debug key 8 = 32 only: measured, the side work
        // delays the chain by what it saves after the factorisation (42.1 against 42.3 ms at N = 32768).
        if (ti != nullptr && la->side != nullptr && (NNGP_KNOB(8) & 32) && k == nblk - kTriInvTail && ti->bs % nb == 0 && k >= 2) {
            const int64_t jdone = ((int64_t)(k - 1) * nb) / ti->bs;  // block columns 0 .. k - 2 are final (P_{k-1} has been waited for by Tc_{k-1})
            if (jdone > 0) {
                hipStream_t SS = NNGP_KNOB(11) == 3 ? la->aux : NNGP_KNOB(11) == 4 ? la->bulk : la->side;
                NNGP_HIP_CHECK(hipStreamWaitEvent(SS, la->ev_tc[k - 1], 0));
#ifdef NNGP_TIMING_KNOBS
                if (dbg) (void)hipEventRecord(dbg_ev[1], SS);
#endif
                rc = triinv_build_range(a, ld, dinv, n, *ti, 0, jdone, SS);
                if (rc != 0) break;
#ifdef NNGP_TIMING_KNOBS
                if (dbg) (void)hipEventRecord(dbg_ev[2], SS);
#endif
                NNGP_HIP_CHECK(hipEventRecord(la->ev_side_done, SS));
                ti->done_blocks = jdone;
                side_used = true;
            }
        }
        // ---- update stream: this step's share of the previous group's far update ----
        bool colrows = false, c1ev = false;
        ph.on = false;
        rc = far_step(k, &colrows, &c1ev);
        NNGP_HIP_CHECK(hipEventRecord(la->ev_far[k], SU));
        // what the chain's next links (G_k, P_{k+1}) wait for: everything on the update stream that touches diagonal block k + 1 --
        // the near updates up to N_{k-1} and this step's launch over column k + 1 (or, at a group's end, the whole chunk: the
        // previous group's shares cover the next group's first diagonal block)
        la->ev_chain[k] = (c1ev && k + 1 < gend) ? la->ev_c1[k] : la->ev_far[k];
        if (rc != 0 || m == 0) break;
        // ---- the panel solves: Tc_k on the panel stream, Tb_k on the bulk stream ----
        const int64_t nb2 = g.width(o + nbk);
        float* below = akk + nbk * ld;           // panel rows below the diagonal block: [m, nbk]
        float* c = below + nbk;                  // trailing matrix: [m, m]
        char* pk_rows = g.plane_rows(k, o + nbk);
        hipEvent_t ev_rows = nullptr;            // block column k below its diagonal block has received everything
        if (k > g0) ev_rows = la->ev_near[k - 1];
        else if (colrows) ev_rows = la->ev_col[k];
        if (ev_rows != nullptr) NNGP_HIP_CHECK(hipStreamWaitEvent(SP, ev_rows, 0));
        DiagSolve ds;  // (split-copy buffers by block-column parity: Tb_k may still be reading one while the panel stream prepares k + 1)
        rc = diag_solve_begin(&ds, k > 0, akk, ld, dk, nbk, sw, k & 1, SP);
        if (rc == 0) rc = diag_solve_rows(ds, below, nb2, pk_rows, g.ldp, sw->scale, SP);
        if (rc != 0) break;
        NNGP_HIP_CHECK(hipEventRecord(la->ev_tc[k], SP));  // (also: the diagonal block is factored and split)
        if (m > nb2) {
            NNGP_HIP_CHECK(hipStreamWaitEvent(SB, la->ev_tc[k], 0));
            if (ev_rows != nullptr) NNGP_HIP_CHECK(hipStreamWaitEvent(SB, ev_rows, 0));
            rc = diag_solve_rows(ds, below + nb2 * ld, m - nb2, pk_rows + nb2 * g.ldp, g.ldp, sw->scale, SB);
            if (rc != 0) break;
        }
        NNGP_HIP_CHECK(hipEventRecord(la->ev_tb[k], SB));
        // The far chunk's helper grid: the `reserve` compute units the chunk's own grid leaves free carry the diagonal-block chain (a
        // workgroup at a time) and the bulk solve; that many workgroups join the chunk from a stream of their own (debug key 8 = 8:
        // from the bulk stream, behind Tb_k).  Not from the panel stream as in round 3: the chain no longer waits for the chunk.
        if (ph.on) {
            hipStream_t SH = SB;
            NNGP_HIP_CHECK(hipStreamWaitEvent(SH, la->ev_chunk[ph.step], 0));
            rc = g.far_grid(far, ph.reg, ph.nreg, ph.lead, SH, 2);  // (far is still the group the chunk belongs to)
            if (rc != 0) break;
            NNGP_HIP_CHECK(hipEventRecord(la->ev_helper[ph.step], SH));
            NNGP_HIP_CHECK(hipStreamWaitEvent(SU, la->ev_helper[ph.step], 0));
            ph.on = false;
        }
        // ---- G_k, the product of the rows just solved onto the next diagonal block.  This step's far chunk carries that block's
        // share of the previous group (same C tiles): the product waits for it, as P_{k+1} has to anyway. ----
        NNGP_HIP_CHECK(hipStreamWaitEvent(SP, la->ev_chain[k], 0));
        if (k + 1 < gend) {
            rc = launch_gemm_nt_f32(c, ld, below, ld, below, ld, nb2, nb2, nbk, -1.0f, 1.0f, true, SP);
        } else {
            // The next group's first diagonal block receives the whole finished group.  Its D - 1 earlier panels are solved once the
            // bulk stream has passed Tb_{k-1}, and the previous group's last far chunk (this step's: it covers that block too) has to
            // be through: behind both, on a stream of its own, the K = nb (D - 1) product runs beside P_k when the chain is what
            // bounds the factorisation (the late block columns); only the last panel's K = nb product is left in the chain.
            const int np = k + 1 - g0;
            const float* rows = a + (o + nbk) * ld + (int64_t)g0 * nb;  // rows of the next diagonal block, columns of the group
            if (early_gp && np >= 2 && la->aux != nullptr) {
                NNGP_HIP_CHECK(hipStreamWaitEvent(la->aux, la->ev_far[k], 0));
                NNGP_HIP_CHECK(hipStreamWaitEvent(la->aux, la->ev_tb[k - 1], 0));
                rc = launch_gemm_nt_f32(c, ld, rows, ld, rows, ld, nb2, nb2, (int64_t)(np - 1) * nb, -1.0f, 1.0f, true, la->aux);
                if (rc != 0) break;
                NNGP_HIP_CHECK(hipEventRecord(la->ev_gp[k], la->aux));
                NNGP_HIP_CHECK(hipStreamWaitEvent(SP, la->ev_gp[k], 0));
                rc = launch_gemm_nt_f32(c, ld, below, ld, below, ld, nb2, nb2, nbk, -1.0f, 1.0f, true, SP);
            } else {  // all panels of the group at once (the earlier panels' rows were solved on the bulk stream)
                if (np >= 2) NNGP_HIP_CHECK(hipStreamWaitEvent(SP, la->ev_tb[k - 1], 0));
                rc = launch_gemm_nt_f32(c, ld, rows, ld, rows, ld, nb2, nb2, (int64_t)np * nb, -1.0f, 1.0f, true, SP);
            }
        }
        if (rc != 0) break;
        // ---- update stream: block column k is solved ----
        NNGP_HIP_CHECK(hipStreamWaitEvent(SU, la->ev_tc[k], 0));
        NNGP_HIP_CHECK(hipStreamWaitEvent(SU, la->ev_tb[k], 0));
        if (k + 1 < gend) {
            // inside the group: block column k goes to the group's remaining columns only (K = nbk)
            int64_t wn = (int64_t)(gend - 1 - k) * nb;  // columns of the group after block column k
            if (wn > m) wn = m;
            if (m > nb2) rc = g.near_update(c, below, pk_rows, nb2, m, wn, nbk, k == 0 ? kLeadF32Cols : 0);
            NNGP_HIP_CHECK(hipEventRecord(la->ev_near[k], SU));
        } else {
            // the group is complete: set up its far update (issued in pieces at the next steps)
            far.begin(g0, k + 1 - g0, o + nbk, (nblk - (k + 1) < D) ? nblk - (k + 1) : D, n, nb);
        }
    }
    bool dummy = false, dummy2 = false;
    while (rc == 0 && far.active) rc = far_step(-1, &dummy, &dummy2);  // (nothing is left when the loop ran to the last block column)
    if (rc == 0) sw->l_ready = true;
#ifdef NNGP_TIMING_KNOBS
    if (dbg) { (void)hipEventRecord(dbg_ev[3], SP); (void)hipEventRecord(dbg_ev[4], SU); (void)hipEventRecord(dbg_ev[5], SB); }
#endif
    NNGP_TRY(lookahead_join(la, user));
    NNGP_HIP_CHECK(hipEventRecord(la->ev_bulk_done, SB));
    NNGP_HIP_CHECK(hipStreamWaitEvent(user, la->ev_bulk_done, 0));
    if (side_used) NNGP_HIP_CHECK(hipStreamWaitEvent(user, la->ev_side_done, 0));
#ifdef NNGP_TIMING_KNOBS
    if (dbg) {
        (void)hipEventRecord(dbg_ev[6], user);
        (void)hipEventSynchronize(dbg_ev[6]);
        float t[7] = {};
        for (int i = 1; i <= 6; ++i)
            if (i > 2 || side_used) (void)hipEventElapsedTime(&t[i], dbg_ev[0], dbg_ev[i]);
        fprintf(stderr, "v4 timing (ms from entry): side %.2f -> %.2f | panel end %.2f  update end %.2f  bulk end %.2f | user resumes %.2f\n", t[1], t[2], t[3],
                t[4], t[5], t[6]);
    }
#endif
    return rc;  // (the aux stream's last product was waited for by the panel stream)
}

}  // namespace

int potrf_lookahead_f32(float* a, int64_t n, int64_t ld, float* dinv, int32_t* clamped, float pivot_floor,
                        LookAhead* la, SplitWork* sw, hipStream_t user, TriInv* ti) {
    if (ti != nullptr) ti->done_blocks = 0;
    NNGP_REQUIRE(n > 0 && n % TB == 0, "potrf_f32: n must be a positive multiple of %d (got %lld)", TB, (long long)n);
    // block-column width: 1024 measured best at N = 32768 (119.4 ms; 2048: 121.3, 4096: 123.2, recursion only: 125)
    int64_t nb = NNGP_KNOB(1) > 0 ? (int64_t)NNGP_KNOB(1) : kLookAheadNb;
    nb = (nb / TB) * TB;
    // large trailing updates on the float16 matrix pipe (gemm_h3.hip) unless the workspace is missing / too small or
    // debug key 2 == 2 asks for the float32-MFMA updates (A/B timing)
    const bool h3 = h3_workspace_ok(sw, n, nb) && sw->counters != nullptr && sw->col_stride >= sw->rows_cap * 4 * sw->k_cap;
    if (sw != nullptr) sw->l_ready = sw->lt_ready = false;
    // (measured and dropped: solving the panel rows in four row chunks on a third stream, each chunk's trailing update
    // starting as soon as it is solved -- 64.8 vs 59.2 ms: four smaller split-float16 launches lose more in their tails
    // than the overlap gains)
    // (measured twice and dropped: inverting each diagonal block on the panel stream as it is factored -- neutral, 59.1 vs
    // 58.9 ms, and 58.1 vs 57.9 ms with CUs reserved for the panel stream -- and solving the panel rows with that inverse as one GEMM: Cholesky -3.7 ms but CG iterations 6 -> 8)
    if (la == nullptr || NNGP_KNOB(2) == 1 || n < 4 * nb || (n + nb - 1) / nb > LookAhead::kMaxSteps)
        return potrf_f32(a, n, ld, dinv, clamped, pivot_floor, user);
    // grouped form: deep-K far updates (debug key 2 = 10 + D overrides the group size; D = 1: the round-2 form below)
    const int group = (NNGP_KNOB(2) >= 11 && NNGP_KNOB(2) <= 26) ? NNGP_KNOB(2) - 10 : (NNGP_KNOB(2) >= 31 && NNGP_KNOB(2) <= 46) ? NNGP_KNOB(2) - 30 : kLookAheadGroup;
    if (h3 && group > 1 && nb == 1024 && (NNGP_KNOB(2) == 0 || NNGP_KNOB(2) >= 11) && NNGP_KNOB(3) == 0 && ld % 4 == 0) {
        // (round 4's schedule with the panel solves off the update stream -- measured equal at N = 32768, slower at the other sizes,
        // see the note above it -- runs on request only: debug key 8 bit 1, set before the model is created)
        if (la->bulk != nullptr && (NNGP_KNOB(8) & 1))
            return potrf_lookahead_grouped_v4(a, n, ld, dinv, clamped, pivot_floor, la, sw, user, nb, group, ti);
        return potrf_lookahead_grouped(a, n, ld, dinv, clamped, pivot_floor, la, sw, user, nb, group);
    }
    // ---- the one-column form: every block column goes to the whole trailing matrix at once (K = nb) ----
    la->tu_count = 0;
    NNGP_TRY(lookahead_fork(la, user));
    int rc = 0;
    int k = 0;
    bool panel_split_done = false;  // the panel solve already left the split copy of this block column's rows in place
    for (int64_t o = 0; o < n && rc == 0; o += nb, ++k) {
        const int64_t nbk = (n - o < nb) ? n - o : nb;
        const int64_t m = n - o - nbk;  // rows below this block column
        float* akk = a + o * ld + o;
        float* dk = dinv + (o / TB) * TB * TB;
        // panel stream: factor the diagonal block (chain of small kernels)
        if (k > 0) NNGP_HIP_CHECK(hipStreamWaitEvent(la->panel, la->ev_col[k - 1], 0));
        rc = potrf_rec(akk, nbk, ld, dk, clamped, pivot_floor, la->panel);
        NNGP_HIP_CHECK(hipEventRecord(la->ev_panel[k], la->panel));
        if (rc != 0 || m == 0) break;
        // update stream: triangular solve of the rows below, then the trailing update
        NNGP_HIP_CHECK(hipStreamWaitEvent(la->update, la->ev_panel[k], 0));
        const int64_t nb2 = (m < nb) ? m : nb;
        const float* p = akk + nbk * ld;        // panel rows below the diagonal block: [m, nbk]
        float* c = akk + nbk * ld + nbk;        // trailing matrix: [m, m]
        // critical path first: solve only the nb2 panel rows the next diagonal block needs, update that block, and
        // release the panel stream; the remaining panel rows and the rest of the trailing update follow.  Both solves are
        // single fused launches (trsm_panel.hip) that also leave the rows' float16 split copy in this block column's planes
        // (rows at their global index: the trailing update and, later, the posterior's blocked solves read them there).
        const bool fused = NNGP_KNOB(2) != 4 && nbk <= 1024;
        const bool planes_here = h3 && nbk == nb && fused;
        const int64_t ldp = h3 ? 4 * sw->k_cap : 0;
        char* pk_rows = h3 ? sw->planes + (int64_t)k * sw->col_stride + (o + nbk) * ldp : nullptr;  // split copy of row o + nbk
        // (One launch for ALL m rows: a separate launch for the nb2 rows the next diagonal block needs kept 32 workgroups -- an
        // eighth of the GPU -- busy for a whole 0.14 ms workgroup round per block column, 4.4 ms per factorisation at N = 32768;
        // the first workgroups of the merged launch are those rows anyway.)
        if (fused)
            rc = solve_rows_below(planes_here && k > 0, akk, ld, dk, nbk, sw, akk + nbk * ld, m, planes_here ? pk_rows : nullptr, ldp,
                                  h3 ? sw->scale : 1.0f, la->update);
        else
            rc = trsm_rlt_f32(akk + nbk * ld, ld, nb2, akk, ld, dk, nbk, la->update);
        if (rc == 0) rc = launch_gemm_nt_f32(c, ld, p, ld, p, ld, nb2, nb2, nbk, -1.0f, 1.0f, true, la->update);
        NNGP_HIP_CHECK(hipEventRecord(la->ev_col[k], la->update));
        // ... then the other panel rows and the rest of the trailing matrix, overlapped with the next diagonal block
        if (rc == 0 && m > nb2) {
            panel_split_done = false;
            if (fused) {
                panel_split_done = planes_here;  // every row was solved (and split) by the launch above
            } else {
                // Round-1 form (debug key 2 = 4).  The solve of the remaining panel rows, X = B L_kk^-T, splits as
                // X1 = B1 L11^-T, B2 -= X1 L21^T, X2 = B2 L22^-T over the two 512-column halves; the product in the middle runs
                // on the float16 pipe from the second block column on (X1 split straight into the planes, L21 into the planes'
                // unused rows of the diagonal block).
                const bool h3_panel = h3 && k > 0 && nbk == nb && nb == 1024 && m - nb2 >= 2048 && NNGP_KNOB(2) != 3 &&
                                      !(NNGP_KNOB(3) >= 10 && NNGP_KNOB(3) < 20 && k < NNGP_KNOB(3) - 10);
                if (h3_panel) {
                    const int64_t h = nbk / 2, mr = m - nb2;
                    char* pk = sw->planes + (int64_t)k * sw->col_stride;        // planes of block column k, global row 0
                    char* xrows = pk + (o + nbk + nb2) * ldp;                    // rows of the panel being solved
                    float* b = akk + (nbk + nb2) * ld;
                    rc = trsm_rlt_f32(b, ld, mr, akk, ld, dk, h, la->update);                                  // X1
                    if (rc == 0) rc = launch_split_rows(b, ld, mr, h, sw->scale, xrows, ldp, la->update);
                    if (rc == 0) rc = launch_split_rows(akk + h * ld, ld, h, h, sw->scale, pk + (o + h) * ldp, ldp, la->update);  // L21
                    if (rc == 0)
                        rc = launch_gemm_nt_h3(b + h, ld, xrows, pk + (o + h) * ldp, ldp, mr, h, h, -1.0f / (sw->scale * sw->scale), 1.0f,
                                               false, 0, sw->counters, NNGP_KNOB(4) > 0 ? NNGP_KNOB(4) : 32, la->update);
                    if (rc == 0) rc = trsm_rlt_f32(b + h, ld, mr, akk + h * ld + h, ld, dk + (h / TB) * TB * TB, h, la->update);  // X2
                    if (rc == 0) rc = launch_split_rows(b + h, ld, mr, h, sw->scale, xrows + h * 4, ldp, la->update);
                    if (rc == 0)  // the rows solved first (critical path) go into the planes as well
                        rc = launch_split_rows(p, ld, nb2, nbk, sw->scale, pk + (o + nbk) * ldp, ldp, la->update);
                    panel_split_done = true;
                } else {
                    rc = trsm_rlt_f32(akk + (nbk + nb2) * ld, ld, m - nb2, akk, ld, dk, nbk, la->update);
                }
            }
            // the first columns of block column 0 stay on the float32 MFMA (kLeadF32Cols; debug key 3 = 10 + n: n whole block
            // columns on float32; 20 + c: lead = 128 c; 31 / 32: lead = 32 / 64)
            const bool f32_first = !h3 || (NNGP_KNOB(3) >= 10 && NNGP_KNOB(3) < 20 && k < NNGP_KNOB(3) - 10);
            int64_t lead = 0;
            if (h3 && !f32_first && k == 0) lead = (NNGP_KNOB(3) >= 20 && NNGP_KNOB(3) < 28) ? 128 * (int64_t)(NNGP_KNOB(3) - 20) :
                                                  (NNGP_KNOB(3) == 31 || NNGP_KNOB(3) == 32) ? 32 * (int64_t)(NNGP_KNOB(3) - 30) : kLeadF32Cols;
            if (lead > nbk - 128) lead = 0;
            // (the split copy of block column k stays in place, rows at their global index: the blocked triangular solves of the
            // posterior read it again -- also when the update itself runs in float32)
            if (h3 && rc == 0 && !panel_split_done) rc = launch_split_rows(p, ld, m, nbk, sw->scale, pk_rows, ldp, la->update);
            if (!f32_first) {
                // the persistent GEMM grid leaves `reserve` compute units to the panel stream, whose small kernels
                // otherwise queue behind 128-KB-LDS workgroups (measured at N = 32768: 0/8/16 -> 62.7 ms, 32 -> 58.7,
                // 24 -> 65.0, 48 -> 58.8, 64 -> 60.4; debug key 4 overrides)
                const int reserve = NNGP_KNOB(4) > 0 ? NNGP_KNOB(4) : 32;
                // one launch: rows [nb2, m) x columns [0, m) of the trailing matrix, on or below its diagonal; columns [lead, nbk)
                // of the panel (K blocks are walked from the high end down)
                if (rc == 0)
                    rc = h3_update_timed(la, c + nb2 * ld, ld, pk_rows + nb2 * ldp + lead * 4, pk_rows + lead * 4, ldp, 0, 1, 0, m - nb2, m,
                                         nbk - lead, -1.0f / (sw->scale * sw->scale), nb2, sw, reserve);
                if (rc == 0 && lead > 0) rc = f32_update_below(c, ld, p, nb2, m, m, lead, la->update);
            } else if (rc == 0) {
                rc = f32_update_below(c, ld, p, nb2, m, m, nbk, la->update);
            }
        } else if (rc == 0 && h3 && nbk == nb && !planes_here) {  // last panel: no trailing update left, but keep its split copy complete
            rc = launch_split_rows(p, ld, m, nbk, sw->scale, pk_rows, ldp, la->update);
        }
    }
    if (rc == 0 && h3) sw->l_ready = true;
    NNGP_TRY(lookahead_join(la, user));
    return rc;
}

// ---- block-column pieces of the right-looking factorisation (multi-GPU: block columns are dealt cyclically) ----
namespace {

// columns of panel [po, po + pw) that stay on the float32 MFMA in its updates: the lead of block column 0, as in the schedules above
int64_t abi_lead(int64_t po, int64_t pw) { return (po == 0 && pw > 256) ? kLeadF32Cols : 0; }

}  // namespace

// Factor block column [o, o+w): Cholesky of the diagonal block, then the rows below times its inverse transpose.
int potrf_panel_f32(float* a, int64_t n, int64_t ld, float* dinv, int32_t* clamped, float pivot_floor, int64_t o,
                    int64_t w, hipStream_t s, SplitWork* sw) {
    NNGP_REQUIRE(o >= 0 && w > 0 && o + w <= n && o % TB == 0 && w % TB == 0, "potrf_panel: bad block column");
    float* akk = a + o * ld + o;
    float* dk = dinv + (o / TB) * TB * TB;
    NNGP_TRY(potrf_rec(akk, w, ld, dk, clamped, pivot_floor, s));
    const int64_t m = n - o - w;
    if (m <= 0) return 0;
    // rows below: ONE fused launch (trsm_panel.hip) as in the single-GPU look-ahead, on the float16 pipe from the second block
    // column on; with the model's split workspace it also leaves the rows' split copy in place (the owner's own updates of this
    // block column then need no separate split pass).
    const bool planes_ok = h3_workspace_ok(sw, n, w) && o % w == 0 && sw->col_stride >= sw->rows_cap * 4 * sw->k_cap;
    if (w <= 1024 && NNGP_KNOB(2) != 4) {
        const int64_t ldp = planes_ok ? 4 * sw->k_cap : 0;
        char* rows = planes_ok ? sw->planes + (o / w) * sw->col_stride + (o + w) * ldp : nullptr;
        NNGP_TRY(solve_rows_below(planes_ok && o > 0, akk, ld, dk, w, sw, akk + w * ld, m, rows, ldp, planes_ok ? sw->scale : 1.0f, s));
        if (planes_ok) sw->split_panel = o;
        return 0;
    }
    return trsm_rlt_f32(akk + w * ld, ld, m, akk, ld, dk, w, s);
}

// Apply the finished block column [po, po+pw) to block column [o, o+w), o >= po + pw:
//   A[o:, o:o+w] -= L[o:, po:po+pw] L[o:o+w, po:po+pw]^T   (lower part of the diagonal block only)
int potrf_update_f32(float* a, int64_t n, int64_t ld, int64_t po, int64_t pw, int64_t o, int64_t w, hipStream_t s,
                     SplitWork* sw) {
    NNGP_REQUIRE(po >= 0 && pw > 0 && o >= po + pw && w > 0 && o + w <= n && o % TB == 0 && w % TB == 0 && po % TB == 0 &&
                     pw % TB == 0, "potrf_update: bad block columns");
    const float* p = a + o * ld + po;   // panel rows [o, n), columns [po, po+pw)
    float* c = a + o * ld + o;
    // float16 pipe (same split copies as the single-GPU look-ahead, so the posterior solves find them afterwards): the
    // panel is split once, when its first update arrives; the leading columns of the first panel stay on the float32 MFMA
    if (h3_workspace_ok(sw, n, pw) && po % pw == 0 && sw->counters != nullptr && (n - o) * w >= 96 * 256 * 256) {
        const int64_t ldp = 4 * sw->k_cap;
        const char* rows = sw->planes + (po / pw) * sw->col_stride + o * ldp;  // rows at their global index
        NNGP_TRY(ensure_panel_split(sw, a, ld, n, po, pw, s));
        const int64_t lead = abi_lead(po, pw);
        NNGP_TRY(launch_gemm_nt_h3(c, ld, rows + lead * 4, rows + lead * 4, ldp, n - o, w, pw - lead, -1.0f / (sw->scale * sw->scale), 1.0f, true,
                                   0, sw->counters, 0, s));
        return f32_update_trap(c, ld, p, p, n - o, w, lead, s);
    }
    return f32_update_trap(c, ld, p, p, n - o, w, pw, s);
}

// The same for SEVERAL target block columns of one rank (multi-GPU: the block columns a rank owns, dealt cyclically): the columns
// that qualify for the float16 pipe go out four to a launch (regions of one split-float16 pass: fewer launches, fewer tails), the
// others one by one as above.  cols: first rows / columns of the targets, ascending, all of width w except possibly the last.
int potrf_update_cols_f32(float* a, int64_t n, int64_t ld, int64_t po, int64_t pw, const int64_t* cols, int ncols, int64_t w,
                          hipStream_t s, SplitWork* sw) {
    NNGP_REQUIRE(cols != nullptr && ncols >= 0 && w > 0 && w % TB == 0, "potrf_update_cols: bad arguments");
    const bool h3 = h3_workspace_ok(sw, n, pw) && po % pw == 0 && sw->counters != nullptr && ld % 4 == 0;
    H3RegionSpec reg[4];
    int nreg = 0;
    const int64_t lead = abi_lead(po, pw);
    auto flush = [&]() -> int {
        if (nreg == 0) return 0;
        const int64_t ldp = 4 * sw->k_cap;
        const char* col = sw->planes + (po / pw) * sw->col_stride;  // rows at their global index
        NNGP_TRY(ensure_panel_split(sw, a, ld, n, po, pw, s));
        NNGP_TRY(launch_gemm_nt_h3r(a, ld, col + lead * 4, col + lead * 4, ldp, 0, 1, 0, reg, nreg, pw - lead, -1.0f / (sw->scale * sw->scale),
                                    1.0f, true, sw->counters, 0, s));
        NNGP_TRY(lead_pass_f32(a, ld, a + po, reg, nreg, lead, s));
        nreg = 0;
        return 0;
    };
    for (int i = 0; i < ncols; ++i) {
        const int64_t o = cols[i];
        const int64_t wi = (n - o < w) ? n - o : w;
        NNGP_REQUIRE(o >= po + pw && o % TB == 0 && wi > 0, "potrf_update_cols: bad target column");
        if (h3 && (n - o) * wi >= 96 * 256 * 256) {
            reg[nreg++] = H3RegionSpec{o, o, n - o, wi, 0};
            if (nreg == 4) NNGP_TRY(flush());
        } else {
            NNGP_TRY(flush());
            NNGP_TRY(potrf_update_f32(a, n, ld, po, pw, o, wi, s, sw));
        }
    }
    return flush();
}

}  // namespace nngp
