// The covariance's residual products at float64 grade on the int8 matrix pipe (kernels: gemm_i8s.hip), as the model uses them: when the
// path is taken, its workspace, the cut of K's digit planes and the streams around it, the products, and the guard that can take a fit
// off the path.  Host code only.  What needs no device -- the size thresholds, the guard's trust record -- is in i8_trust.h.
#include "model.h"

namespace nngp {

// ---- float64-grade residual products on the int8 matrix pipe (gemm_i8s.hip) ----
constexpr int64_t kI8RowBlock = 2048;  // right-hand-side rows per pass (bounds the int32 partial buffer)

// Where it pays (profiles/r3_i8s_crossover.jsonl, predict with the diagonal variance, float64 / int8 residual, ms): a predict that also
// has to cut the planes of K (the first after a fit) wins from two 128-row tiles of right-hand sides on -- N = 2048, M = 256: 0.57 /
// 0.50; N = 8192: M = 128 2.04 / 2.39, M = 256 2.45 / 2.56, M = 512 3.63 / 3.06, M = 1024 5.02 / 3.99; N = 16384, M = 1024: 15.5 / 11.4
// -- later predicts on the same fit from any size on (N = 16384, M = 128: 4.51 / 4.42).  Debug key 5 = 50: float64 matrix pipe instead.
bool use_i8s(const nngp_model* m, int64_t mp) {
    if (m->i8.suspended || m->i8.unavailable || m->i8.trust.distrusted) return false;
    if (NNGP_KNOB(5) == 54) return true;  // timing experiment: at any size (scripts/i8s_crossover.py)
    return i8_coarse_pays(m->np, mp) && NNGP_KNOB(5) != 50;
}

// Two grades of the product.  COARSE: 3 x 5 planes (z ROUNDED to its three and written back, round 4; 5 x 5 before), pairs with
// ia + ib <= 4 (12 exact plane products, 15 before; error ~2^-32 sqrt(N) of the row maxima, all of it from the kernel's side now)
// -- for a FIRST residual.  FINE: 7 x 7 planes, ia + ib <= 6 (28 products; ~2^-48 sqrt(N): what the float64 matrix pipe
// delivers; since late round 4 z is ROUNDED to five planes there as well and written back: 5 x 7 planes, 25 products, the iterate
// moves by 9e-13 of its row maximum) -- for the later residuals and the NTK's W = Z K_dd, where the coarse floor would show (see residual_rows); 28 products
// still cost 3/4 of the float64 product at N = 32768.  A model that will ask for FINE products (NTK fits, covariance levels >= 2)
// has its kernel matrix cut into 7 planes once; coarse products then read the first five of them.
enum { I8_COARSE = 0, I8_FINE = 1 };
constexpr int kI8FinePlanes = 7, kI8FineCut = 6;
constexpr int kI8CoarseZPlanes = 3;  // a first residual's z is rounded to three digits and written back (i8s_product_rows)
constexpr int kI8FineZPlanes = 5;    // a later residual's z (an iterate good to ~1e-8) and the NTK's final Z: rounded to 40 bits below the row maximum (9e-13 of it)

// FINE pays later than COARSE (28 against 15 products): from N = 4096 and four 128-row tiles of right-hand sides on.  Debug key 5 = 57: off.
static bool use_i8s_fine(const nngp_model* m, int64_t mp) { return use_i8s(m, mp) && i8_fine_pays(m->np, mp) && NNGP_KNOB(5) != 57; }
// (want_fine: a predict of this model has needed a FINE product before -- a full covariance at level 1 is promoted to level 2, a weak
// fit's rows continue with later residuals -- so the planes are cut seven deep from the start instead of being thrown away, reallocated
// and cut again in the middle of a predict)
static int i8s_planes_policy(const nngp_model* m) {
    return (m->get == NNGP_GET_NTK || m->var_refine >= 2 || m->i8.want_fine) && NNGP_KNOB(5) != 57 ? kI8FinePlanes : 5;
}


// Workspace of the int8 path: `planes` N^2 bytes of digit planes of the kernel matrix `pk` + the planes and exact plane products of
// one block of rows.  Returns 1 -- and the model stays on the float64 pipe from then on -- when the device has no room for them (a
// kernel matrix that fills most of the 288 GB leaves none): the int8 path is an accelerator, not a requirement.
static int ensure_i8s(nngp_model* m, int64_t mp, I8Planes& pk, int planes) {
    I8Work& w = m->i8.work;
    if (NNGP_KNOB(5) == 51) { w.ns_k = w.ns_z = 4; w.cut = 3; }
    else if (NNGP_KNOB(5) == 52) { w.ns_k = w.ns_z = 6; w.cut = 5; }
    else { w.ns_k = 5; w.ns_z = NNGP_KNOB(5) == 58 ? 5 : kI8CoarseZPlanes; w.cut = 4; }
    if (planes < w.ns_k) planes = w.ns_k;
    w.k_rows = round_up(m->np_cap, 256);
    auto give_up = [&]() -> int {
        dev_free(w.k.planes); dev_free(w.k.scale); dev_free(w.aux.planes); dev_free(w.aux.scale);
        dev_free(w.zplanes); dev_free(w.zscale); dev_free(w.partial); dev_free(w.rowpart);
        w.rowpart_rows = 0;
        w.k.ready = w.aux.ready = false;
        w.k.alloc_planes = w.aux.alloc_planes = 0;
        w.z_rows = 0;
        w.z_planes = 0;
        m->i8.unavailable = true;
        return 1;
    };
    if (pk.alloc_planes < planes) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(pk.planes); dev_free(pk.scale);
        pk.alloc_planes = 0;
        if (!soft_alloc(&pk.planes, planes * w.k_rows * m->np_cap) || !soft_alloc(&pk.scale, m->np_cap + 1)) return give_up();
        NNGP_HIP_CHECK(hipMemset(pk.planes, 0, (size_t)(planes * w.k_rows * m->np_cap)));
        pk.alloc_planes = planes;
        pk.ready = false;
    }
    if (mp > w.rowpart_rows) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(w.rowpart);
        w.rowpart_rows = 0;
        NNGP_TRY(dev_alloc(&w.rowpart, mp * i8s_col_blocks(m->np_cap) * 4));
        w.rowpart_rows = mp;
    }
    if (w.counters == nullptr) {
        NNGP_TRY(dev_alloc(&w.counters, 16));
        NNGP_HIP_CHECK(hipMemset(w.counters, 0, 16 * sizeof(int)));
    }
    const int64_t rows = mp < kI8RowBlock ? mp : kI8RowBlock;
    if (rows > w.z_rows || planes > w.z_planes) {
        NNGP_HIP_CHECK(hipDeviceSynchronize());
        dev_free(w.zplanes); dev_free(w.zscale); dev_free(w.partial);
        const int64_t nr = rows > w.z_rows ? rows : w.z_rows;
        const int np_ = planes > w.z_planes ? planes : w.z_planes;
        w.z_rows = 0;
        w.z_planes = 0;
        if (!soft_alloc(&w.zplanes, np_ * (nr + 256) * m->np_cap) || !soft_alloc(&w.zscale, nr) ||
            !soft_alloc(&w.partial, i8s_chunks(m->np_cap) * np_ * nr * m->np_cap))  // diagonals = cut + 1 <= planes
            return give_up();
        NNGP_HIP_CHECK(hipMemset(w.zplanes, 0, (size_t)(np_ * (nr + 256) * m->np_cap)));
        w.z_rows = nr;
        w.z_planes = np_;
    }
    return 0;
}

// the digit planes of a kernel matrix (as many as were allocated for it).  It is positive semi-definite: row i is bounded by
// sqrt(K_ii max_j K_jj) -- no pass over the matrix for the scales
static int i8s_cut_planes(nngp_model* m, I8Planes& pk, const double* kmat, int64_t kld, hipStream_t s) {
    I8Work& w = m->i8.work;
    NNGP_TRY(launch_i8s_diag_bound_scale(kmat, kld, m->np, pk.scale, s));
    // a bitwise symmetric matrix (one symmetric kernel build; the NNGP kernel beside an NTK fit always is): every entry read once
    const bool sym = (kmat == m->kaux64 || m->k64_symmetric) && (pk.alloc_planes == 5 || pk.alloc_planes == 7) && NNGP_KNOB(5) != 62;
    if (sym)
        NNGP_TRY(launch_i8s_slice_sym(kmat, kld, m->np, pk.alloc_planes, pk.scale, pk.planes, m->np_cap, w.k_rows * m->np_cap, s));
    else
        NNGP_TRY(launch_i8s_slice_rows(kmat, kld, m->np, m->np, pk.alloc_planes, pk.scale, nullptr, pk.planes, m->np_cap, w.k_rows * m->np_cap, s));
    NNGP_TRY(launch_i8s_scale_sqsum(pk.scale, m->np, pk.scale + m->np_cap, s));
    pk.ns_done = pk.alloc_planes;
    pk.ready = true;
    return 0;
}

// out [mp, np] = beta cin + alpha z Kmat + gamma z on the int8 pipe; Kmat: a symmetric positive semi-definite [np, np] kernel matrix
// (k64, or kaux64 beside an NTK fit) whose digit planes are kept in pk (workspace: ensure_i8s, by the caller).
// The planes (13 N^2 bytes of HBM traffic to cut 5 of them: 2.7 ms at N = 32768) are cut once per change of the matrix: by
// nngp_model_predict on the solve stream beside its first blocked solves (-0.8 ms against stream order at N = 32768), else here in
// stream order.  Measured and dropped (profiles/r3_i8s_slicing_placement.json): slicing beside the FACTORISATION on a second stream
// costs the Cholesky exactly what the slicing takes, at any stream priority and wherever in the factorisation it starts -- its 32768
// small workgroups settle on every compute unit a trailing-update launch has just left and the next launch waits for them -- and on
// a CU-masked stream (1 / 2 / 4 units per XCD) it needs 95 / 64 / 55 ms: one compute unit moves ~20 GB/s of it.
static int i8s_product_rows(nngp_model* m, I8Planes& pk, const double* kmat, int64_t kld, double* out, const double* cin, double beta,
                            double alpha, double* z, double gamma, int64_t mp, hipStream_t s, int grade, ResidualNote* note = nullptr) {
    const int64_t np = m->np;
    I8Work& w = m->i8.work;
    // COARSE: z comes straight from the float32 solves and every identity downstream holds for WHATEVER z they returned -- so z is
    // rounded to 24-bit fixed point below its row maximum (three planes; the solves' own error is ~1e-4 of it) and written back:
    // the planes ARE z, planes 3 and 4 do not exist, 12 plane products instead of 15 and no truncation on the z side
    // FINE (round 4, late): the same for the later residuals and the NTK's W = Z K_dd with five planes -- 25 products instead of 28 (timing-knob key 5 = 64: seven)
    const int fine_z = NNGP_KNOB(5) == 64 ? kI8FinePlanes : kI8FineZPlanes;
    const bool round_z = grade == I8_COARSE ? w.ns_z < w.ns_k : fine_z < kI8FinePlanes;
    const bool fuse_rows = grade == I8_COARSE && note != nullptr && note->want_fused_rows && cin != nullptr && w.rowpart_rows >= mp && NNGP_KNOB(5) != 59;
    const int ns_z = grade == I8_FINE ? fine_z : w.ns_z, ns_k = grade == I8_FINE ? kI8FinePlanes : w.ns_k;
    const int cut = grade == I8_FINE ? kI8FineCut : w.cut;
    NNGP_REQUIRE(pk.alloc_planes >= ns_k && w.z_planes >= ns_z, "i8s_product_rows: workspace for %d planes missing", ns_k);
    if (!pk.ready || pk.ns_done < ns_k) {
        NNGP_TRY(i8s_cut_planes(m, pk, kmat, kld, s));
    } else if (&pk == &w.k && m->i8.k_pending) {  // cut on the solve stream at the start of this predict
        NNGP_HIP_CHECK(hipStreamWaitEvent(s, m->i8.ev_i8, 0));
    }
    if (&pk == &w.k) m->i8.k_pending = false;
    I8Plan pl;
    NNGP_TRY(i8s_plan(ns_z, ns_k, cut, &pl));
    const int64_t nchunk = i8s_chunks(np, &pl);
    for (int64_t r0 = 0; r0 < mp; r0 += kI8RowBlock) {
        const int64_t mb = mp - r0 < kI8RowBlock ? mp - r0 : kI8RowBlock;
        const int64_t slab = mb * np;
        NNGP_TRY(launch_i8s_slice_rows(z + r0 * np, np, mb, np, ns_z, nullptr, w.zscale, w.zplanes, m->np_cap, (w.z_rows + 256) * m->np_cap, s,
                                       round_z ? z + r0 * np : nullptr));
        if (r0 == 0 && grade == I8_COARSE && !m->alpha_solve.gate_recorded && NNGP_KNOB(2) != 8 && NNGP_KNOB(2) != 9 && !cg_from_the_start(m, mp)) {
            // The deferred alpha CG (solve stream) starts HERE, not with the blocked solves before this product: its hundreds of small
            // GEMV launches settle on compute units between the solves' persistent split-float16 launches (which need a whole unit's
            // LDS) and cost them 3.7 ms at N = 32768 (scripts/cov_alone.py); beside this one long launch they fit the wave slots and
            // the 32 KB of LDS it leaves.
            NNGP_TRY(record_cg_gate(m, s));
        }
        int slot = -1;
        NNGP_TRY(m->i8.timer.begin(s, &slot));
        NNGP_TRY(launch_gemm_nt_i8s(w.partial, np, slab, w.zplanes, m->np_cap, (w.z_rows + 256) * m->np_cap, pk.planes, m->np_cap,
                                    w.k_rows * m->np_cap, pl, mb, np, np, w.counters, 0, s));
        NNGP_TRY(m->i8.timer.end(slot));
        if (slot >= 0) {
            w.t_flops[slot] = 2.0 * (double)mb * (double)np * (double)np;
            w.t_ops[slot] = w.t_flops[slot] * pl.npairs;
        }
        I8Fuse fuse;
        fuse.out32 = m->b32 + r0 * np;
        fuse.ld32 = np;
        fuse.part = w.rowpart + r0 * i8s_col_blocks(np) * 4;
        NNGP_TRY(launch_i8s_combine(out + r0 * np, np, cin ? cin + r0 * np : nullptr, np, beta, alpha, z + r0 * np, np, gamma, w.partial, np,
                                    slab, (int)nchunk, pl.ndiag, w.zscale, pk.scale, mb, np, s, fuse_rows ? &fuse : nullptr));
    }
    if (fuse_rows) note->fused = true;
    // timing experiment: the CG starts when the product has ended
    if (grade == I8_COARSE && !m->alpha_solve.gate_recorded && NNGP_KNOB(2) == 9) NNGP_TRY(record_cg_gate(m, s));
    return 0;
}

// out [mp, np] = rhs - z (K + reg I) for z = z64 (or another [mp, np] block).
// first_residual: z comes straight from the float32 solves, so the residual is ~1e-4 of rhs and the COARSE product's error floor
// (2^-32 sqrt(N) of the row maxima, ~1e-3 of such a residual) is harmless: the NNGP level-1 variance moves by 2e-7 (N = 32768) ..
// 7e-7 (ill-conditioned sweep case), a first correction sweep loses nothing.  Every LATER residual is ~1e-8 of rhs and needs float64
// grade proper -- measured with the coarse product there (scripts/i8s_hard_case.py): NTK variances off by 3e-5 .. 2e-4 (first order
// in the rows' error) against 1e-8, NNGP level 2 at 1e-7 instead of 1e-8, the explicit inverse of the serving mode stuck four digits
// short of float64 (serving variances 4e-3 off).  Those take the FINE product where it pays, else the float64 pipe.
// note (optional): what the caller asks of this residual and learns about it (ResidualNote).
int residual_rows(nngp_model* m, double* out, const double* rhs, double* z, int64_t mp, hipStream_t s, bool first_residual,
                  ResidualNote* note) {
    const int64_t np = m->np;
    const bool coarse = first_residual;
    if (!coarse && use_i8s_fine(m, mp)) m->i8.want_fine = true;
    if (coarse ? use_i8s(m, mp) : use_i8s_fine(m, mp)) {
        const int rc = ensure_i8s(m, mp, m->i8.work.k, coarse ? i8s_planes_policy(m) : kI8FinePlanes);
        if (rc == 0) {
            if (coarse && note != nullptr) note->used_int8 = true;
            return i8s_product_rows(m, m->i8.work.k, m->k64, m->ld, out, rhs, 1.0, -1.0, z, -m->reg, mp, s, coarse ? I8_COARSE : I8_FINE,
                                    note);
        }
        if (rc != 1) return rc;  // 1: no room for the planes -- the float64 pipe below
    }
    NNGP_TRY(launch_gemm_nt_f64(out, np, rhs, np, z, np, m->k64, m->ld, mp, np, np, -1.0, 1.0, s));
    return launch_axpby_mat(out, 1.0, z, -m->reg, np, mp, np, s);
}

// NTK: out [mp, np] = z K_aux, the NNGP kernel of the training rows beside the fit's own (W = Z K_dd).  Its error is the variance's --
// float64 grade proper (the FINE product where it pays)
int kaux_product_rows(nngp_model* m, double* out, double* z, int64_t mp, hipStream_t s) {
    const int64_t np = m->np;
    const int rc_w = use_i8s_fine(m, mp) ? ensure_i8s(m, mp, m->i8.work.aux, kI8FinePlanes) : 1;
    if (rc_w == 0) return i8s_product_rows(m, m->i8.work.aux, m->kaux64, np, out, nullptr, 0.0, 1.0, z, 0.0, mp, s, I8_FINE);
    if (rc_w != 1) return rc_w;
    return launch_gemm_nt_f64(out, np, nullptr, 0, z, np, m->kaux64, np, mp, np, np, 1.0, 0.0, s);
}

// Stage 2.  A predict whose covariance will take the int8 residual product right after a fit: the digit planes of K (13 N^2 bytes of HBM
// traffic, 2.7 ms alone at N = 32768) are cut beside the predict's first kernels.  The cut's workgroups hold 132 KB of LDS and cannot
// share a compute unit with a workgroup of the persistent solves, so what is left of it when the first solve starts waits for the
// gaps between and behind the solves: it is enqueued FIRST (round 5: before the cross kernel and the inverted blocks, on the
// look-ahead's idle update stream -- it needs nothing but K) and has the chip until then.  (debug key 5 = 53: in stream order
// where the planes are first needed)
int cut_planes_early(nngp_model* m, PredictCall& c) {
    if (!(c.want_cov && m->var_refine >= 1 && use_i8s(m, c.mp) && !c.serving && NNGP_KNOB(5) != 53)) return 0;
    I8Residual& r = m->i8;
    if (c.full && use_i8s_fine(m, c.mp)) r.want_fine = true;  // a full covariance runs at level >= 2: later residuals
    const int rc_i8 = ensure_i8s(m, c.mp, r.work.k, i8s_planes_policy(m));
    if (rc_i8 != 0 && rc_i8 != 1) return rc_i8;
    if (rc_i8 != 0 || r.work.k.ready) return 0;
    if (r.ev_i8 == nullptr) NNGP_HIP_CHECK(hipEventCreateWithFlags(&r.ev_i8, hipEventDisableTiming));
    NNGP_HIP_CHECK(hipEventRecord(r.ev_i8, c.s));  // K is complete; earlier readers of the planes are behind us
    const hipStream_t cs = early_cut_stream(m, c.mp);
    NNGP_HIP_CHECK(hipStreamWaitEvent(cs, r.ev_i8, 0));
    NNGP_TRY(i8s_cut_planes(m, r.work.k, m->k64, m->ld, cs));
    NNGP_HIP_CHECK(hipEventRecord(r.ev_i8, cs));
    r.k_pending = true;
    return 0;
}

// the guard's word and its pinned mirror (level-1 variances)
static int ensure_guard_word(nngp_model* m) {
    if (m->i8.guard != nullptr) return 0;
    NNGP_TRY(dev_alloc(&m->i8.guard, 1));
    NNGP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m->i8.guard_host), sizeof(unsigned long long), hipHostMallocDefault));
    return 0;
}

// nngp_model_reserve: what a predict of mp padded rows with this covariance mode would allocate for the path
int i8s_reserve(nngp_model* m, int64_t mp, int32_t cov_mode) {
    if (!(i8_coarse_pays(m->np_cap, mp) && !m->i8.unavailable && (m->var_refine >= 1 || m->get == NNGP_GET_NTK))) return 0;
    if (cov_mode == NNGP_COV_FULL && i8_fine_pays(m->np_cap, mp)) m->i8.want_fine = true;
    const int rc = ensure_i8s(m, mp, m->i8.work.k, i8s_planes_policy(m));
    if (rc != 0 && rc != 1) return rc;
    if (rc == 0) NNGP_TRY(ensure_guard_word(m));
    return 0;
}

// K has new entries (nngp_model_build_rows, nngp_model_append): its planes are stale, and the new fit is trusted again
void i8s_kernel_changed(nngp_model* m) {
    m->i8.work.k.ready = false;
    m->i8.trust.new_kernel();
}

// the guard's threshold (key 5 = 56: distrust whatever the estimate says (test))
static double guard_threshold() { return NNGP_KNOB(5) == 56 ? 0.0 : kI8FloorThr; }

// An int8 residual went into a level-1 batch: what may the dropped digit pairs have cost THIS batch's variances?  The estimate's one
// word waits for the first predict's verdict (first_guard_verdict), or travels to the host for the NEXT predict (take_in_guard_word).
int record_i8_guard_estimate(nngp_model* m, PredictCall& c) {
    I8Residual& r = m->i8;
    const I8Work& w = r.work;
    I8Plan pl;
    NNGP_TRY(i8s_plan(w.ns_z, w.ns_k, w.cut, &pl));
    NNGP_TRY(ensure_guard_word(m));
    if (r.ev_guard == nullptr) NNGP_HIP_CHECK(hipEventCreateWithFlags(&r.ev_guard, hipEventDisableTiming));
    NNGP_HIP_CHECK(hipMemsetAsync(r.guard, 0, sizeof(unsigned long long), c.s));
    NNGP_TRY(launch_i8s_floor_ratio_rows(m->rows.zstat, c.mt, c.var_or_cov, pl, w.ns_z, w.ns_k, w.k.scale + m->np_cap, r.guard, c.s));
    if (!r.trust.checked) {
        c.i8_check_pending = true;   // first predict of the fit: waits for its own estimate (first_guard_verdict)
    } else {
        NNGP_HIP_CHECK(hipMemcpyAsync(r.guard_host, r.guard, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.s));
        NNGP_HIP_CHECK(hipEventRecord(r.ev_guard, c.s));
        r.trust.pending = true;  // looked at when the next predict starts
    }
    return 0;
}

// Stage 5: the previous level-1 batch's guard estimate, if it has arrived (record_i8_guard_estimate sent it on its way)
void take_in_guard_word(nngp_model* m) {
    if (!(m->i8.trust.pending && hipEventQuery(m->i8.ev_guard) == hipSuccess)) return;
    double ratio = 0.0;
    memcpy(&ratio, m->i8.guard_host, sizeof(double));
    m->i8.trust.fold(ratio, guard_threshold());  // distrusted: float64 pipe from this predict on
}

// Stage 8: the first level-1 predict of a fit on the int8 residual waits for its own guard estimate; distrusted (*redo), the covariance
// is formed again on the float64 pipe, where the fit stays.
// (the host has just waited for the alpha solve: this read-back waits for the covariance kernels enqueued before it, once
// per fit -- later predicts on the fit stay asynchronous)
int first_guard_verdict(nngp_model* m, PredictCall& c, bool* redo) {
    *redo = false;
    if (!c.i8_check_pending) return 0;
    NNGP_HIP_CHECK(hipMemcpyAsync(m->i8.guard_host, m->i8.guard, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.s));
    NNGP_HIP_CHECK(hipStreamSynchronize(c.s));
    double ratio = 0.0;
    memcpy(&ratio, m->i8.guard_host, sizeof(double));
    if (!m->i8.trust.first_verdict(ratio, guard_threshold())) return 0;
    c.used_i8 = false;  // use_i8s is false from here on: the covariance again, on the float64 pipe
    *redo = true;
    return 0;
}

// ---- nngp_model_residual_timer[_read], nngp_model_residual_floor (api.hip) ----

int i8s_timer_enable(nngp_model* m, int32_t enable) {
    m->i8.timer.enable(enable != 0);
    return 0;
}

int i8s_timer_read(nngp_model* m, int64_t* launches, double* ms_total, double* flops_total, double* int8_ops_total) {
    const I8Work& w = m->i8.work;
    auto& timer = m->i8.timer;
    double ms = 0.0, fl = 0.0, ops = 0.0;
    NNGP_TRY(timer.read(&ms));
    for (int t = 0; t < timer.count; ++t) {
        fl += w.t_flops[t];
        ops += w.t_ops[t];
    }
    if (launches) *launches = timer.count;
    if (ms_total) *ms_total = ms;
    if (flops_total) *flops_total = fl;
    if (int8_ops_total) *int8_ops_total = ops;
    timer.count = 0;
    return 0;
}

int i8s_residual_floor(nngp_model* m, double* ratio, int32_t* distrusted) {
    I8Residual& r = m->i8;
    if (r.trust.pending && r.ev_guard != nullptr) {  // the last level-1 batch's own estimate: wait for it and fold it in, so that a
        NNGP_HIP_CHECK(hipEventSynchronize(r.ev_guard));  // caller can ask after a batch whether THAT batch tripped the guard
        double est = 0.0;
        memcpy(&est, r.guard_host, sizeof(double));
        r.trust.fold(est, kI8FloorThr);
    }
    if (ratio) *ratio = r.trust.checked ? r.trust.floor_ratio : -1.0;
    if (distrusted) *distrusted = r.trust.distrusted ? 1 : 0;
    return 0;
}

}  // namespace nngp
