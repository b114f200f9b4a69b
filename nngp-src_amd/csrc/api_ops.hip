// Stand-alone operator entry points of the C ABI (no model object): the factorisation, the GEMMs, pool selection, the ticket tables --
// what tests/, scripts/ and the multi-GPU drivers call directly.
#include "model.h"
#include "gp_f64.h"
#include "trsm_order.h"
#include "../../include/nngp_i8s.h"

extern "C" {

int nngp_trsm_ticket_order(int32_t row_tiles, int32_t block_cols, int32_t tail_tiles, int32_t backward, int32_t workers, int32_t merged,
                           int32_t* items, int64_t cap, int64_t* count) {
    return tk_order_export(row_tiles, block_cols, tail_tiles, backward, workers, merged, 1, items, nullptr, cap, count);
}

int nngp_trsm_ticket_queues(int32_t row_tiles, int32_t block_cols, int32_t tail_tiles, int32_t backward, int32_t workers, int32_t merged,
                            int32_t queues, int32_t* items, int32_t* queue_of, int64_t cap, int64_t* count) {
    return tk_order_export(row_tiles, block_cols, tail_tiles, backward, workers, merged, queues, items, queue_of, cap, count);
}

int nngp_potrf_f32(float* a, int64_t n, int64_t ld, float* dinv, int32_t* clamped, void* stream) {
    NNGP_REQUIRE(a != nullptr && dinv != nullptr, "potrf_f32: NULL argument");
    if (clamped) NNGP_HIP_CHECK(hipMemsetAsync(clamped, 0, sizeof(int32_t), (hipStream_t)stream));
    return potrf_f32(a, n, ld, dinv, clamped, 0.0f, (hipStream_t)stream);
}

int nngp_potrf_f64(double* a, int64_t n, int64_t ld, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(a != nullptr && n > 0 && n % TB == 0, "potrf_f64: n must be a positive multiple of %d (n=%lld)", TB, (long long)n);
    double* dinv = nullptr;
    int* status = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&dinv), sizeof(double) * (size_t)n * TB, s));
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&status), sizeof(int), s));
    int rc = potrf_f64(a, n, ld, dinv, status, s);
    if (rc == 0) rc = potrf_f64_status(status, s, "potrf_f64");
    (void)hipFreeAsync(dinv, s);
    (void)hipFreeAsync(status, s);
    return rc;
}

int nngp_potrf_dinv_f64(double* a, int64_t n, int64_t ld, double* dinv, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(a != nullptr && dinv != nullptr && n > 0 && n % TB == 0, "potrf_dinv_f64: n must be a positive multiple of %d (n=%lld)", TB,
                 (long long)n);
    NNGP_REQUIRE(((uintptr_t)dinv & 15) == 0, "potrf_dinv_f64: dinv must be 16-byte aligned");
    int* status = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&status), sizeof(int), s));
    int rc = potrf_f64(a, n, ld, dinv, status, s);
    if (rc == 0) rc = potrf_f64_status(status, s, "potrf_dinv_f64");
    (void)hipFreeAsync(status, s);
    return rc;
}

int nngp_trsm_fwd_f64(double* bt, int64_t ldb, int64_t rows, const double* l, int64_t ldl, const double* dinv, int64_t n, int32_t tri,
                      void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(bt != nullptr && l != nullptr && dinv != nullptr, "trsm_fwd_f64: NULL argument");
    NNGP_REQUIRE(rows > 0 && n > 0 && rows % TB == 0 && n % TB == 0, "trsm_fwd_f64: rows, n must be positive multiples of %d (rows=%lld n=%lld)",
                 TB, (long long)rows, (long long)n);
    NNGP_REQUIRE(tri == 0 || rows == n, "trsm_fwd_f64: the triangular mode solves the identity, rows must equal n (rows=%lld n=%lld)",
                 (long long)rows, (long long)n);
    // what the GEMMs inside would reject after the first launches: said here, before any
    NNGP_REQUIRE(ldb >= n && ldl >= n && ldb % 2 == 0 && ldl % 2 == 0, "trsm_fwd_f64: ldb, ldl must be >= n and even (ldb=%lld ldl=%lld n=%lld)",
                 (long long)ldb, (long long)ldl, (long long)n);
    NNGP_REQUIRE((((uintptr_t)bt | (uintptr_t)l | (uintptr_t)dinv) & 15) == 0, "trsm_fwd_f64: operands must be 16-byte aligned");
    double* t = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&t), sizeof(double) * (size_t)rows * TB, s));
    const int rc = trsm_fwd_f64(bt, ldb, rows, l, ldl, dinv, n, t, tri != 0, s);
    (void)hipFreeAsync(t, s);
    return rc;
}

namespace {
// the body of nngp_factor_solve_f64 on its workspace (the caller frees it whatever happens here)
int factor_solve_on(GpWorkspace* w, const double* a, int64_t lda, const double* y, int64_t n, int mode, double* l, double* wout,
                    double* zt, double* ainv, double* alpha, double* neg_rowsq, hipStream_t s) {
    const int64_t np = round_up(n, TB);
    NNGP_TRY(ws_alloc(w, n, 1, 1, 1, np));
    NNGP_TRY(ws_set_train(w, y, y, hipMemcpyDeviceToDevice, n, s));  // no inputs here: y stands in for the n x 1 "x"
    hipLaunchKernelGGL(k_eye, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, s, w->a, np, np);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_HIP_CHECK(hipMemcpy2DAsync(w->a, sizeof(double) * np, a, sizeof(double) * lda, sizeof(double) * n, n, hipMemcpyDeviceToDevice, s));
    NNGP_TRY(factor_and_solve(w, mode, "factor_solve_f64", s, mode == kGpSolveW ? nullptr : neg_rowsq));
    const size_t vec = sizeof(double) * np, mat = vec * np;
    if (l) NNGP_HIP_CHECK(hipMemcpyAsync(l, w->a, mat, hipMemcpyDeviceToDevice, s));
    if (wout) NNGP_HIP_CHECK(hipMemcpyAsync(wout, w->wrow, vec, hipMemcpyDeviceToDevice, s));
    if (zt) NNGP_HIP_CHECK(hipMemcpyAsync(zt, w->zt, mat, hipMemcpyDeviceToDevice, s));
    if (ainv) NNGP_HIP_CHECK(hipMemcpyAsync(ainv, w->ainv, mat, hipMemcpyDeviceToDevice, s));
    if (alpha) NNGP_HIP_CHECK(hipMemcpyAsync(alpha, w->alpha, vec, hipMemcpyDeviceToDevice, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}
}  // namespace

int nngp_factor_solve_f64(const double* a, int64_t lda, const double* y, int64_t n, int32_t mode, double* l, double* w, double* zt,
                          double* ainv, double* alpha, double* neg_rowsq, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(a != nullptr && y != nullptr && n >= 1 && lda >= n, "factor_solve_f64: need a, y, n >= 1 and lda >= n (n=%lld lda=%lld)",
                 (long long)n, (long long)lda);
    NNGP_REQUIRE(mode == kGpSolveW || mode == kGpSolveInverse || mode == kGpSolveRows, "factor_solve_f64: unknown mode %d", (int)mode);
    NNGP_REQUIRE(mode != kGpSolveW || (zt == nullptr && alpha == nullptr && neg_rowsq == nullptr),
                 "factor_solve_f64: mode 0 produces L and w only");
    NNGP_REQUIRE(mode == kGpSolveInverse || ainv == nullptr, "factor_solve_f64: only mode 1 produces A^-1");
    GpWorkspace ws;
    const int rc = factor_solve_on(&ws, a, lda, y, n, mode, l, w, zt, ainv, alpha, neg_rowsq, s);
    if (rc != 0) (void)hipStreamSynchronize(s);
    ws_free(&ws);
    return rc;
}

int nngp_gemm_nt_f32(float* c, int64_t ldc, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m,
                     int64_t n, int64_t k, float alpha, float beta, int32_t lower_only, void* stream) {
    NNGP_REQUIRE(a != nullptr && b != nullptr && c != nullptr, "gemm_nt_f32: NULL argument");
    return launch_gemm_nt_f32(c, ldc, a, lda, b, ldb, m, n, k, alpha, beta, lower_only != 0, (hipStream_t)stream);
}

// Split workspace of nngp_gemm_nt_h3, kept between calls (round 4; until then every call allocated, synchronised and freed -- a host
// wait and a hipMalloc per block column inside the distributed factorisation's collective loop): one grow-only buffer per stream, a
// few streams at most; work on one stream is ordered, so the buffer is reused without waiting.
namespace {
struct H3Scratch {
    hipStream_t stream = nullptr;
    char* p = nullptr;
    size_t bytes = 0;
    bool used = false;
};
std::mutex g_h3_scratch_mutex;
H3Scratch g_h3_scratch[4];

int h3_scratch_get(hipStream_t s, size_t bytes, char** out) {
    std::lock_guard<std::mutex> lock(g_h3_scratch_mutex);
    H3Scratch* e = nullptr;
    for (auto& c : g_h3_scratch)
        if (c.used && c.stream == s) e = &c;
    if (e == nullptr)
        for (auto& c : g_h3_scratch)
            if (!c.used && e == nullptr) e = &c;
    if (e == nullptr) {  // every slot belongs to another stream: take the first one over once its work is through
        e = &g_h3_scratch[0];
        // (the stored handle may belong to a stream its owner has destroyed since: then the whole device is waited for instead)
        if (hipStreamSynchronize(e->stream) != hipSuccess) {
            (void)hipGetLastError();
            NNGP_HIP_CHECK(hipDeviceSynchronize());
        }
        (void)hipFree(e->p);
        *e = H3Scratch();
    }
    if (e->bytes < bytes) {
        if (e->p != nullptr) {
            NNGP_HIP_CHECK(hipStreamSynchronize(s));
            (void)hipFree(e->p);
            e->p = nullptr;
            e->bytes = 0;
        }
        NNGP_HIP_CHECK(hipMalloc((void**)&e->p, bytes));
        e->bytes = bytes;
    }
    e->used = true;
    e->stream = s;
    *out = e->p;
    return 0;
}
}  // namespace

int nngp_gemm_nt_h3(float* c, int64_t ldc, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m, int64_t n,
                    int64_t k, float alpha, float beta, float scale, int32_t lower_only, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(a != nullptr && b != nullptr && c != nullptr && scale > 0.0f, "gemm_nt_h3: bad argument");
    NNGP_REQUIRE(m > 0 && n > 0 && k > 0 && k % 32 == 0, "gemm_nt_h3: k must be a multiple of 32");
    const int64_t mp = round_up(m, 256), np = round_up(n, 256), ldp = 4 * k;
    char* pa = nullptr;
    NNGP_TRY(h3_scratch_get(s, (size_t)((mp + np) * ldp + 64), &pa));
    char* pb = pa + mp * ldp;
    int* counters = reinterpret_cast<int*>(pb + np * ldp);
    // the padding rows' products are never stored, but they are read: zero (finite) operands; the work counters start at zero
    if (mp > m) NNGP_HIP_CHECK(hipMemsetAsync(pa + m * ldp, 0, (size_t)((mp - m) * ldp), s));
    NNGP_HIP_CHECK(hipMemsetAsync(pb + n * ldp, 0, (size_t)((np - n) * ldp + 64), s));
    NNGP_TRY(launch_split_rows(a, lda, m, k, scale, pa, ldp, s));
    NNGP_TRY(launch_split_rows(b, ldb, n, k, scale, pb, ldp, s));
    return launch_gemm_nt_h3(c, ldc, pa, pb, ldp, m, n, k, alpha / (scale * scale), beta, lower_only != 0, 0, counters,
                             NNGP_KNOB(4) > 0 ? NNGP_KNOB(4) : 0, s);
}

int nngp_gemm_nt_f64(double* c, int64_t ldc, const double* cin, int64_t ldcin, const double* a, int64_t lda,
                     const double* b, int64_t ldb, int64_t m, int64_t n, int64_t k, double alpha, double beta,
                     void* stream) {
    NNGP_REQUIRE(a != nullptr && b != nullptr && c != nullptr, "gemm_nt_f64: NULL argument");
    return launch_gemm_nt_f64(c, ldc, cin, ldcin, a, lda, b, ldb, m, n, k, alpha, beta, (hipStream_t)stream);
}

int nngp_gemm_nt_i8s(double* c, int64_t ldc, const double* cin, int64_t ldcin, const double* a, int64_t lda, const double* b,
                     int64_t ldb, int64_t m, int64_t n, int64_t k, double alpha, double beta, int32_t slices_a, int32_t slices_b,
                     int32_t cut, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(a != nullptr && b != nullptr && c != nullptr && m > 0 && n > 0 && k > 0 && m % TB == 0 && n % TB == 0 && ldc >= n &&
                     lda >= k && ldb >= k,
                 "gemm_nt_i8s: m, n must be multiples of %d", TB);
    I8Plan pl;
    NNGP_TRY(i8s_plan(slices_a, slices_b, cut, &pl));
    const int64_t mp = round_up(m, 256), np = round_up(n, 256), kp = round_up(k, 128);
    const int64_t nchunk = i8s_chunks(k, &pl);
    const int64_t slab = m * n;
    const size_t plane_bytes = (size_t)((mp * slices_a + np * slices_b) * kp);
    const size_t part_bytes = (size_t)(nchunk * pl.ndiag * slab) * sizeof(int32_t);
    NNGP_REQUIRE(part_bytes < (size_t)16 << 30, "gemm_nt_i8s: the test entry keeps all partial products (16 GB limit)");
    char* ws = nullptr;
    NNGP_HIP_CHECK(hipMalloc((void**)&ws, plane_bytes + part_bytes + sizeof(double) * (size_t)(m + n) + 64));
    NNGP_HIP_CHECK(hipMemsetAsync(ws, 0, plane_bytes, s));
    int8_t* pa = reinterpret_cast<int8_t*>(ws);
    int8_t* pb = pa + mp * slices_a * kp;
    int32_t* part = reinterpret_cast<int32_t*>(ws + plane_bytes);
    double* sca = reinterpret_cast<double*>(ws + plane_bytes + part_bytes);
    double* scb = sca + m;
    int* counters = reinterpret_cast<int*>(scb + n);
    NNGP_HIP_CHECK(hipMemsetAsync(counters, 0, 64, s));
    int rc = launch_i8s_slice_rows(a, lda, m, k, slices_a, nullptr, sca, pa, kp, mp * kp, s);
    if (rc == 0) rc = launch_i8s_slice_rows(b, ldb, n, k, slices_b, nullptr, scb, pb, kp, np * kp, s);
    if (rc == 0)
        rc = launch_gemm_nt_i8s(part, n, slab, pa, kp, mp * kp, pb, kp, np * kp, pl, m, n, k, counters,
                                NNGP_KNOB(4) > 0 ? NNGP_KNOB(4) : 0, s);
    if (rc == 0)
        rc = launch_i8s_combine(c, ldc, cin ? cin : c, cin ? ldcin : ldc, beta, alpha, nullptr, 0, 0.0, part, n, slab, (int)nchunk,
                                pl.ndiag, sca, scb, m, n, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(ws);
    return rc;
}

// ---- include/nngp_i8s.h: the launches of the int8 residual pipeline without a model object (tests/test_gpu_i8s.py) ----
// i8s_cut_planes and i8s_product_rows (residual_i8.hip) take their buffers, events, timers and the alpha CG's gate from nngp_model;
// the operators below issue the same launch_i8s_* / launch_gemm_nt_i8s calls in the same order on a workspace of their own.
int nngp_i8s_cut_rows(const double* src, int64_t ld, int64_t rows, int64_t cols, int32_t ns, const double* scale_in, double* scale_out,
                      int8_t* planes, int64_t ldp, double* writeback, void* stream) {
    NNGP_REQUIRE(src != nullptr && planes != nullptr && (scale_in != nullptr || scale_out != nullptr), "i8s_cut_rows: NULL argument");
    NNGP_REQUIRE(ns >= 2 && ns <= 7, "i8s_cut_rows: 2..7 planes (ns=%d)", (int)ns);
    NNGP_REQUIRE(rows > 0 && cols > 0 && ld >= cols && ld % 2 == 0, "i8s_cut_rows: ld must be even and >= cols (rows=%lld cols=%lld ld=%lld)",
                 (long long)rows, (long long)cols, (long long)ld);
    NNGP_REQUIRE(ldp >= round_up(cols, 128) && ldp % 16 == 0, "i8s_cut_rows: ldp must be a multiple of 16 and >= cols rounded up to 128 (ldp=%lld)",
                 (long long)ldp);
    NNGP_REQUIRE((((uintptr_t)src | (uintptr_t)planes | (uintptr_t)writeback) & 15) == 0, "i8s_cut_rows: operands must be 16-byte aligned");
    return launch_i8s_slice_rows(src, ld, rows, cols, ns, scale_in, scale_out, planes, ldp, rows * ldp, (hipStream_t)stream, writeback);
}

int nngp_i8s_cut_sym(const double* src, int64_t ld, int64_t n, int32_t ns, double* scale_out, int8_t* planes, int64_t ldp,
                     int32_t by_rows, double* sqsum, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(src != nullptr && planes != nullptr && scale_out != nullptr, "i8s_cut_sym: NULL argument");
    NNGP_REQUIRE(by_rows != 0 ? (ns >= 2 && ns <= 7) : (ns == 5 || ns == 7), "i8s_cut_sym: 5 or 7 planes (by rows: 2..7) (ns=%d)", (int)ns);
    NNGP_REQUIRE(n > 0 && n % TB == 0 && ld >= n && ld % 2 == 0, "i8s_cut_sym: n must be a positive multiple of %d, ld even and >= n (n=%lld ld=%lld)",
                 TB, (long long)n, (long long)ld);
    NNGP_REQUIRE(ldp >= n && ldp % 16 == 0, "i8s_cut_sym: ldp must be a multiple of 16 and >= n (ldp=%lld)", (long long)ldp);
    NNGP_REQUIRE((((uintptr_t)src | (uintptr_t)planes) & 15) == 0, "i8s_cut_sym: operands must be 16-byte aligned");
    NNGP_TRY(launch_i8s_diag_bound_scale(src, ld, n, scale_out, s));
    if (by_rows != 0)
        NNGP_TRY(launch_i8s_slice_rows(src, ld, n, n, ns, scale_out, nullptr, planes, ldp, n * ldp, s));
    else
        NNGP_TRY(launch_i8s_slice_sym(src, ld, n, ns, scale_out, planes, ldp, n * ldp, s));
    if (sqsum != nullptr) NNGP_TRY(launch_i8s_scale_sqsum(scale_out, n, sqsum, s));
    return 0;
}

namespace {
struct I8sResidualWs {  // one allocation, carved up
    int8_t *kplanes, *zplanes;
    double *kscale, *zscale, *rowpart;
    int32_t* partial;
    int* counters;
};

int i8s_residual_on(const I8sResidualWs& w, const I8Plan& pl, double* out, int64_t ldo, const double* cin, int64_t ldcin, double* z, int64_t ldz,
                    const double* kmat, int64_t ldk, int64_t mp, int64_t n, double alpha, double beta, double gamma, int ns_z, int ns_k,
                    bool round_z, bool sym, float* out32, const double* base, double* var, double* delta, double* zstat,
                    double* floor_rows, double* floor_z, hipStream_t s) {
    const int64_t kr = round_up(n, 256), zr = round_up(mp, 256);
    // the kernel matrix's planes: scales from the diagonal, no pass over the matrix (i8s_cut_planes)
    NNGP_TRY(launch_i8s_diag_bound_scale(kmat, ldk, n, w.kscale, s));
    if (sym)
        NNGP_TRY(launch_i8s_slice_sym(kmat, ldk, n, ns_k, w.kscale, w.kplanes, n, kr * n, s));
    else
        NNGP_TRY(launch_i8s_slice_rows(kmat, ldk, n, n, ns_k, w.kscale, nullptr, w.kplanes, n, kr * n, s));
    NNGP_TRY(launch_i8s_scale_sqsum(w.kscale, n, w.kscale + n, s));
    // z's planes, the exact plane products, the combination (i8s_product_rows)
    const int64_t nchunk = i8s_chunks(n, &pl), slab = mp * n;
    NNGP_TRY(launch_i8s_slice_rows(z, ldz, mp, n, ns_z, nullptr, w.zscale, w.zplanes, n, zr * n, s, round_z ? z : nullptr));
    NNGP_TRY(launch_gemm_nt_i8s(w.partial, n, slab, w.zplanes, n, zr * n, w.kplanes, n, kr * n, pl, mp, n, n, w.counters, 0, s));
    I8Fuse fuse;
    fuse.out32 = out32;
    fuse.ld32 = n;
    fuse.part = w.rowpart;
    NNGP_TRY(launch_i8s_combine(out, ldo, cin, ldcin, beta, alpha, z, ldz, gamma, w.partial, n, slab, (int)nchunk, pl.ndiag, w.zscale,
                                w.kscale, mp, n, s, out32 != nullptr ? &fuse : nullptr));
    if (out32 != nullptr) {
        NNGP_TRY(launch_i8s_rowstat_finish(w.rowpart, n, mp, base, var, delta, zstat, s));
        if (floor_rows != nullptr) {
            NNGP_HIP_CHECK(hipMemsetAsync(floor_rows, 0, sizeof(double), s));
            NNGP_TRY(launch_i8s_floor_ratio_rows(zstat, mp, var, pl, ns_z, ns_k, w.kscale + n, reinterpret_cast<unsigned long long*>(floor_rows), s));
        }
        if (floor_z != nullptr) {
            NNGP_HIP_CHECK(hipMemsetAsync(floor_z, 0, sizeof(double), s));
            NNGP_TRY(launch_i8s_floor_ratio(z, ldz, mp, n, var, pl, ns_z, ns_k, w.kscale + n, reinterpret_cast<unsigned long long*>(floor_z), s));
        }
    }
    return 0;
}
}  // namespace

int nngp_i8s_residual(double* out, int64_t ldo, const double* cin, int64_t ldcin, double* z, int64_t ldz, const double* kmat,
                      int64_t ldk, int64_t mp, int64_t n, double alpha, double beta, double gamma, int32_t ns_z, int32_t ns_k,
                      int32_t cut, int32_t round_z, int32_t sym, float* out32, const double* base, double* var, double* delta,
                      double* zstat, double* floor_rows, double* floor_z, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(out != nullptr && z != nullptr && kmat != nullptr && (beta == 0.0 || cin != nullptr), "i8s_residual: NULL argument");
    NNGP_REQUIRE(mp > 0 && n > 0 && mp % TB == 0 && n % TB == 0, "i8s_residual: mp, n must be positive multiples of %d (mp=%lld n=%lld)", TB,
                 (long long)mp, (long long)n);
    NNGP_REQUIRE(ns_z >= 2 && ns_z <= 7 && ns_k >= 2 && ns_k <= 7, "i8s_residual: 2..7 planes per operand (ns_z=%d ns_k=%d)", (int)ns_z, (int)ns_k);
    NNGP_REQUIRE(cut >= 0, "i8s_residual: cut must be >= 0 (cut=%d)", (int)cut);
    NNGP_REQUIRE(sym == 0 || ns_k == 5 || ns_k == 7, "i8s_residual: the symmetric cut makes 5 or 7 planes (ns_k=%d)", (int)ns_k);
    NNGP_REQUIRE(ldo >= n && ldz >= n && ldk >= n && (cin == nullptr || ldcin >= n) && ldo % 2 == 0 && ldz % 2 == 0 && ldk % 2 == 0 &&
                     (cin == nullptr || ldcin % 2 == 0),
                 "i8s_residual: leading dimensions must be even and >= n (ldo=%lld ldcin=%lld ldz=%lld ldk=%lld)", (long long)ldo,
                 (long long)ldcin, (long long)ldz, (long long)ldk);
    NNGP_REQUIRE((((uintptr_t)out | (uintptr_t)cin | (uintptr_t)z | (uintptr_t)kmat | (uintptr_t)out32) & 15) == 0,
                 "i8s_residual: operands must be 16-byte aligned");
    const bool any = out32 || base || var || delta || zstat, all = out32 && base && var && delta && zstat;
    NNGP_REQUIRE(any == all, "i8s_residual: the fused outputs (out32, base, var, delta, zstat) come all or none");
    NNGP_REQUIRE(!all || cin != nullptr, "i8s_residual: the fused outputs need cin");
    NNGP_REQUIRE(all || (floor_rows == nullptr && floor_z == nullptr), "i8s_residual: the floor ratios need the fused outputs");
    I8Plan pl;
    NNGP_TRY(i8s_plan(ns_z, ns_k, cut, &pl));
    const int64_t kr = round_up(n, 256), zr = round_up(mp, 256), nchunk = i8s_chunks(n, &pl);
    const size_t kp_bytes = (size_t)(ns_k * kr * n), zp_bytes = (size_t)(ns_z * zr * n);
    const size_t part_bytes = (size_t)(nchunk * pl.ndiag * mp * n) * sizeof(int32_t);
    const size_t f64s = (size_t)(n + 2) + (size_t)mp + (size_t)(mp * i8s_col_blocks(n) * 4);
    NNGP_REQUIRE(part_bytes < (size_t)16 << 30, "i8s_residual: the test entry keeps all partial products (16 GB limit)");
    char* ws = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&ws), kp_bytes + zp_bytes + part_bytes + sizeof(double) * f64s + 64, s));
    I8sResidualWs w;
    w.kplanes = reinterpret_cast<int8_t*>(ws);
    w.zplanes = w.kplanes + kp_bytes;
    w.partial = reinterpret_cast<int32_t*>(ws + kp_bytes + zp_bytes);
    w.kscale = reinterpret_cast<double*>(ws + kp_bytes + zp_bytes + part_bytes);
    w.zscale = w.kscale + n + 2;
    w.rowpart = w.zscale + mp;
    w.counters = reinterpret_cast<int*>(w.rowpart + mp * i8s_col_blocks(n) * 4);
    int rc = 0;
    // rows up to the next multiple of 256 are read by the product (never stored): zero planes, as ensure_i8s leaves them
    if (hipMemsetAsync(ws, 0, kp_bytes + zp_bytes, s) != hipSuccess || hipMemsetAsync(w.counters, 0, 64, s) != hipSuccess) {
        nngp::set_error("i8s_residual: hipMemsetAsync failed");
        rc = -1;
    }
    if (rc == 0)
        rc = i8s_residual_on(w, pl, out, ldo, cin, ldcin, z, ldz, kmat, ldk, mp, n, alpha, beta, gamma, ns_z, ns_k, round_z != 0, sym != 0,
                             out32, base, var, delta, zstat, floor_rows, floor_z, s);
    (void)hipFreeAsync(ws, s);
    return rc;
}

int nngp_pool_select(const double* mean, int64_t m, int32_t ny, const double* var, int64_t count, int32_t biased, uint64_t seed,
                     int64_t* indices, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(mean != nullptr && var != nullptr && indices != nullptr && m > 0 && ny >= 1 && count >= 0 && count <= m,
                 "pool_select: bad arguments (m=%lld, count=%lld)", (long long)m, (long long)count);
    if (count == 0) return 0;
    double* key = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&key), sizeof(double) * (size_t)m, s));
    const int rc = launch_pool_select(mean, m, ny, var, count, biased != 0, seed, key, indices, s);
    NNGP_HIP_CHECK(hipFreeAsync(key, s));
    return rc;
}

int nngp_pool_select_greedy(const double* cov, int64_t m, int64_t ld, double noise, int64_t count, int64_t* indices, double* gains,
                            double* factor, int64_t ldf, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(cov != nullptr && indices != nullptr, "pool_select_greedy: NULL cov or indices");
    NNGP_REQUIRE(m >= 1 && count >= 0 && count <= m, "pool_select_greedy: need m >= 1 and 0 <= count <= m (m=%lld, count=%lld)",
                 (long long)m, (long long)count);
    NNGP_REQUIRE(ld >= m, "pool_select_greedy: ld < m (ld=%lld, m=%lld)", (long long)ld, (long long)m);
    NNGP_REQUIRE(factor == nullptr || ldf >= m, "pool_select_greedy: ldf < m (ldf=%lld, m=%lld)", (long long)ldf, (long long)m);
    NNGP_REQUIRE(noise >= 0.0 && noise <= 1.7976931348623157e308, "pool_select_greedy: noise must be finite and >= 0 (noise=%g)", noise);
    if (count == 0) return 0;
    // the two copies of d, and the factor rows when the caller keeps none
    const size_t own = (factor == nullptr) ? (size_t)count * (size_t)m : 0;
    double* ws = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&ws), sizeof(double) * ((size_t)2 * (size_t)m + own), s));
    const int rc = launch_pool_greedy(cov, m, ld, noise, count, indices, gains, own ? ws + 2 * m : factor, own ? m : ldf, ws, s);
    NNGP_HIP_CHECK(hipFreeAsync(ws, s));
    return rc;
}

int nngp_syrk_tn_f64(double* c, int64_t ldc, double* r, const double* a, int64_t lda, const double* y, int64_t rows, int64_t mp,
                     int32_t ny, double beta, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_TRY(syrk_check(c, ldc, r, a, lda, y, rows, mp, ny, beta));
    double* ws = nullptr;
    const int64_t ws_doubles = syrk_ws_doubles(rows, mp);
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&ws), sizeof(double) * (size_t)ws_doubles, s));
    const int rc = launch_syrk_tn_f64(c, ldc, r, a, lda, y, rows, mp, ny, beta, ws, ws_doubles, s);
    NNGP_HIP_CHECK(hipFreeAsync(ws, s));
    return rc;
}

int nngp_symv_f64(const double* a, int64_t lda, int64_t n, const double* x, double* y, double diag_add, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(a != nullptr && x != nullptr && y != nullptr && n > 0 && lda >= n, "symv_f64: bad arguments");
    const int64_t np = round_up(n, TB);
    double* part = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&part), sizeof(double) * (size_t)(np / TB) * np, s));
    const int rc = launch_symv_f64(a, lda, n, x, y, diag_add, part, np, s);
    NNGP_HIP_CHECK(hipFreeAsync(part, s));
    return rc;
}

int nngp_trsm_rlt_f32(float* b, int64_t ldb, int64_t m, const float* l, int64_t ldl, const float* dinv, int64_t n,
                      void* stream) {
    NNGP_REQUIRE(b != nullptr && l != nullptr && dinv != nullptr, "trsm_rlt_f32: NULL argument");
    NNGP_REQUIRE(m % TB == 0 && n % TB == 0 && m > 0 && n > 0, "trsm_rlt_f32: m, n must be multiples of %d", TB);
    return trsm_rlt_f32(b, ldb, m, l, ldl, dinv, n, (hipStream_t)stream);
}

}  // extern "C"
