// The float64 exact-GP core (gp_f64.h): blocked Cholesky, triangular solves, and the evaluation sequence of the RBF GP and the NNGP
// marginal likelihood.  Everything is float64: the NNGP path's float32 factor cannot give log det A or tr(A^-1 dA) to that grade
// (DESIGN.md section 9).
//
//   k_chol_diag       factors one 128 x 128 diagonal block in LDS and writes the block's inverse
//   potrf_f64         blocked right-looking Cholesky: k_chol_diag, then the panel L21 = A21 L11^-T and the trailing update
//                     A22 -= L21 L21^T on the float64 MFMA GEMM (gemm_f64.hip)
//   trsm_fwd_f64      B^T <- B^T L^-T (each row b of B^T becomes L^-1 b), left-looking by 128-column blocks, two GEMMs per block
//   factor_and_solve  potrf_f64, w = L^-1 y and, for a gradient, L^-T (trsm_fwd_f64 on the identity), A^-1 = L^-T L^-1 and alpha;
//                     kGpSolveRows stops short of the A^-1 product (the leave-one-out values need only the rows of L^-T)
#include "gp_f64.h"

namespace nngp {

namespace {

constexpr int NB = TB;  // diagonal block of the Cholesky (the GEMM's tile edge)
constexpr int SLD = NB + 1;

// One 128 x 128 diagonal block: L11 = chol(A11) in place (zeros above the diagonal) and dinv = L11^-1 (lower).  A pivot that is
// not positive (or not finite) stops the factorisation: status <- its global column, and every later block returns at once.
__global__ __launch_bounds__(256) void k_chol_diag(double* a, int64_t ld, int64_t kb, double* dinv, int* status) {
    extern __shared__ __attribute__((aligned(16))) double S[];  // NB x SLD, then NB inverted pivots
    double* invd = S + NB * SLD;
    if (*status >= 0) return;
    const int tid = threadIdx.x;
    double* a0 = a + kb * NB * ld + kb * NB;
    for (int e = tid; e < NB * NB; e += 256) S[(e / NB) * SLD + e % NB] = a0[(int64_t)(e / NB) * ld + e % NB];
    __syncthreads();
    for (int j = 0; j < NB; ++j) {
        const double p = S[j * SLD + j];
        if (!(p > 0.0) || !isfinite(p)) {  // uniform: every thread read the same LDS word
            if (tid == 0) *status = (int)(kb * NB + j);
            return;
        }
        const double ljj = sqrt(p);
        __syncthreads();
        if (tid == 0) S[j * SLD + j] = ljj;
        for (int i = j + 1 + tid; i < NB; i += 256) S[i * SLD + j] = S[i * SLD + j] / ljj;
        __syncthreads();
        for (int i = j + 1 + (tid >> 5); i < NB; i += 8) {  // trailing lower triangle: 8 rows x 32 columns per pass
            const double lij = S[i * SLD + j];
            for (int k = j + 1 + (tid & 31); k <= i; k += 32) S[i * SLD + k] -= lij * S[k * SLD + j];
        }
        __syncthreads();
    }
    // L11^-1 by forward substitution, one column per thread: X(i, c) for i > c goes to S(c, i) (the free upper triangle)
    if (tid < NB) {
        const int c = tid;
        const double dc = 1.0 / S[c * SLD + c];
        invd[c] = dc;
        for (int i = c + 1; i < NB; ++i) {
            double sum = S[i * SLD + c] * dc;
            for (int k = c + 1; k < i; ++k) sum += S[i * SLD + k] * S[c * SLD + k];
            S[c * SLD + i] = -sum / S[i * SLD + i];
        }
    }
    __syncthreads();
    double* di = dinv + kb * NB * NB;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        a0[(int64_t)r * ld + c] = c <= r ? S[r * SLD + c] : 0.0;
        di[e] = r > c ? S[c * SLD + r] : (r == c ? invd[r] : 0.0);
    }
}

constexpr size_t kDiagLds = sizeof(double) * (NB * SLD + NB);

}  // namespace

// B^T (r rows of length np) <- B^T L^-T.  tri: B^T is the identity, so the result (L^-T) is upper triangular and block step kb only
// touches rows < (kb + 1) NB.  t: r x NB scratch.
int trsm_fwd_f64(double* bt, int64_t ldb, int64_t r, const double* l, int64_t ldl, const double* dinv, int64_t np, double* t,
                 bool tri, hipStream_t s) {
    for (int64_t kb = 0; kb * NB < np; ++kb) {
        const int64_t m = tri ? (kb + 1) * NB : r;
        double* col = bt + kb * NB;
        const double* di = dinv + kb * NB * NB;
        if (kb == 0) {  // in place: each output row tile is read (k = 128) only by the workgroup that writes it
            NNGP_TRY(launch_gemm_nt_f64(col, ldb, nullptr, 0, col, ldb, di, NB, m, NB, NB, 1.0, 0.0, s));
        } else {
            NNGP_TRY(launch_gemm_nt_f64(t, NB, col, ldb, bt, ldb, l + kb * NB * ldl, ldl, m, NB, kb * NB, -1.0, 1.0, s));
            NNGP_TRY(launch_gemm_nt_f64(col, ldb, nullptr, 0, t, NB, di, NB, m, NB, NB, 1.0, 0.0, s));
        }
    }
    return 0;
}

__global__ __launch_bounds__(256) void k_eye(double* a, int64_t ld, int64_t n) {
    const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) a[i * ld + j] = i == j ? 1.0 : 0.0;
}

// per row: dot[row] = dot_add + sum_k m[row, k] v[k];  sq[row] = sq_from - sum_k m[row, k]^2  (either may be NULL)
__global__ __launch_bounds__(256) void k_rowdot(const double* m, int64_t ld, int64_t cols, const double* v, double* dot,
                                               double dot_add, double* sq, double sq_from) {
    __shared__ double red[256];
    const double* row = m + (int64_t)blockIdx.x * ld;
    double a = 0.0, b = 0.0;
    for (int64_t k = threadIdx.x; k < cols; k += 256) {
        const double x = row[k];
        if (dot) a += x * v[k];
        b += x * x;
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        if (dot) dot[blockIdx.x] = dot_add + a;
        if (sq) sq[blockIdx.x] = sq_from - b;
    }
}

int potrf_f64(double* a, int64_t n, int64_t ld, double* dinv, int* status, hipStream_t s) {
    NNGP_REQUIRE(a != nullptr && dinv != nullptr && status != nullptr, "potrf_f64: NULL argument");
    NNGP_REQUIRE(n > 0 && n % NB == 0 && ld >= n && ld % 2 == 0 && ((uintptr_t)a & 15) == 0,
                 "potrf_f64: n must be a positive multiple of %d and ld >= n even (n=%lld ld=%lld)", NB, (long long)n, (long long)ld);
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chol_diag), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDiagLds);
    });
    NNGP_HIP_CHECK(attr);
    NNGP_HIP_CHECK(hipMemsetAsync(status, 0xff, sizeof(int), s));  // -1: no failed pivot
    for (int64_t kb = 0; kb * NB < n; ++kb) {
        hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), kDiagLds, s, a, ld, kb, dinv, status);
        NNGP_HIP_CHECK(hipGetLastError());
        const int64_t rem = n - (kb + 1) * NB;
        if (rem == 0) break;
        double* a21 = a + (kb + 1) * NB * ld + kb * NB;
        // panel in place: one column tile, so each row tile of A21 is read only by the workgroup that overwrites it
        NNGP_TRY(launch_gemm_nt_f64(a21, ld, nullptr, 0, a21, ld, dinv + kb * NB * NB, NB, rem, NB, NB, 1.0, 0.0, s));
        double* a22 = a21 + NB;
        NNGP_TRY(launch_gemm_nt_f64(a22, ld, a22, ld, a21, ld, a21, ld, rem, rem, NB, -1.0, 1.0, s));
    }
    return 0;
}

int potrf_f64_status(const int* status, hipStream_t s, const char* who) {
    int st = -1;
    NNGP_HIP_CHECK(hipMemcpyAsync(&st, status, sizeof(int), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    NNGP_REQUIRE(st < 0, "%s: the matrix is not positive definite: the pivot of column %d is not positive", who, st);
    return 0;
}

int ws_alloc(GpWorkspace* w, int64_t n_cap, int d, int parts_per_tile, int64_t red_len, int64_t scratch_rows) {
    w->n_cap = n_cap;
    w->d = d;
    w->np_cap = round_up(n_cap, NB);
    const int64_t np = w->np_cap;
    NNGP_TRY(dev_alloc(&w->x, n_cap * d));
    NNGP_TRY(dev_alloc(&w->y, np));
    NNGP_TRY(dev_alloc(&w->a, np * np));
    NNGP_TRY(dev_alloc(&w->zt, np * np));
    NNGP_TRY(dev_alloc(&w->ainv, np * np));
    NNGP_TRY(dev_alloc(&w->dinv, np * NB));
    NNGP_TRY(dev_alloc(&w->wrow, NB * np));
    NNGP_TRY(dev_alloc(&w->alpha, np));
    NNGP_TRY(dev_alloc(&w->part, parts_per_tile * gp_lower_tiles(n_cap)));
    NNGP_TRY(dev_alloc(&w->red, red_len));
    NNGP_TRY(dev_alloc(&w->status, 1));
    return ws_reserve_scratch(w, scratch_rows);
}

int ws_reserve_scratch(GpWorkspace* w, int64_t rows) {
    if (rows <= w->t_rows) return 0;
    dev_free(w->t);
    w->t_rows = 0;
    NNGP_TRY(dev_alloc(&w->t, rows * NB));
    w->t_rows = rows;
    return 0;
}

void ws_free(GpWorkspace* w) {
    for (double** p : {&w->x, &w->y, &w->a, &w->zt, &w->ainv, &w->dinv, &w->wrow, &w->alpha, &w->part, &w->red, &w->t}) dev_free(*p);
    dev_free(w->status);
}

int ws_set_train(GpWorkspace* w, const double* x, const double* y, hipMemcpyKind y_kind, int64_t n, hipStream_t s) {
    w->n = w->np = 0;
    w->factored = false;
    const int64_t np = round_up(n, NB);
    NNGP_HIP_CHECK(hipMemcpyAsync(w->x, x, sizeof(double) * n * w->d, hipMemcpyDeviceToDevice, s));
    NNGP_HIP_CHECK(hipMemsetAsync(w->y, 0, sizeof(double) * np, s));
    NNGP_HIP_CHECK(hipMemcpyAsync(w->y, y, sizeof(double) * n, y_kind, s));
    NNGP_HIP_CHECK(hipMemsetAsync(w->wrow, 0, sizeof(double) * NB * np, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));  // a host y may leave scope
    w->n = n;
    w->np = np;
    return 0;
}

int factor_and_solve(GpWorkspace* w, int mode, const char* who, hipStream_t s, double* neg_rowsq) {
    const int64_t np = w->np;
    NNGP_TRY(potrf_f64(w->a, np, np, w->dinv, w->status, s));
    NNGP_TRY(potrf_f64_status(w->status, s, who));
    NNGP_HIP_CHECK(hipMemcpyAsync(w->wrow, w->y, sizeof(double) * np, hipMemcpyDeviceToDevice, s));
    NNGP_TRY(trsm_fwd_f64(w->wrow, np, NB, w->a, np, w->dinv, np, w->t, false, s));
    if (mode == kGpSolveW) return 0;
    hipLaunchKernelGGL(k_eye, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, s, w->zt, np, np);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_TRY(trsm_fwd_f64(w->zt, np, np, w->a, np, w->dinv, np, w->t, true, s));
    if (mode == kGpSolveInverse) NNGP_TRY(launch_gemm_nt_f64(w->ainv, np, nullptr, 0, w->zt, np, w->zt, np, np, np, np, 1.0, 0.0, s));
    hipLaunchKernelGGL(k_rowdot, dim3((unsigned)np), dim3(256), 0, s, w->zt, np, np, w->wrow, w->alpha, 0.0, neg_rowsq, 0.0);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nngp
