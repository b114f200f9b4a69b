// The float64 exact-GP core of the RBF GP (rbf_gp.hip) and the NNGP marginal likelihood (nngp_mll.hip): the blocked Cholesky and
// triangular solves (gp_f64.hip, also behind nngp_potrf_f64 and the three core operators of api_ops.hip), the evidence workspace both models hold with the
// evaluation sequence they share, and the device helpers of their lower-tile passes and fixed-order finish kernels.
#pragma once
#include "model.h"

namespace nngp {

// ---- float64 blocked Cholesky (n multiple of 128; dinv: n x 128; status: device int, -1 or the failed column) ----
int potrf_f64(double* a, int64_t n, int64_t ld, double* dinv, int* status, hipStream_t s);
int potrf_f64_status(const int* status, hipStream_t s, const char* who);  // syncs; rc < 0 naming the column if a pivot failed
// B^T (r rows of length np) <- B^T L^-T (tri: B^T is the identity); t: r x 128 scratch
int trsm_fwd_f64(double* bt, int64_t ldb, int64_t r, const double* l, int64_t ldl, const double* dinv, int64_t np, double* t,
                 bool tri, hipStream_t s);
// a [n, ld] <- the identity (grid: (n + 255) / 256 by n)
__global__ __launch_bounds__(256) void k_eye(double* a, int64_t ld, int64_t n);
// per row: dot[row] = dot_add + sum_k m[row, k] v[k];  sq[row] = sq_from - sum_k m[row, k]^2  (either may be NULL)
__global__ __launch_bounds__(256) void k_rowdot(const double* m, int64_t ld, int64_t cols, const double* v, double* dot,
                                               double dot_add, double* sq, double sq_from);

// ---- the evidence workspace: A = L L^T, w = L^-1 y and, for a gradient, A^-1 and alpha = A^-1 y (Np = n rounded up to 128) ----
constexpr int kGpTile = 64;  // edge of the lower tiles of the gradient passes: one vector of partials per tile

inline int64_t gp_lower_tiles(int64_t n) {
    const int64_t tn = (n + kGpTile - 1) / kGpTile;
    return tn * (tn + 1) / 2;
}

struct GpWorkspace {
    int64_t n_cap = 0, np_cap = 0, t_rows = 0;
    int d = 0;
    int64_t n = 0, np = 0;    // n = 0: no training data
    bool factored = false;
    double* x = nullptr;      // n_cap x d
    double* y = nullptr;      // np_cap, zero padded
    double* a = nullptr;      // np_cap^2: A, then its factor L (lower)
    double* zt = nullptr;     // np_cap^2: L^-T
    double* ainv = nullptr;   // np_cap^2: A^-1 = L^-T L^-1
    double* dinv = nullptr;   // np_cap x 128: inverted diagonal blocks
    double* wrow = nullptr;   // 128 x np_cap: row 0 = y, solved in place to w = L^-1 y; the other rows stay 0
    double* alpha = nullptr;  // np_cap
    double* part = nullptr;   // gradient partials, component-major: part[c * tiles + tile]
    double* red = nullptr;    // the finish kernel's sums
    int* status = nullptr;
    double* t = nullptr;      // t_rows x 128 solve scratch
};

// parts_per_tile partials for each of gp_lower_tiles(n_cap) tiles, red_len reduced sums, scratch_rows rows of solve scratch
int ws_alloc(GpWorkspace* w, int64_t n_cap, int d, int parts_per_tile, int64_t red_len, int64_t scratch_rows);
int ws_reserve_scratch(GpWorkspace* w, int64_t rows);  // grows t to at least rows x 128
void ws_free(GpWorkspace* w);
// x: device [n, d]; y: n values, device or host by y_kind, zero padded to Np; zeroes wrow and synchronises
int ws_set_train(GpWorkspace* w, const double* x, const double* y, hipMemcpyKind y_kind, int64_t n, hipStream_t s);
// L = chol(A) in place (A filled by the caller), w = L^-1 y; kGpSolveInverse (what `true` converts to): also L^-T, A^-1 and
// alpha; kGpSolveRows: L^-T and alpha without the A^-1 product.  neg_rowsq [Np]: minus the row sums of squares of L^-T, that is
// -[A^-1]_ii, from the pass that forms alpha (alpha's bits do not depend on it).  who prefixes the error.
enum { kGpSolveW = 0, kGpSolveInverse = 1, kGpSolveRows = 2 };
int factor_and_solve(GpWorkspace* w, int mode, const char* who, hipStream_t s, double* neg_rowsq = nullptr);

// Workgroup b runs on XCD b % 8: deal each XCD a contiguous range of the tile order, so that neighbouring tiles (which share
// row panels of X) meet in one L2 -- the ordering of gemm_f64.hip / kernel_build.hip.
__device__ __forceinline__ int64_t xcd_tile(int64_t b, int64_t total) {
    const int64_t q = total >> 3, r = total & 7, x = b & 7, slot = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + slot;
}

// lower tile t (row-major over the lower triangle) -> (ti, tj), tj <= ti
__device__ __forceinline__ void lower_tile(int64_t t, int64_t* ti, int64_t* tj) {
    int64_t i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    *ti = i;
    *tj = t - i * (i + 1) / 2;
}

// fixed-order block sum of 256 values (thread 0 holds the result)
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// The shared part of the finish kernels (one workgroup, fixed order): s[0] = sum log L_ii, s[1] = |w|^2 (= y^T A^-1 y) and, with
// alpha, s[2] = alpha^T alpha, s[3] = tr A^-1 (else 0)
__device__ __forceinline__ void finish_sums(const double* l, int64_t ldl, int64_t n, const double* w, const double* alpha,
                                            const double* ainv, double* red, double s[4]) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        v[0] += log(l[i * ldl + i]);
        v[1] += w[i] * w[i];
        if (alpha) {
            v[2] += alpha[i] * alpha[i];
            v[3] += ainv[i * ldl + i];
        }
    }
    s[0] = block_sum(v[0], red);
    s[1] = block_sum(v[1], red);
    s[2] = alpha ? block_sum(v[2], red) : 0.0;
    s[3] = alpha ? block_sum(v[3], red) : 0.0;
}

// component c of the gradient partials summed over the nparts tiles, in a fixed order
__device__ __forceinline__ double finish_part(const double* part, int64_t nparts, int c, double* red) {
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nparts; b += 256) s += part[(int64_t)c * nparts + b];
    return block_sum(s, red);
}

}  // namespace nngp
