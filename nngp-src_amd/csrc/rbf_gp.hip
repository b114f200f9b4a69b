// float64 RBF Gaussian process with marginal-likelihood training (reference train.py:60-150, GP_train_and_test).
//
// Everything here is float64, like the reference (train.py:24): the kernel matrix A = amp K + (noise + 1e-6) I, its
// Cholesky factor, log det A = 2 sum log L_ii, alpha = A^-1 y and A^-1 itself for the gradient's trace terms.  The factor,
// the solves and A^-1 are the float64 core of gp_f64.h, shared with the NNGP marginal likelihood; the NNGP model is untouched.
//
//   k_rbf_tile        K(i, j) = exp(-sum_k (x1_ik / ls - x2_jk / ls)^2) on 64 x 64 tiles, the differences formed directly
//                     (no Gram identity: raw forest rows have |x|^2 ~ 2e7 and the identity would cancel to ~1e-9)
//   k_gp_grad_partial one pass over the lower triangle of A^-1 with K recomputed: the four trace / quadratic-form sums
//   k_gp_finish       fixed-order second stage of every reduction (no atomics: repeated evaluations are bit-identical)
#include "gp_f64.h"

#include <vector>

namespace nngp {

namespace {

constexpr int RT = kGpTile;   // edge of the kernel-build and gradient tiles
constexpr int RKC = 32;       // feature chunk staged in LDS
constexpr int RLD = RKC + 1;  // LDS row stride (odd: the 16 rows a wave reads sit in different banks)
constexpr int NB = TB;        // padding of the test rows (the Cholesky's block)
constexpr int NPART = 4;      // partial sums per gradient workgroup

// Squared distances of the scaled rows for the 16 entries of this thread: rows i0 + tr + 16 p, columns j0 + tc + 16 q.
// The features are summed in order k = 0 .. d-1 (as a plain reduction over the last axis does).
__device__ __forceinline__ void tile_sqdist(const double* x1, int64_t n1, const double* x2, int64_t n2, int d, double ls,
                                            int64_t i0, int64_t j0, double (*s1)[RLD], double (*s2)[RLD], double acc[4][4]) {
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    for (int k0 = 0; k0 < d; k0 += RKC) {
        const int kc = d - k0 < RKC ? d - k0 : RKC;
        for (int e = tid; e < RT * RKC; e += 256) {
            const int r = e / RKC, k = e % RKC;
            const int64_t i = i0 + r, j = j0 + r;
            s1[r][k] = (k < kc && i < n1) ? x1[i * d + k0 + k] / ls : 0.0;
            s2[r][k] = (k < kc && j < n2) ? x2[j * d + k0 + k] / ls : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) a[p] = s1[tr + 16 * p][k];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = s2[tc + 16 * q][k];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double t = a[p] - b[q];
                    acc[p][q] += t * t;
                }
        }
        __syncthreads();
    }
}

struct RbfArgs {
    const double* x1;
    const double* x2;
    int64_t n1, n2;
    int d;
    double ls, amp, diag_add;
    int sym;              // x2 == x1: lower tiles only, mirrored; the diagonal gets amp + diag_add, the padding 1 on its diagonal
    double* out;
    int64_t ld, rows, cols;  // output extent (>= n1, n2); padded entries are 0 (sym: 1 on the diagonal)
    const double* sub;       // optional: out = value - sub[i, j]
    int64_t ld_sub;
    int64_t tiles_c;         // column tiles (non-symmetric grids)
};

__global__ __launch_bounds__(256) void k_rbf_tile(RbfArgs a) {
    __shared__ double s1[RT][RLD], s2[RT][RLD];
    const int64_t tiles_r = (a.rows + RT - 1) / RT;
    const int64_t total = a.sym ? tiles_r * (tiles_r + 1) / 2 : tiles_r * a.tiles_c;
    const int64_t t = xcd_tile(blockIdx.x, total);
    int64_t ti, tj;
    if (a.sym) {
        lower_tile(t, &ti, &tj);
    } else {
        ti = t / a.tiles_c;
        tj = t % a.tiles_c;
    }
    const int64_t i0 = ti * RT, j0 = tj * RT;
    double acc[4][4];
    tile_sqdist(a.x1, a.n1, a.x2, a.n2, a.d, a.ls, i0, j0, s1, s2, acc);
    const int tc = threadIdx.x & 15, tr = threadIdx.x >> 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + tr + 16 * p, j = j0 + tc + 16 * q;
            if (i >= a.rows || j >= a.cols) continue;
            double v;
            if (i < a.n1 && j < a.n2) {
                v = a.amp * exp(-acc[p][q]);
                if (a.sym && i == j) v += a.diag_add;
            } else {
                v = (a.sym && i == j) ? 1.0 : 0.0;
            }
            if (a.sub) v -= a.sub[i * a.ld_sub + j];
            a.out[i * a.ld + j] = v;
            if (a.sym && ti != tj) a.out[j * a.ld + i] = v;
        }
}

int launch_rbf(RbfArgs a, hipStream_t s) {
    NNGP_REQUIRE(a.d >= 1 && a.d <= 1024 && a.rows >= a.n1 && a.cols >= a.n2 && a.ld >= a.cols && a.ls > 0.0,
                 "rbf_gp: bad kernel-build arguments (d=%d)", a.d);
    if (a.rows <= 0 || a.cols <= 0) return 0;
    const int64_t tr = (a.rows + RT - 1) / RT;
    a.tiles_c = (a.cols + RT - 1) / RT;
    const int64_t total = a.sym ? tr * (tr + 1) / 2 : tr * a.tiles_c;
    NNGP_REQUIRE(total < 2147483647LL, "rbf_gp: kernel build grid too large");
    hipLaunchKernelGGL(k_rbf_tile, dim3((unsigned)total), dim3(256), 0, s, a);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

// One lower tile of the n x n training matrix: with K and the scaled squared distance d2 recomputed,
//   part[0] = sum alpha_i alpha_j K_ij,  part[1] = sum Ainv_ij K_ij,  part[2] = sum alpha_i alpha_j K_ij d2_ij,  part[3] = sum Ainv_ij K_ij d2_ij
// over the whole square (off-diagonal entries of the lower triangle count twice).
__global__ __launch_bounds__(256) void k_gp_grad_partial(const double* x, int64_t n, int d, double ls, const double* ainv, int64_t ld,
                                                         const double* alpha, double* part) {
    __shared__ double s1[RT][RLD], s2[RT][RLD];
    __shared__ double red[256];
    const int64_t tn = (n + RT - 1) / RT;
    const int64_t t = xcd_tile(blockIdx.x, tn * (tn + 1) / 2);
    int64_t ti, tj;
    lower_tile(t, &ti, &tj);
    const int64_t i0 = ti * RT, j0 = tj * RT;
    double acc[4][4];
    tile_sqdist(x, n, x, n, d, ls, i0, j0, s1, s2, acc);
    const int tc = threadIdx.x & 15, tr = threadIdx.x >> 4;
    double v[NPART] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + tr + 16 * p, j = j0 + tc + 16 * q;
            if (i >= n || j > i) continue;
            const double w = i == j ? 1.0 : 2.0;
            const double k = exp(-acc[p][q]);
            const double aa = w * (alpha[i] * alpha[j]) * k, ai = w * ainv[i * ld + j] * k;
            v[0] += aa;
            v[1] += ai;
            v[2] += aa * acc[p][q];
            v[3] += ai * acc[p][q];
        }
#pragma unroll
    for (int c = 0; c < NPART; ++c) {
        const double r = block_sum(v[c], red);
        if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = r;  // component-major (finish_part)
    }
}

// Second stage, one workgroup, fixed order:  out[0] = sum log L_ii,  out[1] = |w|^2 (w = L^-1 y, so y^T A^-1 y),
// out[2..5] = the gradient partials summed,  out[6] = alpha^T alpha,  out[7] = tr A^-1   (the last six only with grad)
__global__ __launch_bounds__(256) void k_gp_finish(const double* l, int64_t ldl, int64_t n, const double* w, const double* part,
                                                   int64_t nparts, const double* alpha, const double* ainv, double* out) {
    __shared__ double red[256];
    double s[4];
    finish_sums(l, ldl, n, w, alpha, ainv, red, s);
    if (threadIdx.x == 0) {
        out[0] = s[0];
        out[1] = s[1];
        out[6] = s[2];
        out[7] = s[3];
    }
    if (!part) return;
    for (int c = 0; c < NPART; ++c) {
        const double r = finish_part(part, nparts, c, red);
        if (threadIdx.x == 0) out[2 + c] = r;
    }
}

}  // namespace

}  // namespace nngp

// ---------------------------------------------------------------------------------------------------------------------------
// C ABI (include/nngp_hip.h, "RBF Gaussian process")

struct nngp_rbf_gp {
    GpWorkspace w;            // y: y - mean(y); t: max(np_cap, mp_cap) rows
    int64_t m_cap = 0, mp_cap = 0;
    double ymean = 0.0;
    bool have_terms = false;
    double amp = 0, noise = 0, ls = 0;
    double terms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double* cross = nullptr;  // mp_cap x np_cap: amp K(X_t, X), solved in place to V^T
    double* covtmp = nullptr; // mp_cap^2: V^T V
};

namespace {

void gp_free_test(nngp_rbf_gp* g) {
    dev_free(g->cross);
    dev_free(g->covtmp);
}

int gp_alloc_test(nngp_rbf_gp* g, int64_t m_cap) {
    gp_free_test(g);
    g->m_cap = m_cap;
    g->mp_cap = round_up(m_cap > 0 ? m_cap : 1, NB);
    NNGP_TRY(dev_alloc(&g->cross, g->mp_cap * g->w.np_cap));
    NNGP_TRY(dev_alloc(&g->covtmp, g->mp_cap * g->mp_cap));
    return ws_reserve_scratch(&g->w, g->mp_cap > g->w.np_cap ? g->mp_cap : g->w.np_cap);
}

void gp_free(nngp_rbf_gp* g) {
    gp_free_test(g);
    ws_free(&g->w);
}

double softplus(double x) { return x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x)); }  // logaddexp(x, 0)
double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

}  // namespace

extern "C" {

int nngp_rbf_gp_create(nngp_rbf_gp** out, int64_t n_cap, int64_t m_cap, int32_t d) {
    NNGP_REQUIRE(out != nullptr && n_cap > 0 && m_cap >= 0 && d >= 1 && d <= 1024, "rbf_gp_create: bad arguments (n_cap=%lld, d=%d)",
                 (long long)n_cap, d);
    *out = nullptr;
    nngp_rbf_gp* g = new (std::nothrow) nngp_rbf_gp();
    NNGP_REQUIRE(g != nullptr, "rbf_gp_create: out of host memory");
    int rc = ws_alloc(&g->w, n_cap, d, NPART, 8, round_up(n_cap > m_cap ? n_cap : m_cap, NB));  // scratch for predict too
    if (rc == 0) rc = gp_alloc_test(g, m_cap);
    if (rc != 0) {
        gp_free(g);
        delete g;
        return rc;
    }
    *out = g;
    return 0;
}

int nngp_rbf_gp_destroy(nngp_rbf_gp* g) {
    if (g == nullptr) return 0;
    (void)hipDeviceSynchronize();
    gp_free(g);
    delete g;
    return 0;
}

int nngp_rbf_gp_set_train(nngp_rbf_gp* g, const double* x, const double* y, int64_t n, int32_t ny, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(g != nullptr && x != nullptr && y != nullptr, "rbf_gp_set_train: NULL argument");
    NNGP_REQUIRE(ny == 1, "rbf_gp_set_train: the GP takes one output column (ny=%d)", ny);
    NNGP_REQUIRE(n >= 1 && n <= g->w.n_cap, "rbf_gp_set_train: n=%lld outside [1, n_cap=%lld]", (long long)n, (long long)g->w.n_cap);
    g->have_terms = false;
    std::vector<double> h((size_t)n);
    NNGP_HIP_CHECK(hipMemcpyAsync(h.data(), y, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) sum += h[i];
    const double mean = sum / (double)n;
    for (int64_t i = 0; i < n; ++i) h[i] -= mean;
    g->ymean = mean;
    return ws_set_train(&g->w, x, h.data(), hipMemcpyHostToDevice, n, s);
}

int nngp_rbf_gp_evaluate(nngp_rbf_gp* g, const double* raw, double* nlml, double* grad_raw, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(g != nullptr && raw != nullptr && nlml != nullptr, "rbf_gp_evaluate: NULL argument");
    NNGP_REQUIRE(g->w.n > 0, "rbf_gp_evaluate: no training data (nngp_rbf_gp_set_train)");
    NNGP_REQUIRE(std::isfinite(raw[0]) && std::isfinite(raw[1]) && std::isfinite(raw[2]),
                 "rbf_gp_evaluate: non-finite hyperparameter (raw = %g, %g, %g)", raw[0], raw[1], raw[2]);
    const double amp = softplus(raw[0]), noise = softplus(raw[1]), ls = softplus(raw[2]);
    NNGP_REQUIRE(amp > 0.0 && ls > 0.0, "rbf_gp_evaluate: amplitude and length scale must be positive (raw = %g, %g, %g)", raw[0],
                 raw[1], raw[2]);
    GpWorkspace& w = g->w;
    w.factored = g->have_terms = false;
    const int64_t n = w.n, np = w.np;
    RbfArgs ra{};
    ra.x1 = ra.x2 = w.x;
    ra.n1 = ra.n2 = n;
    ra.d = w.d;
    ra.ls = ls;
    ra.amp = amp;
    ra.diag_add = noise + 1e-6;
    ra.sym = 1;
    ra.out = w.a;
    ra.ld = ra.rows = ra.cols = np;
    NNGP_TRY(launch_rbf(ra, s));
    const bool grad = grad_raw != nullptr;
    NNGP_TRY(factor_and_solve(&w, grad, "rbf_gp_evaluate", s));
    g->amp = amp;
    g->noise = noise;
    g->ls = ls;
    const int64_t nparts = gp_lower_tiles(n);
    if (grad) {
        hipLaunchKernelGGL(k_gp_grad_partial, dim3((unsigned)nparts), dim3(256), 0, s, w.x, n, w.d, ls, w.ainv, np, w.alpha, w.part);
        NNGP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_gp_finish, dim3(1), dim3(256), 0, s, w.a, np, n, w.wrow, grad ? w.part : nullptr, nparts,
                       grad ? w.alpha : nullptr, w.ainv, w.red);
    NNGP_HIP_CHECK(hipGetLastError());
    double r[8];
    NNGP_HIP_CHECK(hipMemcpyAsync(r, w.red, sizeof(r), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    const double c = log(2.0 * 3.1415);
    const double la = log(amp);
    *nlml = 0.5 * r[1] + r[0] + ((double)n / 2.0) * c - 0.5 * c - la * la;
    if (grad) {
        const double g_amp = -0.5 * r[2] + 0.5 * r[3] - 2.0 * la / amp;
        const double g_noise = -0.5 * r[6] + 0.5 * r[7];
        const double g_ls = amp * (2.0 / ls) * (-0.5 * r[4] + 0.5 * r[5]);
        grad_raw[0] = g_amp * sigmoid(raw[0]);
        grad_raw[1] = g_noise * sigmoid(raw[1]);
        grad_raw[2] = g_ls * sigmoid(raw[2]);
        for (int i = 0; i < 8; ++i) g->terms[i] = r[i];
        g->have_terms = true;
    }
    w.factored = true;
    return 0;
}

int nngp_rbf_gp_terms(const nngp_rbf_gp* g, double* out) {
    NNGP_REQUIRE(g != nullptr && out != nullptr, "rbf_gp_terms: NULL argument");
    NNGP_REQUIRE(g->have_terms, "rbf_gp_terms: no gradient evaluation yet");
    for (int i = 0; i < 8; ++i) out[i] = g->terms[i];
    return 0;
}

int nngp_rbf_gp_predict(nngp_rbf_gp* g, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var_or_cov,
                        void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(g != nullptr && x_test != nullptr && mean != nullptr && mt >= 1, "rbf_gp_predict: bad arguments");
    NNGP_REQUIRE(cov_mode == NNGP_COV_NONE || cov_mode == NNGP_COV_DIAG || cov_mode == NNGP_COV_FULL, "rbf_gp_predict: bad cov_mode %d",
                 cov_mode);
    NNGP_REQUIRE(cov_mode == NNGP_COV_NONE || var_or_cov != nullptr, "rbf_gp_predict: NULL covariance output");
    NNGP_REQUIRE(g->w.factored, "rbf_gp_predict: no successful nngp_rbf_gp_evaluate since the training data was set");
    if (mt > g->m_cap) {  // the only allocation after create
        NNGP_HIP_CHECK(hipStreamSynchronize(s));
        NNGP_TRY(gp_alloc_test(g, mt));
    }
    const int64_t np = g->w.np, mp = round_up(mt, NB);
    RbfArgs ra{};
    ra.x1 = x_test;
    ra.x2 = g->w.x;
    ra.n1 = mt;
    ra.n2 = g->w.n;
    ra.d = g->w.d;
    ra.ls = g->ls;
    ra.amp = g->amp;
    ra.out = g->cross;
    ra.ld = np;
    ra.rows = mp;
    ra.cols = np;
    NNGP_TRY(launch_rbf(ra, s));
    NNGP_TRY(trsm_fwd_f64(g->cross, np, mp, g->w.a, np, g->w.dinv, np, g->w.t, false, s));  // V^T = amp K(X_t, X) L^-T
    // mean = V^T w + mean(y)  (= amp K(X_t, X) alpha + mean(y));  var = amp - |V^T row|^2
    hipLaunchKernelGGL(k_rowdot, dim3((unsigned)mt), dim3(256), 0, s, g->cross, np, np, g->w.wrow, mean, g->ymean,
                       cov_mode == NNGP_COV_DIAG ? var_or_cov : nullptr, g->amp);
    NNGP_HIP_CHECK(hipGetLastError());
    if (cov_mode == NNGP_COV_FULL) {
        NNGP_TRY(launch_gemm_nt_f64(g->covtmp, mp, nullptr, 0, g->cross, np, g->cross, np, mp, mp, np, 1.0, 0.0, s));
        RbfArgs rc{};
        rc.x1 = rc.x2 = x_test;
        rc.n1 = rc.n2 = mt;
        rc.d = g->w.d;
        rc.ls = g->ls;
        rc.amp = g->amp;
        rc.out = var_or_cov;
        rc.ld = rc.rows = rc.cols = mt;
        rc.sub = g->covtmp;
        rc.ld_sub = mp;
        NNGP_TRY(launch_rbf(rc, s));
    }
    return 0;
}

int nngp_rbf_gp_kernel(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d, double ls, double* out, int64_t ld,
                       void* stream) {
    NNGP_REQUIRE(x1 != nullptr && out != nullptr && n1 >= 1 && (x2 == nullptr || n2 >= 1) && ld >= (x2 ? n2 : n1) &&
                     std::isfinite(ls) && ls > 0.0,
                 "rbf_gp_kernel: bad arguments");
    RbfArgs ra{};
    ra.x1 = x1;
    ra.x2 = x2 ? x2 : x1;
    ra.n1 = ra.rows = n1;
    ra.n2 = ra.cols = x2 ? n2 : n1;
    ra.d = d;
    ra.ls = ls;
    ra.amp = 1.0;
    ra.out = out;
    ra.ld = ld;
    return launch_rbf(ra, (hipStream_t)stream);
}

int nngp_rbf_gp_factor_buffer(const nngp_rbf_gp* g, double** l, int64_t* ld, int64_t* n_padded) {
    NNGP_REQUIRE(g != nullptr && l != nullptr && ld != nullptr, "rbf_gp_factor_buffer: NULL argument");
    NNGP_REQUIRE(g->w.factored, "rbf_gp_factor_buffer: no factor (nngp_rbf_gp_evaluate)");
    *l = g->w.a;
    *ld = g->w.np;
    if (n_padded) *n_padded = g->w.np;
    return 0;
}

}  // extern "C"
