// The matrix-free exact NNGP posterior (include/nngp_matfree.h): preconditioned CG on a block of right-hand sides, A = K + sigma2 I
// applied by the fused operator of kmv_f64.hip, P = sigma2 I + Vt Vt^T of the sparse model (sparse_gp.hip) inverted by Woodbury.
//
//   vectors     RHS-major [r, np]: each vector contiguous, np = n_cap rounded up to 128, the padding columns zero (the products with
//               Vt contract over them).  All products with Vt run on rp = rhs_cap rounded up to 128 rows whatever r is, so the
//               GEMMs' tiling and split never depend on r: a column's result does not depend on its neighbours.
//   P^-1        T^T = R VtT^T [rp, mp] (VtT: the transposed copy of Vt kept beside it, 2 n mp doubles in all -- gemm_f64.hip is an NT
//               product and this contraction runs over Vt's slow index; the copy costs memory, a skinny TN kernel would have cost a
//               second hot loop to write and pin), the forward solve with L_B (trsm_fwd_f64), the backward one as an NT product with
//               L_B^-T formed once per fit, then Z = (R - W^T Vt^T) / sigma2 in one NT product with R as its input term.
//   scalars     one workgroup per column and a fixed-order block sum for every dot product: rho, p^T A p, |r|^2 live on the device,
//               a frozen column (converged, or p^T A p not positive and finite) takes step 0.
//   stop rule   a host loop bounded by max_iter that reads the r residual norms and states back EVERY iteration (3 rp doubles; the
//               K pass beside it is at least tens of milliseconds at the sizes this model is for).
//   true residual  after the loop one more pass forms B - A X; columns above tol restart once from it; what is reported is the
//               recomputed residual.
#include "sparse_gp.h"
#include "kmv_f64.h"

#include <algorithm>
#include <cmath>
#include <new>

struct nngp_matfree {
    int64_t n_cap = 0, np = 0, m_cap = 0, mp_cap = 0, chunk_rows = 0, rhs_cap = 0, rp = 0;
    int d = 0, ny = 1;
    nngp::ArchDev arch{};
    double diag_reg = 0.0, jitter = 0.0;
    int absolute = 0;
    nngp_sparse* sp = nullptr;   // the preconditioner's model (m_cap > 0)
    nngp::GroupsDev groups{};    // additive handle (include/nngp_matfree_additive.h): the table arch.groups points to

    int64_t n = 0, m = 0, mp = 0;
    bool fitted = false;
    double sigma2 = 0.0;

    double* x = nullptr;      // [n_cap, d]
    double* q = nullptr;      // [n_cap] |x|^2 / d
    double* kd = nullptr;     // [max(n_cap, rp)] K(x, x) of the training rows (m = 0: the trace), then of a test block
    double* xq = nullptr;     // [rp] |x|^2 / d of a test block
    double* vt = nullptr;     // [np, mp]
    double* vtt = nullptr;    // [mp, np]
    double* lbit = nullptr;   // [mp, mp] L_B^-T
    double* tt = nullptr;     // [rp, mp] T^T, solved in place
    double* wt = nullptr;     // [rp, mp] W^T
    double* tscr = nullptr;   // [max(rp, mp_cap), 128] solve scratch
    double* r = nullptr;      // [rp, np] the solver's residuals, preconditioned residuals, directions and A p
    double* z = nullptr;
    double* p = nullptr;
    double* ap = nullptr;
    double* bt = nullptr;     // [rp, np] K(X_b, X) of a test block; the columns of y during a fit
    double* zt = nullptr;     // [rp, np] its solution
    double* alpha = nullptr;  // [16, np]
    double* ws = nullptr;     // the operator's split partials
    int64_t ws_doubles = 0;
    double* scal = nullptr;   // [4][rp]: rho, |b|^2, |r|^2, state (0 iterating, 1 converged, 2 broken down); then [1] the trace
    double* host = nullptr;   // pinned [3 rp + 1]

    int iterations = 0, k_passes = 0, restarts = 0, converged = 0;
    double rel_residual = 0.0;
};

namespace nngp {

namespace {

__global__ __launch_bounds__(256) void k_mf_transpose(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd,
                                                      int64_t rows, int64_t cols) {
    __shared__ double tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        tile[i][tx] = (r0 + i < rows && c0 + tx < cols) ? src[(r0 + i) * lds + c0 + tx] : 0.0;
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < cols && r0 + tx < rows) dst[(c0 + i) * ldd + r0 + tx] = tile[tx][i];
}

// out[0] = sum of v[0 .. n): one workgroup, fixed order
__global__ __launch_bounds__(256) void k_mf_sum(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += v[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// per column: x = 0, r = b, |b|^2; a zero right-hand side is solved already
__global__ __launch_bounds__(256) void k_mf_begin(const double* __restrict__ b, int64_t ldb, double* __restrict__ x, int64_t ldx,
                                                  double* __restrict__ r, int64_t ld, int64_t n, double* __restrict__ scal, int64_t rp,
                                                  double tol2) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double v = b[c * ldb + i];
        x[c * ldx + i] = 0.0;
        r[c * ld + i] = v;
        s += v * v;
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        scal[c] = 0.0;
        scal[rp + c] = s;
        scal[2 * rp + c] = s;
        scal[3 * rp + c] = (s <= tol2 * s) ? 1.0 : 0.0;
    }
}

// per iterating column: rho' = r . z, p = z + (rho' / rho) p (first: p = z)
__global__ __launch_bounds__(256) void k_mf_dir(const double* __restrict__ r, const double* __restrict__ z, double* __restrict__ p,
                                                int64_t ld, int64_t n, double* __restrict__ scal, int64_t rp, int first) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x;
    if (scal[3 * rp + c] != 0.0) return;
    const double rho_old = scal[c];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += r[c * ld + i] * z[c * ld + i];
    const double rho = block_sum(s, red);
    const double beta = first ? 0.0 : rho / rho_old;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double zi = z[c * ld + i];
        p[c * ld + i] = first ? zi : zi + beta * p[c * ld + i];
    }
    if (threadIdx.x == 0) scal[c] = rho;
}

// per iterating column: a = rho / p . Ap, x += a p, r -= a Ap, |r|^2 and the new state
__global__ __launch_bounds__(256) void k_mf_step(double* __restrict__ x, int64_t ldx, double* __restrict__ r, const double* __restrict__ p,
                                                 const double* __restrict__ ap, int64_t ld, int64_t n, double* __restrict__ scal,
                                                 int64_t rp, double tol2) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x;
    if (scal[3 * rp + c] != 0.0) return;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += p[c * ld + i] * ap[c * ld + i];
    const double pap = block_sum(s, red);
    if (!(pap > 0.0) || !isfinite(pap)) {  // the same value in every thread
        if (threadIdx.x == 0) scal[3 * rp + c] = 2.0;
        return;
    }
    const double a = scal[c] / pap;
    double rr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        x[c * ldx + i] += a * p[c * ld + i];
        const double ri = r[c * ld + i] - a * ap[c * ld + i];
        r[c * ld + i] = ri;
        rr += ri * ri;
    }
    rr = block_sum(rr, red);
    if (threadIdx.x == 0) {
        scal[2 * rp + c] = rr;
        scal[3 * rp + c] = (rr <= tol2 * scal[rp + c]) ? 1.0 : 0.0;
    }
}

// per column: r = b - A x (ax holds A x), |r|^2, and the state a restart would start from
__global__ __launch_bounds__(256) void k_mf_resid(const double* __restrict__ b, int64_t ldb, const double* __restrict__ ax,
                                                  double* __restrict__ r, int64_t ld, int64_t n, double* __restrict__ scal, int64_t rp,
                                                  double tol2) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x;
    double rr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double ri = b[c * ldb + i] - ax[c * ld + i];
        r[c * ld + i] = ri;
        rr += ri * ri;
    }
    rr = block_sum(rr, red);
    if (threadIdx.x == 0) {
        scal[2 * rp + c] = rr;
        scal[3 * rp + c] = (rr <= tol2 * scal[rp + c]) ? 1.0 : 0.0;
    }
}

// one workgroup per test row: mean[row, y] = B_row . alpha_y;  var[row] = kdiag[row] - B_row . Z_row
// resid (additive handles): the solver's true residual R = B - A Z.  B . Z + Z . R = 2 B . Z - Z . A Z is the quadratic form whose
// maximum over Z is B . A^-1 B: its error is second order in Z's, where B . Z alone keeps a first-order term Z . R that CG removes
// only in exact arithmetic (the Galerkin condition).  The additive kernel's preconditioned solves end after two dozen iterations at
// variances of 2e-4 .. 2e-3 of K(x, x), and there that term is what is left.
__global__ __launch_bounds__(256) void k_mf_predict_finish(const double* __restrict__ bt, const double* __restrict__ zt, int64_t ld,
                                                           int64_t n, const double* __restrict__ alpha, int ny,
                                                           const double* __restrict__ kdiag, double* __restrict__ mean,
                                                           double* __restrict__ var, const double* __restrict__ resid) {
    __shared__ double red[256];
    const int64_t row = blockIdx.x;
    const double* br = bt + row * ld;
    for (int y = 0; y < ny; ++y) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += 256) s += br[i] * alpha[(int64_t)y * ld + i];
        s = block_sum(s, red);
        if (threadIdx.x == 0) mean[row * ny + y] = s;
    }
    if (var == nullptr) return;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += br[i] * zt[row * ld + i];
    s = block_sum(s, red);
    if (resid != nullptr) {
        double c = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += 256) c += zt[row * ld + i] * resid[row * ld + i];
        s += block_sum(c, red);
    }
    if (threadIdx.x == 0) var[row] = kdiag[row] - s;
}

void mf_free(nngp_matfree* h) {
    for (double** p : {&h->x, &h->q, &h->kd, &h->xq, &h->vt, &h->vtt, &h->lbit, &h->tt, &h->wt, &h->tscr, &h->r, &h->z, &h->p, &h->ap,
                       &h->bt, &h->zt, &h->alpha, &h->ws, &h->scal})
        dev_free(*p);
    if (h->host) (void)hipHostFree(h->host);
    h->host = nullptr;
    if (h->sp) (void)nngp_sparse_destroy(h->sp);
    h->sp = nullptr;
    groups_destroy(&h->groups);
    h->arch.groups = nullptr;
}

int mf_alloc(nngp_matfree* h) {
    const int64_t np = h->np, rp = h->rp, mp = h->mp_cap;
    NNGP_TRY(dev_alloc(&h->x, h->n_cap * h->d));
    NNGP_TRY(dev_alloc(&h->q, h->n_cap));
    NNGP_TRY(dev_alloc(&h->kd, std::max(h->n_cap, rp)));
    NNGP_TRY(dev_alloc(&h->xq, rp));
    if (mp > 0) {
        NNGP_TRY(dev_alloc(&h->vt, np * mp));
        NNGP_TRY(dev_alloc(&h->vtt, mp * np));
        NNGP_TRY(dev_alloc(&h->lbit, mp * mp));
        NNGP_TRY(dev_alloc(&h->tt, rp * mp));
        NNGP_TRY(dev_alloc(&h->wt, rp * mp));
        NNGP_TRY(dev_alloc(&h->tscr, std::max(rp, mp) * TB));
    }
    for (double** p : {&h->r, &h->z, &h->p, &h->ap, &h->bt, &h->zt}) {
        NNGP_TRY(dev_alloc(p, rp * np));
        NNGP_HIP_CHECK(hipMemset(*p, 0, sizeof(double) * rp * np));
    }
    NNGP_TRY(dev_alloc(&h->alpha, 16 * np));
    NNGP_HIP_CHECK(hipMemset(h->alpha, 0, sizeof(double) * 16 * np));
    // the split count is a quotient rounded up: at most 2048 + (column blocks) partial blocks of 64 x 64 for any n <= n_cap
    h->ws_doubles = (2048 + (h->n_cap + 63) / 64) * (int64_t)(64 * 64);
    NNGP_TRY(dev_alloc(&h->ws, h->ws_doubles));
    NNGP_TRY(dev_alloc(&h->scal, 4 * rp + 1));
    NNGP_HIP_CHECK(hipMemset(h->scal, 0, sizeof(double) * (4 * rp + 1)));
    if (hipHostMalloc(reinterpret_cast<void**>(&h->host), sizeof(double) * (3 * rp + 1)) != hipSuccess) {
        h->host = nullptr;
        set_error("matfree_create: hipHostMalloc failed");
        return -1;
    }
    return 0;
}

int mf_check_tol(const char* who, double tol, int max_iter) {
    NNGP_REQUIRE(std::isfinite(tol) && tol > 0.0 && tol < 1.0, "%s: tol must be finite and in (0, 1) (tol=%g)", who, tol);
    NNGP_REQUIRE(max_iter >= 1, "%s: max_iter must be >= 1 (max_iter=%d)", who, max_iter);
    return 0;
}

// Z = P^-1 R on all rp rows (m = 0 never comes here)
int mf_precond(nngp_matfree* h, hipStream_t s) {
    const int64_t np = h->np, rp = h->rp, mp = h->mp;
    NNGP_TRY(launch_gemm_nt_f64(h->tt, mp, nullptr, 0, h->r, np, h->vtt, np, rp, mp, np, 1.0, 0.0, s));
    NNGP_TRY(trsm_fwd_f64(h->tt, mp, rp, h->sp->lb, mp, h->sp->dinv_b, mp, h->tscr, false, s));
    NNGP_TRY(launch_gemm_nt_f64(h->wt, mp, nullptr, 0, h->tt, mp, h->lbit, mp, rp, mp, mp, 1.0, 0.0, s));
    const double is2 = 1.0 / h->sigma2;
    return launch_gemm_nt_f64(h->z, np, h->r, np, h->wt, mp, h->vt, mp, rp, np, mp, -is2, is2, s);
}

struct MfStat {
    int iterations = 0, k_passes = 0, restarts = 0;
    double rel_residual = 0.0;
    bool converged = false;
};

int mf_read(nngp_matfree* h, hipStream_t s) {  // host[0 .. 3 rp) = |b|^2, |r|^2, state
    NNGP_HIP_CHECK(hipMemcpyAsync(h->host, h->scal + h->rp, sizeof(double) * 3 * h->rp, hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

// x [r, ldx] = A^-1 b [r, ldb], r <= rp.  0: every column's true residual <= tol; 1: not within max_iter
int mf_solve(nngp_matfree* h, const double* b, int64_t ldb, int r, double* x, int64_t ldx, double tol, int max_iter, hipStream_t s,
             MfStat* st) {
    const int64_t np = h->np, rp = h->rp, n = h->n;
    const double tol2 = tol * tol;
    const dim3 grid((unsigned)r), blk(256);
    auto apply = [&](const double* v, int64_t ldv) {
        ++st->k_passes;
        return launch_kmv_f64(h->ap, np, v, ldv, r, h->x, h->q, n, h->d, h->arch, h->sigma2, h->ws, h->ws_doubles, s);
    };
    auto active = [&]() {
        for (int c = 0; c < r; ++c)
            if (h->host[2 * rp + c] == 0.0) return true;
        return false;
    };
    hipLaunchKernelGGL(k_mf_begin, grid, blk, 0, s, b, ldb, x, ldx, h->r, np, n, h->scal, rp, tol2);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_TRY(mf_read(h, s));
    bool first = true;
    for (;;) {
        while (st->iterations < max_iter && active()) {
            const double* z = h->r;  // m = 0: P = I
            if (h->m > 0) {
                NNGP_TRY(mf_precond(h, s));
                z = h->z;
            }
            hipLaunchKernelGGL(k_mf_dir, grid, blk, 0, s, h->r, z, h->p, np, n, h->scal, rp, first ? 1 : 0);
            NNGP_HIP_CHECK(hipGetLastError());
            first = false;
            NNGP_TRY(apply(h->p, np));
            hipLaunchKernelGGL(k_mf_step, grid, blk, 0, s, x, ldx, h->r, h->p, h->ap, np, n, h->scal, rp, tol2);
            NNGP_HIP_CHECK(hipGetLastError());
            ++st->iterations;
            NNGP_TRY(mf_read(h, s));
        }
        // the true residual, never the recurrence's
        NNGP_TRY(apply(x, ldx));
        hipLaunchKernelGGL(k_mf_resid, grid, blk, 0, s, b, ldb, h->ap, h->r, np, n, h->scal, rp, tol2);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_TRY(mf_read(h, s));
        double worst = 0.0;
        bool ok = true;
        for (int c = 0; c < r; ++c) {
            const double bn2 = h->host[c], rr = h->host[rp + c];
            const double rel = bn2 > 0.0 ? std::sqrt(rr / bn2) : (rr == 0.0 ? 0.0 : INFINITY);
            if (!(rel <= tol)) ok = false;
            if (!(rel <= worst)) worst = rel;  // a NaN is kept
        }
        st->rel_residual = worst;
        st->converged = ok;
        if (ok || st->restarts >= 1 || st->iterations >= max_iter) break;
        ++st->restarts;  // k_mf_resid left r = the true residual and the columns above tol iterating
        first = true;
    }
    return st->converged ? 0 : 1;
}

void mf_note(nngp_matfree* h, const MfStat& st, bool merge) {
    if (!merge) {
        h->iterations = st.iterations;
        h->k_passes = st.k_passes;
        h->restarts = st.restarts;
        h->rel_residual = st.rel_residual;
        h->converged = st.converged ? 1 : 0;
        return;
    }
    h->iterations = std::max(h->iterations, st.iterations);
    h->k_passes += st.k_passes;
    h->restarts += st.restarts;
    if (!(st.rel_residual <= h->rel_residual)) h->rel_residual = st.rel_residual;
    h->converged = (h->converged && st.converged) ? 1 : 0;
}

}  // namespace

}  // namespace nngp

using namespace nngp;

extern "C" {

// groups: NULL, or the table of an additive handle -- the handle's own copy for the operator, the diagonal and the cross build, and
// the caller's for the sparse handle, which copies it too
static int mf_create(nngp_matfree** out, int64_t n_cap, int64_t m_cap, int64_t chunk_rows, int64_t rhs_cap, int32_t d, int32_t ny,
                     const nngp_arch_act* arch, const nngp_groups* groups, double diag_reg, int32_t diag_reg_absolute_scale,
                     double jitter) {
    NNGP_REQUIRE(n_cap >= 1 && n_cap <= ((int64_t)1 << 26), "matfree_create: n_cap must be in 1 .. 2^26 (n_cap=%lld)", (long long)n_cap);
    NNGP_REQUIRE(m_cap >= 0 && m_cap <= 16384, "matfree_create: m_cap must be in 0 .. 16384 (m_cap=%lld)", (long long)m_cap);
    NNGP_REQUIRE(chunk_rows >= TB && chunk_rows % TB == 0, "matfree_create: chunk_rows must be a positive multiple of %d (chunk_rows=%lld)",
                 TB, (long long)chunk_rows);
    NNGP_REQUIRE(rhs_cap >= 1 && rhs_cap <= 4096 && d >= 1, "matfree_create: need 1 <= rhs_cap <= 4096 and d >= 1 (rhs_cap=%lld, d=%d)",
                 (long long)rhs_cap, d);
    NNGP_REQUIRE(ny >= 1 && ny <= 16, "matfree_create: ny must be in 1 .. 16 (ny=%d)", ny);
    NNGP_REQUIRE(std::isfinite(diag_reg) && diag_reg >= 0.0, "matfree_create: diag_reg must be finite and >= 0 (diag_reg=%g)", diag_reg);
    NNGP_REQUIRE(std::isfinite(jitter) && jitter >= 0.0, "matfree_create: jitter must be finite and >= 0 (jitter=%g)", jitter);
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    nngp_matfree* h = new (std::nothrow) nngp_matfree();
    NNGP_REQUIRE(h != nullptr, "matfree_create: out of host memory");
    h->n_cap = n_cap;
    h->np = round_up(n_cap, TB);
    h->m_cap = m_cap;
    h->mp_cap = round_up(m_cap, TB);
    h->chunk_rows = chunk_rows;
    h->rhs_cap = rhs_cap;
    h->rp = round_up(rhs_cap, TB);
    h->d = d;
    h->ny = ny;
    h->arch = ad;
    h->diag_reg = diag_reg;
    h->absolute = diag_reg_absolute_scale != 0;
    h->jitter = jitter;
    int rc = 0;
    if (groups != nullptr) {
        bool plain = false;
        rc = groups_create(groups, d, &h->groups, &plain);
        if (rc == 0 && !plain) h->arch.groups = &h->groups;
    }
    if (rc == 0) rc = mf_alloc(h);
    if (rc == 0 && m_cap > 0)
        rc = nngp_sparse_create(&h->sp, m_cap, chunk_rows, TB, d, ny, arch, h->arch.groups != nullptr ? groups : nullptr, diag_reg,
                                diag_reg_absolute_scale, jitter);
    if (rc != 0) {
        mf_free(h);
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

int nngp_matfree_create(nngp_matfree** out, int64_t n_cap, int64_t m_cap, int64_t chunk_rows, int64_t rhs_cap, int32_t d, int32_t ny,
                        const nngp_arch_act* arch, const nngp_groups* groups, int32_t get, double diag_reg,
                        int32_t diag_reg_absolute_scale, double jitter) {
    NNGP_REQUIRE(out != nullptr && arch != nullptr, "matfree_create: NULL argument");
    *out = nullptr;
    NNGP_REQUIRE(get == NNGP_GET_NNGP, "matfree_create: only the NNGP kernel has a GP posterior to solve for (get=%d)", get);
    NNGP_REQUIRE(groups == nullptr || (groups->n_groups == 0 && groups->full_weight == 1.0),
                 "matfree_create: additive kernels are not supported by the fused operator");
    return mf_create(out, n_cap, m_cap, chunk_rows, rhs_cap, d, ny, arch, nullptr, diag_reg, diag_reg_absolute_scale, jitter);
}

int nngp_matfree_create_additive(nngp_matfree** out, int64_t n_cap, int64_t m_cap, int64_t chunk_rows, int64_t rhs_cap, int32_t d,
                                 int32_t ny, const nngp_arch_act* arch, const nngp_groups* groups, double diag_reg,
                                 int32_t diag_reg_absolute_scale, double jitter) {
    NNGP_REQUIRE(out != nullptr && arch != nullptr, "matfree_create: NULL argument");
    *out = nullptr;
    NNGP_REQUIRE(groups != nullptr, "groups: the group table is NULL");
    return mf_create(out, n_cap, m_cap, chunk_rows, rhs_cap, d, ny, arch, groups, diag_reg, diag_reg_absolute_scale, jitter);
}

int nngp_matfree_destroy(nngp_matfree* h) {
    if (h == nullptr) return 0;
    (void)hipDeviceSynchronize();
    mf_free(h);
    delete h;
    return 0;
}

int nngp_matfree_fit(nngp_matfree* h, const double* x, const double* y, int64_t n, const double* u, int64_t m, double tol,
                     int32_t max_iter, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && x != nullptr && y != nullptr, "matfree_fit: NULL argument");
    NNGP_REQUIRE(n >= 1 && n <= h->n_cap, "matfree_fit: n=%lld outside [1, n_cap=%lld]", (long long)n, (long long)h->n_cap);
    NNGP_REQUIRE(m >= 0 && m <= h->m_cap && (m > 0) == (u != nullptr),
                 "matfree_fit: m=%lld outside [0, m_cap=%lld], or inducing rows without a count (u = NULL goes with m = 0)", (long long)m,
                 (long long)h->m_cap);
    NNGP_TRY(mf_check_tol("matfree_fit", tol, max_iter));
    h->fitted = false;
    h->n = h->m = h->mp = 0;
    h->sigma2 = 0.0;
    const int64_t np = h->np, rp = h->rp;
    NNGP_HIP_CHECK(hipMemcpyAsync(h->x, x, sizeof(double) * n * h->d, hipMemcpyDeviceToDevice, s));
    NNGP_TRY(launch_row_sqnorm(h->x, n, h->d, h->q, s));
    for (double* p : {h->r, h->z, h->p, h->ap, h->bt, h->zt}) NNGP_HIP_CHECK(hipMemsetAsync(p, 0, sizeof(double) * rp * np, s));
    NNGP_HIP_CHECK(hipMemsetAsync(h->alpha, 0, sizeof(double) * 16 * np, s));
    if (m > 0) {
        nngp_sparse* sp = h->sp;
        NNGP_TRY(nngp_sparse_set_inducing(sp, u, m, stream));
        NNGP_TRY(nngp_sparse_add_rows(sp, x, y, n, stream));
        NNGP_TRY(nngp_sparse_finish(sp, stream));
        const int64_t mp = sp->mp;
        h->sigma2 = sp->sigma2;
        // Vt, kept: the chunk walk of add_rows once more, each chunk to its own rows
        NNGP_HIP_CHECK(hipMemsetAsync(h->vt, 0, sizeof(double) * np * mp, s));
        for (int64_t r0 = 0; r0 < n; r0 += h->chunk_rows) {
            const int64_t c = (n - r0 < h->chunk_rows) ? n - r0 : h->chunk_rows;
            NNGP_TRY(sparse_cross(sp, h->x + r0 * h->d, h->q + r0, c, h->vt + r0 * mp, s));
        }
        hipLaunchKernelGGL(k_mf_transpose, dim3((unsigned)(np / 32), (unsigned)(mp / 32)), dim3(256), 0, s, h->vt, mp, h->vtt, np, np, mp);
        hipLaunchKernelGGL(k_eye, dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, s, h->lbit, mp, mp);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_TRY(trsm_fwd_f64(h->lbit, mp, mp, sp->lb, mp, sp->dinv_b, mp, h->tscr, true, s));
        h->mp = mp;
    } else {
        NNGP_TRY(launch_kernel_diag(h->x, h->q, n, h->d, h->arch, h->kd, nullptr, s));
        hipLaunchKernelGGL(k_mf_sum, dim3(1), dim3(256), 0, s, h->kd, n, h->scal + 4 * rp);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_HIP_CHECK(hipMemcpyAsync(h->host + 3 * rp, h->scal + 4 * rp, sizeof(double), hipMemcpyDeviceToHost, s));
        NNGP_HIP_CHECK(hipStreamSynchronize(s));
        h->sigma2 = h->absolute ? h->diag_reg : h->diag_reg * (h->host[3 * rp] / (double)n);
    }
    if (!(h->sigma2 > 0.0) || !std::isfinite(h->sigma2)) {
        set_error("matfree_fit: the noise sigma2 = %g is not positive and finite (diag_reg = %g)", h->sigma2, h->diag_reg);
        return -3;
    }
    h->n = n;
    h->m = m;
    for (int c = 0; c < h->ny; ++c) NNGP_TRY(launch_strided_copy_f64(y + c, h->ny, h->bt + c * np, 1, n, s));
    MfStat st;
    const int rc = mf_solve(h, h->bt, np, h->ny, h->alpha, np, tol, max_iter, s, &st);
    if (rc < 0) return rc;
    mf_note(h, st, false);
    h->fitted = true;
    if (rc == 1)
        set_error("matfree_fit: true relative residual %.3e above tol %.3e after %d iterations", st.rel_residual, tol, st.iterations);
    return rc;
}

int nngp_matfree_solve(nngp_matfree* h, const double* b, int64_t ldb, int32_t r, double* out, int64_t ldo, double tol, int32_t max_iter,
                       void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && b != nullptr && out != nullptr && b != out, "matfree_solve: NULL argument, or out aliases b");
    NNGP_REQUIRE(h->fitted, "matfree_solve: no fit");
    NNGP_REQUIRE(r >= 1 && r <= h->rhs_cap, "matfree_solve: r=%d outside [1, rhs_cap=%lld]", r, (long long)h->rhs_cap);
    NNGP_REQUIRE(ldb >= h->n && ldo >= h->n, "matfree_solve: leading dimensions must be >= n (ldb=%lld, ldo=%lld, n=%lld)", (long long)ldb,
                 (long long)ldo, (long long)h->n);
    NNGP_TRY(mf_check_tol("matfree_solve", tol, max_iter));
    MfStat st;
    const int rc = mf_solve(h, b, ldb, r, out, ldo, tol, max_iter, s, &st);
    if (rc < 0) return rc;
    mf_note(h, st, false);
    if (rc == 1)
        set_error("matfree_solve: true relative residual %.3e above tol %.3e after %d iterations", st.rel_residual, tol, st.iterations);
    return rc;
}

int nngp_matfree_predict(nngp_matfree* h, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var, double tol,
                         int32_t max_iter, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && x_test != nullptr && mean != nullptr, "matfree_predict: NULL argument");
    NNGP_REQUIRE(mt >= 1, "matfree_predict: mt must be >= 1 (mt=%lld)", (long long)mt);
    NNGP_REQUIRE(cov_mode == NNGP_COV_NONE || cov_mode == NNGP_COV_DIAG,
                 "matfree_predict: cov_mode must be NNGP_COV_NONE or NNGP_COV_DIAG (the full covariance is not offered; cov_mode=%d)", cov_mode);
    NNGP_REQUIRE(cov_mode == NNGP_COV_NONE || var != nullptr, "matfree_predict: NULL variance output");
    NNGP_REQUIRE(h->fitted, "matfree_predict: no fit");
    NNGP_TRY(mf_check_tol("matfree_predict", tol, max_iter));
    const int64_t np = h->np, n = h->n;
    const bool diag = cov_mode == NNGP_COV_DIAG;
    int worst_rc = 0;
    bool merge = false;
    if (!diag) {  // no solve: the last call's figures are those of a call that did nothing
        MfStat none;
        none.converged = true;
        mf_note(h, none, false);
    }
    for (int64_t r0 = 0; r0 < mt; r0 += h->rhs_cap) {
        const int64_t rows = (mt - r0 < h->rhs_cap) ? mt - r0 : h->rhs_cap;
        const double* xt = x_test + r0 * h->d;
        NNGP_TRY(launch_row_sqnorm(xt, rows, h->d, h->xq, s));
        if (diag) NNGP_TRY(launch_kernel_diag(xt, h->xq, rows, h->d, h->arch, h->kd, nullptr, s));
        BuildArgs b{};
        b.x1 = xt;
        b.x2 = h->x;
        b.q1 = h->xq;
        b.q2 = h->q;
        b.n1 = rows;
        b.n2 = n;
        b.d = h->d;
        b.row_begin = 0;
        b.row_end = rows;
        b.sym = 0;
        b.nngp64 = h->bt;
        b.ld64 = b.ld32 = np;
        NNGP_TRY(launch_kernel_build(b, h->arch, s));
        if (diag) {
            MfStat st;
            const int rc = mf_solve(h, h->bt, np, (int)rows, h->zt, np, tol, max_iter, s, &st);
            if (rc < 0) return rc;
            mf_note(h, st, merge);
            merge = true;
            if (rc == 1) {
                worst_rc = 1;
                set_error("matfree_predict: true relative residual %.3e above tol %.3e after %d iterations (test rows %lld ..)",
                          st.rel_residual, tol, st.iterations, (long long)r0);
            }
        }
        hipLaunchKernelGGL(k_mf_predict_finish, dim3((unsigned)rows), dim3(256), 0, s, h->bt, h->zt, np, n, h->alpha, h->ny, h->kd,
                           mean + r0 * h->ny, diag ? var + r0 : nullptr, (diag && h->arch.groups != nullptr) ? h->r : nullptr);
        NNGP_HIP_CHECK(hipGetLastError());
    }
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    return worst_rc;
}

int nngp_matfree_alpha(nngp_matfree* h, double* alpha_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && alpha_out != nullptr, "matfree_alpha: NULL argument");
    NNGP_REQUIRE(h->fitted, "matfree_alpha: no fit");
    for (int c = 0; c < h->ny; ++c) NNGP_TRY(launch_strided_copy_f64(h->alpha + c * h->np, 1, alpha_out + c, h->ny, h->n, s));
    return 0;
}

int nngp_matfree_info(nngp_matfree* h, nngp_matfree_info_t* info) {
    NNGP_REQUIRE(h != nullptr && info != nullptr, "matfree_info: NULL argument");
    info->n = h->n;
    info->m = h->m;
    info->sigma2 = h->sigma2;
    info->iterations = h->iterations;
    info->k_passes = h->k_passes;
    info->rel_residual = h->rel_residual;
    info->converged = h->converged;
    info->restarts = h->restarts;
    return 0;
}

}  // extern "C"
