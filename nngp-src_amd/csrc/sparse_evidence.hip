// The evidence of the sparse (inducing-point) NNGP and its gradient (include/nngp_sparse_evidence.h), all float64, on the handle
// of sparse_gp.hip.
//
// The value needs no pass over the data: add_rows keeps y^T y beside G, R and tr K_ff, and the rest are sums over L_B, C and G.
// The gradient hands the rows again and contracts dK / dtheta with its seeds entry by entry, never forming it:
//
//   once per call   K~_uu^-1, M = L_u^-T B^-1 L_u^-1 and gamma on the float64 core of gp_f64.hip (triangular solves of the identity
//                   and products on the float64 MFMA GEMM); then the exact evidence's symmetric adjoint pass over K_uu
//                   (launch_mll_partial of nngp_mll.hip, k_nngp_mll_partial: alpha := gamma, the matrix seed := E with the
//                   jitter's share on its diagonal)
//   per chunk       the cross build K_cu (no solve), beta_c = (y_c - K_cu gamma) / sigma2, D_c = K_cu M' on the MFMA GEMM, and
//   k_sparse_rect_partial   (sparse_rect.h) the adjoint of the layer recursion over the rectangular block K(X_c, U).  One workgroup
//                   per 64 x 64 tile of (rows of X_c) x (rows of U); it runs the pieces of nngp_adjoint.h that adjoint_tile
//                   runs -- the q chains of the tile's rows and columns in the kernel build's order of operations, the Gram
//                   tile from LDS-staged feature chunks, per entry the forward recursion (ReLU and ABRelu, the q = 0 rule,
//                   pi_minus_atan2 on kTrigTab) and the reverse sweep -- but every entry of the tile counts once, there is no
//                   exact-diagonal rule (a training row that is also an inducing row takes the general formula, as in the
//                   cross build), and the seeds are the rank-one beta_i gamma_j (the "quad" half) and the dense D[i, j] (the
//                   "trace" half).  Each tile writes its 2 n_dense partials per half to a slot of its own;
//   k_ev_reduce     one workgroup sums the slots in ascending order and adds the chunk's sums to the accumulators.
// No float atomics, no device-side counter, no workgroup waits for another: a launch boundary is the only synchronisation, so
// nothing here can hang and two runs give the same bits.
#include "sparse_rect.h"
#include "sparse_gp.h"
#include "../../include/nngp_sparse_evidence.h"

namespace nngp {

namespace {

template <int NLC>
__global__ __launch_bounds__(256) void k_sparse_rect_partial(RectArgs a, ArchDev arch) {
    rect_tile<NLC>(a, arch);
}

// acc[c] += sum over the nparts slots of component c, in ascending order (one workgroup)
__global__ __launch_bounds__(256) void k_ev_reduce(const double* part, int64_t nparts, int ncomp4, double* acc) {
    __shared__ double red[256];
    for (int c = 0; c < ncomp4; ++c) {
        const double r = finish_part(part, nparts, c, red);
        if (threadIdx.x == 0) acc[c] += r;
    }
}

// dst (full square) <- G, of which only the 128 x 128 tiles on or below the diagonal are kept
__global__ __launch_bounds__(256) void k_ev_mirror(const double* __restrict__ g, double* __restrict__ dst, int64_t mp) {
    const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < mp) dst[i * mp + j] = (i / TB >= j / TB) ? g[i * mp + j] : g[j * mp + i];
}

__global__ __launch_bounds__(256) void k_ev_axpby(double* __restrict__ dst, double a, const double* __restrict__ src, double b,
                                                  int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) dst[e] = a * dst[e] + b * src[e];
}

// K~_uu = K_uu + jitter / m tr(K_uu) I, so the matrix seed gets jitter / m tr(E) on its diagonal (one workgroup, fixed order)
__global__ __launch_bounds__(256) void k_ev_seed_jitter(double* e, int64_t ld, int64_t m, double jitter) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) s += e[i * ld + i];
    const double add = jitter * (block_sum(s, red) / (double)m);
    for (int64_t i = threadIdx.x; i < m; i += 256) e[i * ld + i] += add;
}

// sums[0] = sum_i log (L_B)_ii, sums[1] = |C|^2, sums[2] = tr G, over the true m (one workgroup, fixed order)
__global__ __launch_bounds__(256) void k_ev_value_sums(const double* lb, const double* gm, const double* ct, int64_t mp, int64_t m,
                                                       double* sums) {
    __shared__ double red[256];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < m; i += 256) {
        v[0] += log(lb[i * mp + i]);
        v[1] += ct[i] * ct[i];
        v[2] += gm[i * mp + i];
    }
    for (int c = 0; c < 3; ++c) {
        const double r = block_sum(v[c], red);
        if (threadIdx.x == 0) sums[c] = r;
    }
}

// sums[3] = |gamma|^2, sums[5] = tr B^-1 = |L_B^-T|_F^2 (neg_rowsq: minus its row sums of squares); qu[l] = sum_j q_u,j^(l)
__global__ __launch_bounds__(256) void k_ev_grad_sums(const double* gamma, const double* neg_rowsq, const double* uq, int64_t m,
                                                      ArchDev arch, double* sums, double* qu) {
    __shared__ double red[256];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) {
        a += gamma[i] * gamma[i];
        b -= neg_rowsq[i];
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        sums[3] = a;
        sums[5] = b;
    }
    finish_qsums(uq, m, arch, red, qu);
}

// one workgroup per row of the chunk: beta_i = (y_i - sum_j K_ij gamma_j) / sigma2
__global__ __launch_bounds__(256) void k_ev_beta(const double* __restrict__ k, int64_t ld, int64_t m, const double* __restrict__ gamma,
                                                 const double* __restrict__ y, double sigma2, double* __restrict__ beta) {
    __shared__ double red[256];
    const double* row = k + (int64_t)blockIdx.x * ld;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < m; j += 256) s += row[j] * gamma[j];
    s = block_sum(s, red);
    if (threadIdx.x == 0) beta[blockIdx.x] = (y[blockIdx.x] - s) / sigma2;
}

// *acc += sum_i v_i^2 (one workgroup, fixed order)
__global__ __launch_bounds__(256) void k_ev_sumsq(const double* v, int64_t count, double* acc) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += 256) s += v[i] * v[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *acc += s;
}

// qacc[l] += sum_i q_i^(l) of a chunk
__global__ __launch_bounds__(256) void k_ev_qsums(const double* q, int64_t c, ArchDev arch, double* qacc) {
    __shared__ double red[256];
    __shared__ double out[NNGP_MAX_DENSE];
    finish_qsums(q, c, arch, red, out);
    __syncthreads();
    if ((int)threadIdx.x < arch.n_dense) qacc[threadIdx.x] += out[threadIdx.x];
}

int launch_rect(const RectArgs& a, const ArchDev& arch, hipStream_t s) {
    return launch_by_nlc(arch, a.nparts, "sparse_evidence", [&](auto nlc, dim3 grid) {
        hipLaunchKernelGGL(k_sparse_rect_partial<decltype(nlc)::value>, grid, dim3(256), 0, s, a, arch);
    });
}

int reduce_into(const double* part, int64_t nparts, int ncomp4, double* acc, hipStream_t s) {
    hipLaunchKernelGGL(k_ev_reduce, dim3(1), dim3(256), 0, s, part, nparts, ncomp4, acc);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

bool has_erf(const ArchDev& arch) {
    for (int l = 0; l < arch.n_dense - 1; ++l)
        if (arch.act[l] == NNGP_ACT_ERF) return true;
    return false;
}

// the checks shared by the value and the gradient; all before any GPU work
int evidence_check(const nngp_sparse* h, int bound, const char* who) {
    NNGP_REQUIRE(bound == NNGP_BOUND_DTC || bound == NNGP_BOUND_VFE, "%s: bound must be NNGP_BOUND_DTC or NNGP_BOUND_VFE (bound=%d)", who,
                 bound);
    NNGP_REQUIRE(h->ny == 1, "%s: the evidence takes one output column (ny=%d)", who, h->ny);
    NNGP_REQUIRE(h->arch.groups == nullptr, "%s: the evidence does not cover the additive kernel over feature groups", who);
    NNGP_REQUIRE(!has_erf(h->arch), "%s: a hidden layer is Erf; the evidence covers ReLU and ABRelu only", who);
    NNGP_REQUIRE(h->m > 0 && h->finished, "%s: no nngp_sparse_finish since the last rows were added", who);
    return 0;
}

double nlml_of(const nngp_sparse* h, const double* sc, int bound) {
    const double s2 = h->sigma2, dn = (double)h->n, dm = (double)h->m;
    double v = 0.5 * (sc[kSpYY] - sc[kSpSums + 1]) / s2 + 0.5 * (dn - dm) * log(s2) + sc[kSpSums] + 0.5 * dn * log(2.0 * kPi);
    if (bound == NNGP_BOUND_VFE) v += (sc[0] - sc[kSpSums + 2]) / (2.0 * s2);
    return v;
}

int value_sums(nngp_sparse* h, hipStream_t s) {
    hipLaunchKernelGGL(k_ev_value_sums, dim3(1), dim3(256), 0, s, h->lb, h->gm, h->ct, h->mp, h->m, h->scal + kSpSums);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int sparse_evidence_sums(nngp_sparse* h, const double* xq, const double* y, int64_t c, hipStream_t s) {
    hipLaunchKernelGGL(k_ev_sumsq, dim3(1), dim3(256), 0, s, y, c * h->ny, h->scal + kSpYY);
    hipLaunchKernelGGL(k_ev_qsums, dim3(1), dim3(256), 0, s, xq, c, h->arch, h->scal + kSpQ);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

void sparse_evidence_free(nngp_sparse* h) {
    for (double** p : {&h->ev_a, &h->ev_m, &h->ev_t, &h->ev_d, &h->ev_vec, &h->ev_part}) dev_free(*p);
    h->ev_reserved = false;
    sparse_ard_free(h);
}

}  // namespace nngp

using namespace nngp;

extern "C" {

int nngp_sparse_reserve_evidence(nngp_sparse* h) {
    NNGP_REQUIRE(h != nullptr, "sparse_reserve_evidence: NULL argument");
    if (h->ev_reserved) return 0;
    const int64_t mp = h->mp_cap;
    const int64_t rect = ((h->chunk_rows + MT - 1) / MT) * ((h->m_cap + MT - 1) / MT), sym = gp_lower_tiles(h->m_cap);
    h->ev_tiles = rect > sym ? rect : sym;
    int rc = dev_alloc(&h->ev_a, mp * mp);
    if (rc == 0) rc = dev_alloc(&h->ev_m, mp * mp);
    if (rc == 0) rc = dev_alloc(&h->ev_t, mp * mp);
    if (rc == 0) rc = dev_alloc(&h->ev_d, h->chunk_rows * mp);
    if (rc == 0) rc = dev_alloc(&h->ev_vec, 2 * mp + h->chunk_rows);
    if (rc == 0) rc = dev_alloc(&h->ev_part, 4 * (int64_t)h->arch.n_dense * h->ev_tiles);
    if (rc != 0) {
        sparse_evidence_free(h);
        return rc;
    }
    h->ev_reserved = true;
    return 0;
}

int nngp_sparse_set_kernel(nngp_sparse* h, const nngp_arch_act* arch, double diag_reg, int32_t diag_reg_absolute_scale) {
    NNGP_REQUIRE(h != nullptr && arch != nullptr, "sparse_set_kernel: NULL argument");
    ArchDev ad{};
    NNGP_TRY(mll_make_arch(arch, diag_reg, "sparse_set_kernel", &ad));
    NNGP_REQUIRE(ad.n_dense == h->arch.n_dense, "sparse_set_kernel: the handle was created for %d Dense layers, got %d", h->arch.n_dense,
                 ad.n_dense);
    ad.groups = h->arch.groups;
    h->arch = ad;
    h->diag_reg = diag_reg;
    h->absolute = diag_reg_absolute_scale != 0;
    sparse_drop_fit(h);
    return 0;
}

int nngp_sparse_evidence(nngp_sparse* h, int32_t bound, double* nlml, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && nlml != nullptr, "sparse_evidence: NULL argument");
    NNGP_TRY(evidence_check(h, bound, "sparse_evidence"));
    NNGP_TRY(value_sums(h, s));
    double sc[kSpSums + 3];
    NNGP_HIP_CHECK(hipMemcpyAsync(sc, h->scal, sizeof(sc), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    *nlml = nlml_of(h, sc, bound);
    return 0;
}

int nngp_sparse_evidence_grad(nngp_sparse* h, const double* x, const double* y, int64_t n, int32_t bound, double* nlml, double* grad,
                              void* stream) {
    NNGP_REQUIRE(h != nullptr && x != nullptr && y != nullptr && nlml != nullptr && grad != nullptr, "sparse_evidence_grad: NULL argument");
    return sparse_evidence_grad_core(h, x, y, n, bound, nlml, grad, nullptr, "sparse_evidence_grad", (hipStream_t)stream);
}

}  // extern "C"

int nngp::sparse_evidence_grad_core(nngp_sparse* h, const double* x, const double* y, int64_t n, int bound, double* nlml, double* grad,
                                    double* grad_s, const char* who, hipStream_t s) {
    NNGP_TRY(evidence_check(h, bound, who));
    NNGP_REQUIRE(h->ev_reserved, "%s: the evidence was not reserved (nngp_sparse_reserve_evidence)", who);
    NNGP_REQUIRE(n == h->n, "%s: n=%lld, but %lld rows were added", who, (long long)n, (long long)h->n);
    const bool ard = grad_s != nullptr;
    NNGP_REQUIRE(!ard || h->have_rel, "%s: no relevances on the handle (nngp_sparse_set_relevance)", who);
    h->have_terms = false;
    h->have_ard_terms = false;
    const bool vfe = bound == NNGP_BOUND_VFE;
    const int64_t m = h->m, mp = h->mp;
    const int nd = h->arch.n_dense, ncomp = 2 * nd;
    const double s2 = h->sigma2;
    double* A = h->ev_a;
    double* M = h->ev_m;
    double* T = h->ev_t;
    double* gamma = h->ev_vec;
    double* rowsq = h->ev_vec + h->mp_cap;
    double* beta = h->ev_vec + 2 * h->mp_cap;
    double* scratch = h->ev_d;  // mp x 128 of it: the solves of the identity run before any chunk
    const dim3 sq((unsigned)((mp + 255) / 256), (unsigned)mp);

    // ---- once per call ----
    NNGP_HIP_CHECK(hipMemsetAsync(h->scal + kSpSums, 0, sizeof(double) * (kSpScal - kSpSums), s));
    NNGP_TRY(value_sums(h, s));
    // tr B^-1 = |L_B^-T|_F^2
    hipLaunchKernelGGL(k_eye, sq, dim3(256), 0, s, T, mp, mp);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_TRY(trsm_fwd_f64(T, mp, mp, h->lb, mp, h->dinv_b, mp, scratch, true, s));
    hipLaunchKernelGGL(k_rowdot, dim3((unsigned)m), dim3(256), 0, s, T, mp, m, nullptr, nullptr, 0.0, rowsq, 0.0);
    // T = L_u^-T
    hipLaunchKernelGGL(k_eye, sq, dim3(256), 0, s, T, mp, mp);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_TRY(trsm_fwd_f64(T, mp, mp, h->lu, mp, h->dinv_u, mp, scratch, true, s));
    if (vfe) {  // M = L_u^-T G L_u^-1
        hipLaunchKernelGGL(k_ev_mirror, sq, dim3(256), 0, s, h->gm, M, mp);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_TRY(launch_gemm_nt_f64(A, mp, nullptr, 0, T, mp, M, mp, mp, mp, mp, 1.0, 0.0, s));
        NNGP_TRY(launch_gemm_nt_f64(M, mp, nullptr, 0, A, mp, T, mp, mp, mp, mp, 1.0, 0.0, s));
    }
    NNGP_TRY(launch_gemm_nt_f64(A, mp, nullptr, 0, T, mp, T, mp, mp, mp, mp, 1.0, 0.0, s));  // A = K~_uu^-1
    NNGP_TRY(trsm_fwd_f64(T, mp, mp, h->lb, mp, h->dinv_b, mp, scratch, true, s));            // T = L_u^-T L_B^-T =: W
    hipLaunchKernelGGL(k_rowdot, dim3((unsigned)mp), dim3(256), 0, s, T, mp, mp, h->ct, gamma, 0.0, nullptr, 0.0);  // gamma = W C
    NNGP_HIP_CHECK(hipGetLastError());
    // the matrix seed of K~_uu in M: E = -A + sigma2 W W^T (+ L_u^-T G L_u^-1 / sigma2); then M' = W W^T (- A / sigma2) in A
    if (vfe) {
        hipLaunchKernelGGL(k_ev_axpby, dim3((unsigned)((mp * mp + 255) / 256)), dim3(256), 0, s, M, 1.0 / s2, A, -1.0, mp * mp);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_TRY(launch_gemm_nt_f64(M, mp, M, mp, T, mp, T, mp, mp, mp, mp, s2, 1.0, s));
        NNGP_TRY(launch_gemm_nt_f64(A, mp, A, mp, T, mp, T, mp, mp, mp, mp, 1.0, -1.0 / s2, s));
    } else {
        NNGP_TRY(launch_gemm_nt_f64(M, mp, A, mp, T, mp, T, mp, mp, mp, mp, s2, -1.0, s));
        NNGP_TRY(launch_gemm_nt_f64(A, mp, nullptr, 0, T, mp, T, mp, mp, mp, mp, 1.0, 0.0, s));
    }
    hipLaunchKernelGGL(k_ev_seed_jitter, dim3(1), dim3(256), 0, s, M, mp, m, h->jitter);
    hipLaunchKernelGGL(k_ev_grad_sums, dim3(1), dim3(256), 0, s, gamma, rowsq, h->uq, m, h->arch, h->scal + kSpSums, h->scal + kSpQu);
    NNGP_HIP_CHECK(hipGetLastError());
    {
        const int64_t tiles = gp_lower_tiles(m);
        if (ard) {  // T = W is dead from here on: the seeded adjoints of K0 over K_uu go there
            NNGP_TRY(sparse_ard_begin(h, s));
            NNGP_TRY(sparse_ard_uu(h, M, gamma, T, s));
        } else {
            MllArgs ma{h->u, h->uq, m, h->d, M, mp, gamma, nullptr, h->ev_part, tiles};
            NNGP_TRY(launch_mll_partial(ma, h->arch, s));  // the exact evidence's own pass, seeded with gamma and E
        }
        NNGP_TRY(reduce_into(h->ev_part, tiles, 2 * ncomp, h->scal + kSpAccUu, s));
    }

    // ---- per chunk ----
    const int64_t tu = (m + MT - 1) / MT;
    for (int64_t r0 = 0; r0 < n; r0 += h->chunk_rows) {
        const int64_t c = (n - r0 < h->chunk_rows) ? n - r0 : h->chunk_rows, rp = round_up(c, TB);
        const double* xraw = x + r0 * h->d;
        const double* xc = xraw;
        if (h->have_rel) {
            NNGP_TRY(sparse_ard_scale(h, xraw, c, h->ard_xs, s));
            xc = h->ard_xs;
        }
        NNGP_TRY(launch_row_sqnorm(xc, c, h->d, h->xq, s));
        NNGP_TRY(sparse_cross(h, xc, h->xq, c, h->chunk, s, 2));  // K_cu, no solve
        hipLaunchKernelGGL(k_ev_beta, dim3((unsigned)c), dim3(256), 0, s, h->chunk, mp, m, gamma, y + r0, s2, beta);
        hipLaunchKernelGGL(k_ev_sumsq, dim3(1), dim3(256), 0, s, beta, c, h->scal + kSpSums + 4);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_TRY(launch_gemm_nt_f64(h->ev_d, mp, nullptr, 0, h->chunk, mp, A, mp, rp, mp, mp, 1.0, 0.0, s));  // D_c = K_cu M'
        const int64_t nparts = ((c + MT - 1) / MT) * tu;
        if (ard) {
            NNGP_TRY(sparse_ard_chunk(h, xraw, xc, c, beta, gamma, s));
        } else {
            RectArgs ra{xc, h->xq, c, h->u, h->uq, m, h->d, h->ev_d, mp, beta, gamma, h->ev_part, nparts, tu};
            NNGP_TRY(launch_rect(ra, h->arch, s));
        }
        NNGP_TRY(reduce_into(h->ev_part, nparts, 2 * ncomp, h->scal + kSpAccFu, s));
    }
    if (ard) NNGP_TRY(sparse_ard_end(h, s));

    // ---- the fixed-order finish on the host ----
    double sc[kSpScal];
    NNGP_HIP_CHECK(hipMemcpyAsync(sc, h->scal, sizeof(sc), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    *nlml = nlml_of(h, sc, bound);
    const double dn = (double)n, dm = (double)m, lam = h->diag_reg;
    const double tr_kff = sc[0], tr_g = sc[kSpSums + 2], gg = sc[kSpSums + 3], bb = sc[kSpSums + 4], tr_binv = sc[kSpSums + 5];
    double trdk_f[kMaxComp], trdk_u[kMaxComp];
    trace_dk(h->arch, sc + kSpQ, dn, trdk_f);
    trace_dk(h->arch, sc + kSpQu, dm, trdk_u);
    const double ts = (dn - dm + s2 * tr_binv) / s2 - (vfe ? (tr_kff - tr_g) / (s2 * s2) : 0.0);
    const double* fu_q = sc + kSpAccFu;
    const double* fu_t = fu_q + ncomp;
    const double* uu_q = sc + kSpAccUu;
    const double* uu_t = uu_q + ncomp;
    double* t = h->terms;
    for (int p = 0; p <= ncomp; ++p) {
        double qa, ta;
        if (p < ncomp) {
            const double ds2 = h->absolute ? 0.0 : lam * (trdk_f[p] / dn);
            qa = 2.0 * fu_q[p] - (uu_q[p] + h->jitter / dm * trdk_u[p] * gg) + bb * ds2;
            ta = 2.0 * fu_t[p] + uu_t[p] + ts * ds2 + (vfe ? trdk_f[p] / s2 : 0.0);
        } else {
            const double ci = h->absolute ? 1.0 : tr_kff / dn;
            qa = bb * ci;
            ta = ts * ci;
        }
        t[2 * p] = qa;
        t[2 * p + 1] = ta;
        if (grad != nullptr) grad[p] = -0.5 * qa + 0.5 * ta;
    }
    if (ard) sparse_ard_finish_host(h, vfe, s2, ts, bb, gg, grad_s);
    double* tail = t + 2 * (ncomp + 1);
    tail[0] = sc[kSpSums];
    tail[1] = sc[kSpYY] - sc[kSpSums + 1];
    tail[2] = tr_kff;
    tail[3] = tr_g;
    tail[4] = s2;
    tail[5] = tr_binv;
    tail[6] = bb;
    h->n_terms = 2 * (ncomp + 1) + 7;
    h->have_terms = true;
    return 0;
}

extern "C" {

int nngp_sparse_evidence_terms(const nngp_sparse* h, double* out, int32_t count) {
    NNGP_REQUIRE(h != nullptr && out != nullptr, "sparse_evidence_terms: NULL argument");
    NNGP_REQUIRE(h->have_terms, "sparse_evidence_terms: no gradient evaluation yet");
    NNGP_REQUIRE(count >= h->n_terms, "sparse_evidence_terms: count=%d, the last evaluation has %d terms", count, h->n_terms);
    for (int i = 0; i < h->n_terms; ++i) out[i] = h->terms[i];
    return 0;
}

int nngp_sparse_adjoint_rect(const double* x, int64_t c, const double* u, int64_t m, int32_t d, const nngp_arch_act* arch,
                             const double* seed, int64_t ld, const double* beta, const double* gamma, double* out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(x != nullptr && u != nullptr && arch != nullptr && seed != nullptr && beta != nullptr && gamma != nullptr && out != nullptr,
                 "sparse_adjoint_rect: NULL argument");
    NNGP_REQUIRE(c >= 1 && m >= 1 && d >= 1 && ld >= m, "sparse_adjoint_rect: need c, m, d >= 1 and ld >= m (c=%lld m=%lld d=%d ld=%lld)",
                 (long long)c, (long long)m, d, (long long)ld);
    ArchDev ad{};
    NNGP_TRY(mll_make_arch(arch, 0.0, "sparse_adjoint_rect", &ad));
    const int n4 = 4 * ad.n_dense;
    const int64_t tu = (m + MT - 1) / MT, tiles = ((c + MT - 1) / MT) * tu;
    double *xq, *uq, *acc, *part;
    return with_stream_block(s, {{&xq, c}, {&uq, m}, {&acc, n4}, {&part, n4 * tiles}}, [&]() -> int {
        NNGP_TRY(launch_row_sqnorm(x, c, d, xq, s));
        NNGP_TRY(launch_row_sqnorm(u, m, d, uq, s));
        NNGP_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(double) * n4, s));
        RectArgs ra{x, xq, c, u, uq, m, d, seed, ld, beta, gamma, part, tiles, tu};
        NNGP_TRY(launch_rect(ra, ad, s));
        NNGP_TRY(reduce_into(part, tiles, n4, acc, s));
        NNGP_HIP_CHECK(hipMemcpyAsync(out, acc, sizeof(double) * n4, hipMemcpyDeviceToHost, s));
        return 0;
    });
}

}  // extern "C"
