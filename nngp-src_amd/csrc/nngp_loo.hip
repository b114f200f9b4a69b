// Leave-one-out cross-validation of the NNGP posterior (include/nngp_loo.h) on the handle of the marginal likelihood
// (nngp_mll.hip): LOO predictions, the mse / nlpd objectives and their gradient with respect to every Dense layer's sigma_w^2,
// sigma_b^2 and the regulariser.  Float64 throughout, on the evidence core of gp_f64.h.
//
// Value (no gradient; all that the NTK gets): K or Theta by the kernel build, potrf_f64, w = L^-1 y, L^-T into zt; alpha_i and
// b_i = [A^-1]_ii are the dot product of row i of L^-T with w and its sum of squares (k_rowdot, one pass) -- no A^-1 product.
// Gradient: A^-1 as for the marginal likelihood, u = A^-1 abar (launch_symv_f64), C = A^-1 diag(bbar) A^-1 on the float64
// MFMA GEMM, then the fused adjoint pass.  Buffers: the handle keeps its 3 Np^2 doubles.  Once alpha and b exist, L^-T is dead,
// so zt takes the column-scaled copy A^-1 diag(bbar); once A^-1 exists the factor is dead as well, so C goes over it (a) and
// nngp_mll_factor_buffer reports an error until an evaluation keeps its factor again.  The pass reads the lower triangle of C
// only, so C is formed in row panels that stop at the diagonal (kLooPanels panels: (P + 1) / 2P of the square's flops).
//
//   k_loo_point          one workgroup, one pass: r_i, s_i, abar_i, bbar_i, the LOO means / variances and both objectives' sums
//   k_loo_scale_cols     zt <- A^-1 diag(bbar)
//   k_nngp_loo_partial   the fused adjoint pass of nngp_adjoint.h from the seeds 1/2 (alpha_i u_j + u_i alpha_j) and C_ij
//   k_loo_finish         one workgroup, fixed order: alpha^T u, tr C, the q chain's per-layer sums, the partial vectors
// No atomics anywhere: repeated evaluations are bit-identical.
// The evaluation itself is loo_evaluate_core, which nngp_mll_loo_evaluate_ard (nngp_ard.hip) calls with relevances.
#include "nngp_adjoint.h"
#include "../../include/nngp_loo.h"

namespace nngp {

namespace {

constexpr int kLooPanels = 8;  // row panels of the lower-triangular C product
enum { kNegB = 0, kAbar = 1, kBbar = 2, kU = 3, kMean = 4, kVar = 5 };  // vectors of nngp_mll::loo (stride np_cap)

// out[0] = sum r_i^2, out[1] = sum [1/2 log(2 pi s_i) + r_i^2 / (2 s_i)].  Rows n .. np (padding) get zeros.
__global__ __launch_bounds__(256) void k_loo_point(const double* alpha, const double* negb, const double* y, int64_t n, int64_t np,
                                                   int objective, double* abar, double* bbar, double* mean, double* var,
                                                   double* out) {
    __shared__ double red[256];
    const double inv_n = 1.0 / (double)n;
    double s_mse = 0.0, s_nlpd = 0.0;
    for (int64_t i = threadIdx.x; i < np; i += 256) {
        double ab = 0.0, bb = 0.0, mu = 0.0, s = 0.0;
        if (i < n) {
            const double b = -negb[i], al = alpha[i];
            const double r = al / b;
            s = 1.0 / b;
            mu = y[i] - r;
            s_mse += r * r;
            s_nlpd += 0.5 * log(2.0 * kPi * s) + (r * r) / (2.0 * s);
            if (objective == NNGP_LOO_MSE) {
                ab = 2.0 * r / b * inv_n;
                bb = -2.0 * (r * r) / b * inv_n;
            } else {
                ab = r * inv_n;                              // alpha_i / (N b_i)
                bb = -(s + r * r) * (0.5 * inv_n);           // -(1 / b_i + alpha_i^2 / b_i^2) / (2 N)
            }
        }
        abar[i] = ab;
        bbar[i] = bb;
        mean[i] = mu;
        var[i] = s;
    }
    const double a = block_sum(s_mse, red);
    const double b = block_sum(s_nlpd, red);
    if (threadIdx.x == 0) {
        out[0] = a;
        out[1] = b;
    }
}

__global__ __launch_bounds__(256) void k_loo_scale_cols(const double* ainv, const double* bbar, double* out, int64_t ld, int64_t np) {
    const int64_t i = blockIdx.y, j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < np) out[i * ld + j] = ainv[i * ld + j] * bbar[j];
}

template <int NLC>
__global__ __launch_bounds__(256) void k_nngp_loo_partial(MllArgs a, ArchDev arch) {
    adjoint_tile<NLC, true>(a, arch);
}

// out[2] = alpha^T u, out[3] = tr C, out[4 + l] = sum_i q_i^(l), out[4 + n_dense + c] = partial component c (c < 2 ncomp)
__global__ __launch_bounds__(256) void k_loo_finish(const double* c, int64_t ld, int64_t n, const double* alpha, const double* u,
                                                    const double* part, int64_t nparts, const double* q, ArchDev arch, double* out) {
    __shared__ double red[256];
    double au = 0.0, tc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        au += alpha[i] * u[i];
        tc += c[i * ld + i];
    }
    au = block_sum(au, red);
    tc = block_sum(tc, red);
    if (threadIdx.x == 0) {
        out[2] = au;
        out[3] = tc;
    }
    const int nd = arch.n_dense;
    finish_qsums(q, n, arch, red, out + 4);
    for (int e = 0; e < 4 * nd; ++e) {
        const double r = finish_part(part, nparts, e, red);
        if (threadIdx.x == 0) out[4 + nd + e] = r;
    }
}

int launch_loo_partial(const MllArgs& a, const ArchDev& arch, hipStream_t s) {
    return launch_by_nlc(arch, a.nparts, "mll_loo", [&](auto nlc, dim3 grid) {
        hipLaunchKernelGGL(k_nngp_loo_partial<decltype(nlc)::value>, grid, dim3(256), 0, s, a, arch);
    });
}

// c (lower triangle, by row panels that end at the diagonal) <- zs ainv^T.  Timing key 15 = 1: the whole square in one product.
int loo_c_product(double* c, const double* zs, const double* ainv, int64_t np, hipStream_t s) {
    if (NNGP_KNOB(15) == 1) return launch_gemm_nt_f64(c, np, nullptr, 0, zs, np, ainv, np, np, np, np, 1.0, 0.0, s);
    const int64_t h = round_up((np + kLooPanels - 1) / kLooPanels, TB);
    for (int64_t r0 = 0; r0 < np; r0 += h) {
        const int64_t r1 = r0 + h < np ? r0 + h : np;
        NNGP_TRY(launch_gemm_nt_f64(c + r0 * np, np, nullptr, 0, zs + r0 * np, np, ainv, np, r1 - r0, r1, np, 1.0, 0.0, s));
    }
    return 0;
}

}  // namespace

int loo_evaluate_core(nngp_mll* h, const nngp_arch_act* arch_in, int get, double diag_reg, int absolute, int objective, double* value,
                      double* grad, const double* rel, double* grad_s, const char* who, hipStream_t s) {
    NNGP_REQUIRE(h != nullptr && arch_in != nullptr && value != nullptr, "%s: NULL argument", who);
    NNGP_REQUIRE(h->w.n > 0, "%s: no training data (nngp_mll_set_train)", who);
    NNGP_REQUIRE(get == NNGP_GET_NNGP || get == NNGP_GET_NTK, "%s: get must be NNGP_GET_NNGP or NNGP_GET_NTK (%d)", who, get);
    NNGP_REQUIRE(objective == NNGP_LOO_NLPD || objective == NNGP_LOO_MSE, "%s: unknown objective %d", who, objective);
    NNGP_REQUIRE(get == NNGP_GET_NNGP || (grad == nullptr && grad_s == nullptr),
                 "%s: no gradient for the NTK (its mean is kernel ridge regression; the ensemble posterior is not a GP "
                 "with prior Theta)", who);
    NNGP_REQUIRE(get == NNGP_GET_NNGP || objective == NNGP_LOO_MSE,
                 "%s: nlpd needs a predictive variance, which the NTK's leave-one-out form does not have", who);
    ArchDev arch{};
    NNGP_TRY(mll_make_arch(arch_in, diag_reg, who, &arch));
    const int nd = arch.n_dense;
    GpWorkspace& w = h->w;
    w.factored = h->have_loo_terms = h->ard.have_terms = false;
    h->loo_get = 0;
    const int64_t n = w.n, np = w.np, npc = w.np_cap;
    double* lv = h->loo;
    const bool want = grad != nullptr || grad_s != nullptr;
    double own_grad[kMaxComp + 1];
    if (want && !grad) grad = own_grad;
    if (rel) NNGP_TRY(ard_begin(h, rel, who, s));
    const double* x = rel ? h->ard.xs : w.x;
    const double* q = rel ? h->ard.q : h->q;

    NNGP_TRY(mll_build_a(h, arch, get, diag_reg, absolute, x, q, s));
    NNGP_TRY(factor_and_solve(&w, want ? kGpSolveInverse : kGpSolveRows, who, s, lv + kNegB * npc));
    hipLaunchKernelGGL(k_loo_point, dim3(1), dim3(256), 0, s, w.alpha, lv + kNegB * npc, w.y, n, np, (int)objective, lv + kAbar * npc,
                       lv + kBbar * npc, lv + kMean * npc, lv + kVar * npc, w.red + kRed);
    NNGP_HIP_CHECK(hipGetLastError());
    const int64_t nparts = gp_lower_tiles(n);
    if (want) {
        NNGP_REQUIRE((np / TB) * np <= w.t_rows * TB, "%s: solve scratch too small for the symmetric product", who);
        NNGP_TRY(launch_symv_f64(w.ainv, np, n, lv + kAbar * npc, lv + kU * npc, 0.0, w.t, np, s));
        hipLaunchKernelGGL(k_loo_scale_cols, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, s, w.ainv, lv + kBbar * npc,
                           w.zt, np, np);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_TRY(loo_c_product(w.a, w.zt, w.ainv, np, s));  // over the factor
        MllArgs ma{x, q, n, w.d, w.a, np, w.alpha, lv + kU * npc, w.part, nparts};
        if (grad_s) NNGP_TRY(launch_ard_partial(h, ma, arch, true, s));  // A^-1 diag(bbar) is dead once C exists
        else NNGP_TRY(launch_loo_partial(ma, arch, s));
        hipLaunchKernelGGL(k_loo_finish, dim3(1), dim3(256), 0, s, w.a, np, n, w.alpha, lv + kU * npc, w.part, nparts, q, arch,
                           w.red + kRed);
        NNGP_HIP_CHECK(hipGetLastError());
        if (grad_s) NNGP_TRY(ard_contract(h, s));
    }
    double r[kRedLen];
    NNGP_HIP_CHECK(hipMemcpyAsync(r, w.red, sizeof(r), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    const double dn = (double)n, tr_k = r[0];
    *value = (objective == NNGP_LOO_MSE ? r[kRed] : r[kRed + 1]) / dn;
    h->n_dense = nd;
    h->loo_get = get;
    w.factored = !want;
    if (!want) return 0;
    const double au = r[kRed + 2], tr_c = r[kRed + 3];
    const double* sq = r + kRed + 4;
    const double* pa = sq + nd;      // rank-two halves of the K components
    const double* pc = pa + 2 * nd;  // C halves
    const int ncomp = 2 * nd;
    double trdk[kMaxComp];
    trace_dk(arch, sq, dn, trdk);
    double* t = h->loo_terms;
    for (int p = 0; p <= ncomp; ++p) {
        double ha, hc;  // sum 1/2 (alpha_i u_j + u_i alpha_j) dA_p,ij and sum C_ij dA_p,ij
        if (p < ncomp) {
            const double ci = absolute ? 0.0 : diag_reg * (trdk[p] / dn);
            ha = pa[p] + ci * au;
            hc = pc[p] + ci * tr_c;
        } else {
            const double ci = absolute ? 1.0 : tr_k / dn;
            ha = ci * au;
            hc = ci * tr_c;
        }
        t[2 * p] = ha;
        t[2 * p + 1] = hc;
        grad[p] = -(ha + hc);
    }
    double* tail = t + 2 * (ncomp + 1);
    tail[0] = au;
    tail[1] = tr_c;
    tail[2] = tr_k;
    for (int p = 0; p < ncomp; ++p) tail[3 + p] = trdk[p];
    h->n_loo_terms = 2 * (ncomp + 1) + 3 + ncomp;
    h->have_loo_terms = true;
    if (grad_s) ard_finish_host(h, arch, diag_reg, absolute, au, tr_c, true, grad_s);
    return 0;
}

}  // namespace nngp

using namespace nngp;

extern "C" {

int nngp_mll_loo_evaluate(nngp_mll* h, const nngp_arch_act* arch_in, int32_t get, double diag_reg, int32_t absolute,
                          int32_t objective, double* value, double* grad, void* stream) {
    return loo_evaluate_core(h, arch_in, get, diag_reg, absolute, objective, value, grad, nullptr, nullptr, "mll_loo_evaluate",
                             (hipStream_t)stream);
}

int nngp_mll_loo_predictions(const nngp_mll* h, double* mean, double* var, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && mean != nullptr, "mll_loo_predictions: NULL argument");
    NNGP_REQUIRE(h->loo_get != 0, "mll_loo_predictions: no leave-one-out evaluation yet (nngp_mll_loo_evaluate)");
    NNGP_REQUIRE(var == nullptr || h->loo_get == NNGP_GET_NNGP,
                 "mll_loo_predictions: the NTK's leave-one-out form has no predictive variance (var must be NULL)");
    const int64_t n = h->w.n, npc = h->w.np_cap;
    NNGP_HIP_CHECK(hipMemcpyAsync(mean, h->loo + kMean * npc, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    if (var) NNGP_HIP_CHECK(hipMemcpyAsync(var, h->loo + kVar * npc, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    return 0;
}

int nngp_mll_loo_terms(const nngp_mll* h, double* out, int32_t count) {
    NNGP_REQUIRE(h != nullptr && out != nullptr, "mll_loo_terms: NULL argument");
    NNGP_REQUIRE(h->have_loo_terms, "mll_loo_terms: no leave-one-out gradient evaluation yet");
    NNGP_REQUIRE(count >= h->n_loo_terms, "mll_loo_terms: count=%d, the last evaluation has %d terms", count, h->n_loo_terms);
    for (int i = 0; i < h->n_loo_terms; ++i) out[i] = h->loo_terms[i];
    return 0;
}

}  // extern "C"
