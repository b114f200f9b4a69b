// Per-feature input relevances (include/nngp_ard.h) for the NNGP evidence (nngp_mll.hip) and the leave-one-out objectives
// (nngp_loo.hip): K_s(x, x') = K(x o sqrt(s), x' o sqrt(s)) and the derivative of either loss with respect to every s_k.
//
//   dL/ds_k = (1/d) [ sum_{j<i} (S o c)_ij x_ik x_jk  +  sum_i qbar_i x_ik^2 ]     per seed S
// with (S o c)_ij and qbar_i what the reverse sweep of adjoint_tile holds once it has passed Dense layer 0: kbar, and qbar1 /
// qbar2 summed over j / i (a diagonal entry's kbar belongs to qbar: K_ii depends on q_i alone).  The off-diagonal weight 2 of
// the lower-triangle pass is already in them, so the strict lower triangle is all there is to contract.
//
//   k_ard_scale          xs = x o sqrt(s)  (s = 1: the bits of x)
//   k_nngp_ard_partial   adjoint_tile with ARD set: the usual partials, S o c of the first seed into the lower triangle of zt
//                        (dead at this point in both paths), of the matrix seed into the upper, and the per-tile sums of qbar
//   k_ard_contract       the hot path, ard_contract_body of ard_contract.h staged from the two triangles of one matrix: per
//                        64-row block I, 32 features and seed, Z_I = sum_{J <= I} (S o c)[I, J] X_J on the float64 MFMA, then
//                        sum_{i in I} x_ik (Z_ik + qbar_i x_ik), rows in order
//   k_ard_finish         the row blocks summed in order
// launch_ard_contract runs the two for the exact evidence, the leave-one-out objectives and the sparse evidence's K_uu half.
// No atomics; every slot of qbar and of the partials has one writer.
#include "ard_contract.h"
#include "../../include/nngp_ard.h"

namespace nngp {

namespace {

__global__ __launch_bounds__(256) void k_ard_scale(const double* x, const double* s, int64_t total, int d, double* xs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) xs[e] = x[e] * sqrt(s[e % d]);
}

template <int NLC, bool LOO>
__global__ __launch_bounds__(256) void k_nngp_ard_partial(MllArgs a, ArchDev arch) {
    adjoint_tile<NLC, LOO, true>(a, arch);
}

// The symmetric form's staging: seed 0 at (i, j), seed 1 at (j, i) of one matrix, j < i < n = nb, every row block walking the
// tiles up to its own; the B operand is x itself.
struct SymStage {
    const double *cmat, *b;
    int64_t ldc, nb;
    __device__ int64_t tiles(int64_t ti) const { return ti + 1; }
    __device__ void stage(double (*ms)[MT + 1], int64_t i0, int64_t j0, int tid) const {
        const int seed = blockIdx.z;
        for (int e = tid; e < MT * MT; e += 256) {  // the fast index runs along memory for either seed
            const int r = seed == 0 ? e >> 6 : e & (MT - 1), c = seed == 0 ? e & (MT - 1) : e >> 6;
            const int64_t i = i0 + r, j = j0 + c;
            ms[r][c] = (i < nb && j < i) ? (seed == 0 ? cmat[i * ldc + j] : cmat[j * ldc + i]) : 0.0;
        }
    }
};

// grid and part as ard_contract_body has them, with tn row blocks; x: the raw inputs
__global__ __launch_bounds__(256) void k_ard_contract(const double* cmat, int64_t ldc, const double* x, int64_t n, int d,
                                                      const double* qbar, int64_t np, int64_t tn, double* part) {
    ard_contract_body(SymStage{cmat, x, ldc, n}, x, n, d, qbar, tn, np, tn, part);
}

// out[v * d + k] = sum over the row blocks, in order, of part[(v * tn + I) * d + k]  (v = 0, 1: the seeds; 2: sum_i x_ik^2)
__global__ __launch_bounds__(256) void k_ard_finish(const double* part, int64_t tn, int d, double* out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < 3 * d) out[e] = ard_block_sum(part, tn, d, e);
}

}  // namespace

int launch_ard_contract(const double* cmat, int64_t ldc, const double* x, int64_t n, int d, const double* qbar, int64_t np, double* part,
                        double* out, hipStream_t s) {
    const int64_t tn = (n + MT - 1) / MT;
    const dim3 grid((unsigned)tn, (unsigned)((d + AKC - 1) / AKC), 2);
    hipLaunchKernelGGL(k_ard_contract, grid, dim3(256), 0, s, cmat, ldc, x, n, d, qbar, np, tn, part);
    hipLaunchKernelGGL(k_ard_finish, dim3((unsigned)((3 * d + 255) / 256)), dim3(256), 0, s, part, tn, d, out);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ard_partial(const MllArgs& a, const ArchDev& arch, bool loo, hipStream_t s) {
    return launch_by_nlc(arch, a.nparts, "mll", [&](auto nlc, dim3 grid) {
        constexpr int NLC = decltype(nlc)::value;
        if (loo) hipLaunchKernelGGL((k_nngp_ard_partial<NLC, true>), grid, dim3(256), 0, s, a, arch);
        else hipLaunchKernelGGL((k_nngp_ard_partial<NLC, false>), grid, dim3(256), 0, s, a, arch);
    });
}

int ard_begin(nngp_mll* h, const double* rel, const char* who, hipStream_t s) {
    ArdBuffers& a = h->ard;
    NNGP_REQUIRE(a.reserved, "%s: relevances need nngp_mll_reserve_ard first", who);
    const int d = h->w.d;
    NNGP_TRY(check_relevances(who, rel, d));
    const int64_t total = h->w.n * d;
    NNGP_HIP_CHECK(hipMemcpyAsync(a.s, rel, sizeof(double) * d, hipMemcpyHostToDevice, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));  // rel is the caller's
    hipLaunchKernelGGL(k_ard_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h->w.x, a.s, total, d, a.xs);
    NNGP_HIP_CHECK(hipGetLastError());
    return launch_row_sqnorm(a.xs, h->w.n, d, a.q, s);
}

int launch_ard_partial(nngp_mll* h, MllArgs a, const ArchDev& arch, bool loo, hipStream_t s) {
    a.cmat = h->w.zt;
    a.ldc = h->w.np;
    a.qbar = h->ard.qbar;
    a.np = h->w.np;
    return launch_ard_partial(a, arch, loo, s);
}

int ard_contract(nngp_mll* h, hipStream_t s) {
    ArdBuffers& a = h->ard;
    const GpWorkspace& w = h->w;
    NNGP_TRY(launch_ard_contract(w.zt, w.np, w.x, w.n, w.d, a.qbar, w.np, a.part, a.out, s));
    NNGP_HIP_CHECK(hipMemcpyAsync(a.host.data(), a.out, sizeof(double) * 3 * w.d, hipMemcpyDeviceToHost, s));
    return 0;
}

void ard_finish_host(nngp_mll* h, const ArchDev& arch, double diag_reg, int absolute, double s1, double s2, bool loo, double* grad_s) {
    ArdBuffers& a = h->ard;
    const int d = h->w.d;
    const double dn = (double)h->w.n, dd = (double)d, d0v0 = diag_q_slope(arch);
    for (int k = 0; k < d; ++k) {
        const double trdk = d0v0 * a.host[2 * d + k] / dd;
        const double ci = absolute ? 0.0 : diag_reg * (trdk / dn);
        const double h1 = a.host[k] / dd + ci * s1, h2 = a.host[d + k] / dd + ci * s2;
        a.terms[2 * k] = h1;
        a.terms[2 * k + 1] = h2;
        a.terms[2 * d + k] = trdk;
        grad_s[k] = loo ? -(h1 + h2) : -0.5 * h1 + 0.5 * h2;
    }
    a.have_terms = true;
}

void ard_free(nngp_mll* h) {
    ArdBuffers& a = h->ard;
    dev_free(a.xs);
    dev_free(a.q);
    dev_free(a.s);
    dev_free(a.qbar);
    dev_free(a.part);
    dev_free(a.out);
    a.reserved = a.have_terms = false;
}

}  // namespace nngp

using namespace nngp;

extern "C" {

int nngp_mll_reserve_ard(nngp_mll* h) {
    NNGP_REQUIRE(h != nullptr, "mll_reserve_ard: NULL argument");
    NNGP_REQUIRE(!h->add.reserved, "mll_reserve_ard: the handle has a group table (nngp_mll_reserve_additive); relevances together "
                                   "with groups are not covered");
    ArdBuffers& a = h->ard;
    if (a.reserved) return 0;
    const GpWorkspace& w = h->w;
    const int64_t tn = (w.n_cap + MT - 1) / MT, d = w.d;
    int rc = dev_alloc(&a.xs, w.n_cap * d);
    if (rc == 0) rc = dev_alloc(&a.q, w.n_cap);
    if (rc == 0) rc = dev_alloc(&a.s, d);
    if (rc == 0) rc = dev_alloc(&a.qbar, 2 * tn * w.np_cap);
    if (rc == 0) rc = dev_alloc(&a.part, 3 * tn * d);
    if (rc == 0) rc = dev_alloc(&a.out, 3 * d);
    if (rc != 0) {
        ard_free(h);
        return rc;
    }
    a.host.assign((size_t)(3 * d), 0.0);
    a.terms.assign((size_t)(3 * d), 0.0);
    a.reserved = true;
    return 0;
}

int nngp_mll_evaluate_ard(nngp_mll* h, const nngp_arch_act* arch, const double* s, double diag_reg, int32_t absolute, double* nlml,
                          double* grad, double* grad_s, void* stream) {
    NNGP_REQUIRE(s != nullptr, "mll_evaluate_ard: NULL argument");
    return mll_evaluate_core(h, arch, diag_reg, absolute, nlml, grad, s, grad_s, "mll_evaluate_ard", (hipStream_t)stream);
}

int nngp_mll_loo_evaluate_ard(nngp_mll* h, const nngp_arch_act* arch, int32_t get, const double* s, double diag_reg, int32_t absolute,
                              int32_t objective, double* value, double* grad, double* grad_s, void* stream) {
    NNGP_REQUIRE(s != nullptr, "mll_loo_evaluate_ard: NULL argument");
    return loo_evaluate_core(h, arch, get, diag_reg, absolute, objective, value, grad, s, grad_s, "mll_loo_evaluate_ard",
                             (hipStream_t)stream);
}

int nngp_mll_ard_terms(const nngp_mll* h, double* out, int32_t count) {
    NNGP_REQUIRE(h != nullptr && out != nullptr, "mll_ard_terms: NULL argument");
    NNGP_REQUIRE(h->ard.have_terms, "mll_ard_terms: no evaluation with grad_s yet");
    const int n_terms = 3 * h->w.d;
    NNGP_REQUIRE(count >= n_terms, "mll_ard_terms: count=%d, the last evaluation has %d terms", count, n_terms);
    for (int i = 0; i < n_terms; ++i) out[i] = h->ard.terms[i];
    return 0;
}

}  // extern "C"
