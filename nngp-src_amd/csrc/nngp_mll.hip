// NNGP marginal likelihood and its gradient (include/nngp_mll.h): the evidence of the NNGP posterior of
// stax.serial(Dense, (act, Dense)*), act ReLU or ABRelu, and its derivative with respect to every Dense layer's sigma_w^2,
// sigma_b^2 and the regulariser -- what neural-tangents users get by differentiating the NLML through kernel_fn with autodiff.
//
// Everything is float64 and factors on its own (the float32 factor of the NNGP fit gives neither log det A nor tr(A^-1 dA) to
// float64 grade): K is built by the kernel build (launch_kernel_build, per-layer recursion, no composite
// map), then the float64 core of gp_f64.h factors it and forms w, A^-1 and alpha, as for the RBF GP.
//
//   k_mll_pad            identity on the padding rows / columns of A (n .. Np)
//   k_mll_diag           tr K (fixed order) and r = lambda tr K / N (or lambda) added to the diagonal
//   k_nngp_mll_partial   the new hot path: one pass over the lower 64 x 64 tiles.  Per tile the Gram x_i.x_j / d is recomputed
//                        (float64 VALU), then per entry the layer recursion runs forward, keeping each layer's input k and the
//                        activation's partials (dK'/dk, s) in registers, and backward (adjoint) from the two seeds
//                        alpha_i alpha_j and A^-1_ij (x 2 off the diagonal), accumulating 2 n_dense partials per seed.  No
//                        dK/dtheta matrix exists anywhere; the partials are reduced in a fixed order, one vector per workgroup.
//   k_mll_finish         one workgroup, fixed order: the partial vectors, sum log L_ii, |w|^2, alpha^T alpha, tr A^-1 and the
//                        per-layer sums of the diagonal's q chain (tr dK/dtheta follows from them in closed form)
// No atomics anywhere: repeated evaluations are bit-identical.
// The evaluation itself is mll_evaluate_core: nngp_mll_evaluate calls it without relevances, nngp_mll_evaluate_ard (nngp_ard.hip) with
// them -- one sequence, so that unit relevances give the bits of the entry point without.
#include "nngp_adjoint.h"

#include <vector>

namespace nngp {

namespace {

__global__ __launch_bounds__(256) void k_mll_pad(double* a, int64_t ld, int64_t n, int64_t np) {
    const int64_t i = blockIdx.x;
    for (int64_t j = (i < n ? n : 0) + threadIdx.x; j < np; j += 256) a[i * ld + j] = i == j ? 1.0 : 0.0;
}

// red[0] = tr K, red[1] = r; the diagonal of A gets + r
__global__ __launch_bounds__(256) void k_mll_diag(double* a, int64_t ld, int64_t n, double lambda, int absolute, double* red) {
    __shared__ double sred[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += a[i * ld + i];
    const double tr = block_sum(s, sred);
    const double r = absolute ? lambda : lambda * (tr / (double)n);
    for (int64_t i = threadIdx.x; i < n; i += 256) a[i * ld + i] += r;
    if (threadIdx.x == 0) {
        red[0] = tr;
        red[1] = r;
    }
}

// the fused adjoint pass (nngp_adjoint.h) from the seeds alpha_i alpha_j and A^-1_ij
template <int NLC>
__global__ __launch_bounds__(256) void k_nngp_mll_partial(MllArgs a, ArchDev arch) {
    adjoint_tile<NLC, false>(a, arch);
}

// One workgroup, fixed order.  out[0] = sum log L_ii, out[1] = |w|^2 (= y^T A^-1 y), out[2] = alpha^T alpha, out[3] = tr A^-1,
// out[4 + l] = sum_i q_i^(l) (the diagonal's q at the input of Dense layer l), out[4 + n_dense + c] = sum over workgroups of
// partial component c (c < 2 ncomp).  Without part / alpha: the first two only.
__global__ __launch_bounds__(256) void k_mll_finish(const double* l, int64_t ldl, int64_t n, const double* w, const double* part,
                                                    int64_t nparts, const double* alpha, const double* ainv, const double* q,
                                                    ArchDev arch, double* out) {
    __shared__ double red[256];
    double s[4];
    finish_sums(l, ldl, n, w, alpha, ainv, red, s);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) out[c] = s[c];
    if (!alpha) return;
    const int nd = arch.n_dense;
    finish_qsums(q, n, arch, red, out + 4);
    for (int c = 0; c < 4 * nd; ++c) {
        const double r = finish_part(part, nparts, c, red);
        if (threadIdx.x == 0) out[4 + nd + c] = r;
    }
}

}  // namespace

int launch_mll_partial(const MllArgs& a, const ArchDev& arch, hipStream_t s) {
    return launch_by_nlc(arch, a.nparts, "mll", [&](auto nlc, dim3 grid) {
        hipLaunchKernelGGL(k_nngp_mll_partial<decltype(nlc)::value>, grid, dim3(256), 0, s, a, arch);
    });
}

int mll_make_arch(const nngp_arch_act* arch_in, double diag_reg, const char* who, ArchDev* out) {
    ArchDev& arch = *out;
    NNGP_TRY(make_arch_dev_act(arch_in, &arch));
    const int nd = arch.n_dense;
    for (int l = 0; l < nd; ++l) {
        const double w = arch_in->base.w_std[l], b = arch_in->base.b_std[l];
        NNGP_REQUIRE(std::isfinite(w) && std::isfinite(b) && w >= 0.0 && b >= 0.0,
                     "%s: w_std / b_std of Dense layer %d must be finite and non-negative (%g, %g)", who, l, w, b);
    }
    for (int l = 0; l < nd - 1; ++l)
        NNGP_REQUIRE(arch.act[l] != NNGP_ACT_ERF, "%s: hidden layer %d is Erf; the gradient covers ReLU and ABRelu only", who, l);
    NNGP_REQUIRE(std::isfinite(diag_reg) && diag_reg >= 0.0, "%s: diag_reg must be finite and non-negative (%g)", who, diag_reg);
    return 0;
}

// K (or Theta) by the kernel build (per-layer recursion: no_comp), the padding the identity, r on the diagonal
int mll_build_a(nngp_mll* h, const ArchDev& arch, int get, double diag_reg, int absolute, const double* x, const double* q,
                hipStream_t s) {
    GpWorkspace& w = h->w;
    const int64_t n = w.n, np = w.np;
    BuildArgs b = symmetric_build_args(x, q, n, w.d);
    if (get == NNGP_GET_NTK) b.ntk64 = w.a;
    else b.nngp64 = w.a;
    b.ld64 = np;
    b.no_comp = 1;
    NNGP_TRY(launch_kernel_build(b, arch, s));
    hipLaunchKernelGGL(k_mll_pad, dim3((unsigned)np), dim3(256), 0, s, w.a, np, n, np);
    hipLaunchKernelGGL(k_mll_diag, dim3(1), dim3(256), 0, s, w.a, np, n, diag_reg, (int)(absolute != 0), w.red);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

int mll_evaluate_core(nngp_mll* h, const nngp_arch_act* arch_in, double diag_reg, int absolute, double* nlml, double* grad,
                      const double* rel, double* grad_s, const char* who, hipStream_t s, const double* weights, double* grad_w) {
    NNGP_REQUIRE(h != nullptr && arch_in != nullptr && nlml != nullptr, "%s: NULL argument", who);
    NNGP_REQUIRE(h->w.n > 0, "%s: no training data (nngp_mll_set_train)", who);
    ArchDev arch{};
    NNGP_TRY(mll_make_arch(arch_in, diag_reg, who, &arch));
    const int nd = arch.n_dense;
    GpWorkspace& w = h->w;
    w.factored = h->have_terms = h->ard.have_terms = h->add.have_terms = false;
    const int64_t n = w.n, np = w.np;
    if (rel) NNGP_TRY(ard_begin(h, rel, who, s));
    if (weights) NNGP_TRY(add_begin(h, weights, who, &arch.groups, s));
    const double* x = rel ? h->ard.xs : w.x;
    const double* q = rel ? h->ard.q : h->q;
    NNGP_TRY(mll_build_a(h, arch, NNGP_GET_NNGP, diag_reg, absolute, x, q, s));
    const bool want = grad != nullptr || grad_s != nullptr || grad_w != nullptr;
    double own_grad[kMaxComp + 1];
    if (want && !grad) grad = own_grad;
    NNGP_TRY(factor_and_solve(&w, want, who, s));
    const int64_t nparts = gp_lower_tiles(n);
    if (want) {
        MllArgs ma{x, q, n, w.d, w.ainv, np, w.alpha, nullptr, w.part, nparts};
        if (grad_s) NNGP_TRY(launch_ard_partial(h, ma, arch, false, s));  // L^-T is dead: the seeded adjoints go over it
        else if (weights) NNGP_TRY(launch_add_partial(h, ma, arch, s));     // and so do the term partials
        else NNGP_TRY(launch_mll_partial(ma, arch, s));
    }
    if (want && weights) {
        NNGP_TRY(launch_add_finish(h, arch, nparts, s));
    } else {
        hipLaunchKernelGGL(k_mll_finish, dim3(1), dim3(256), 0, s, w.a, np, n, w.wrow, want ? w.part : nullptr, nparts,
                           want ? w.alpha : nullptr, w.ainv, q, arch, w.red + kRed);
        NNGP_HIP_CHECK(hipGetLastError());
    }
    if (grad_s) NNGP_TRY(ard_contract(h, s));
    double r[kRedLen];
    NNGP_HIP_CHECK(hipMemcpyAsync(r, w.red, sizeof(r), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    const double tr_k = r[0], logdet_half = r[kRed], yay = r[kRed + 1];
    const double dn = (double)n;
    *nlml = 0.5 * yay + logdet_half + 0.5 * dn * log(2.0 * kPi);
    h->n_dense = nd;
    w.factored = true;
    if (!want) return 0;
    const double aa = r[kRed + 2], tr_ainv = r[kRed + 3];
    const double* sq = r + kRed + 4;
    const double* pa = sq + nd;         // alpha alpha^T halves of the K components
    const double* pi = pa + 2 * nd;     // A^-1 halves
    const int ncomp = 2 * nd;
    double trdk[kMaxComp];
    if (weights) add_trace_dk(h, arch, dn, trdk);
    else trace_dk(arch, sq, dn, trdk);
    double* t = h->terms;
    for (int p = 0; p <= ncomp; ++p) {
        double qa, ta;  // alpha^T dA_p alpha, tr(A^-1 dA_p)
        if (p < ncomp) {
            const double ci = absolute ? 0.0 : diag_reg * (trdk[p] / dn);
            qa = pa[p] + ci * aa;
            ta = pi[p] + ci * tr_ainv;
        } else {
            const double ci = absolute ? 1.0 : tr_k / dn;
            qa = ci * aa;
            ta = ci * tr_ainv;
        }
        t[2 * p] = qa;
        t[2 * p + 1] = ta;
        grad[p] = -0.5 * qa + 0.5 * ta;
    }
    double* tail = t + 2 * (ncomp + 1);
    tail[0] = logdet_half;
    tail[1] = yay;
    tail[2] = tr_k;
    tail[3] = aa;
    tail[4] = tr_ainv;
    for (int p = 0; p < ncomp; ++p) tail[5 + p] = trdk[p];
    h->n_terms = 2 * (ncomp + 1) + 5 + ncomp;
    h->have_terms = true;
    if (grad_s) ard_finish_host(h, arch, diag_reg, absolute, aa, tr_ainv, false, grad_s);
    if (grad_w) add_finish_host(h, arch, diag_reg, absolute, aa, tr_ainv, grad_w);
    return 0;
}

}  // namespace nngp

using namespace nngp;

// ---------------------------------------------------------------------------------------------------------------------------
// C ABI (include/nngp_mll.h)

static void mll_free(nngp_mll* h) {
    ard_free(h);
    add_free(h);
    dev_free(h->q);
    dev_free(h->loo);
    ws_free(&h->w);
}

extern "C" {

int nngp_mll_create(nngp_mll** out, int64_t n_cap, int32_t d) {
    NNGP_REQUIRE(out != nullptr && n_cap > 0 && d >= 1, "mll_create: bad arguments (n_cap=%lld, d=%d)", (long long)n_cap, d);
    *out = nullptr;
    nngp_mll* h = new (std::nothrow) nngp_mll();
    NNGP_REQUIRE(h != nullptr, "mll_create: out of host memory");
    // solve scratch: Np x 128 for the triangular solves; (Np / 128) x Np for the symmetric product u = A^-1 abar of the
    // leave-one-out gradient (launch_symv_f64's partial rows), whichever is larger
    const int64_t np_cap = round_up(n_cap, TB), blocks = np_cap / TB;
    int rc = dev_alloc(&h->q, n_cap);
    if (rc == 0) rc = dev_alloc(&h->loo, kLooVec * np_cap);
    if (rc == 0) rc = ws_alloc(&h->w, n_cap, d, 2 * kMaxComp, kRedLen, blocks * blocks > np_cap ? blocks * blocks : np_cap);
    if (rc != 0) {
        mll_free(h);
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

int nngp_mll_destroy(nngp_mll* h) {
    if (h == nullptr) return 0;
    (void)hipDeviceSynchronize();
    mll_free(h);
    delete h;
    return 0;
}

int nngp_mll_set_train(nngp_mll* h, const double* x, const double* y, int64_t n, int32_t ny, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && x != nullptr && y != nullptr, "mll_set_train: NULL argument");
    NNGP_REQUIRE(ny == 1, "mll_set_train: the marginal likelihood takes one output column (ny=%d)", ny);
    NNGP_REQUIRE(n >= 1 && n <= h->w.n_cap, "mll_set_train: n=%lld outside [1, n_cap=%lld]", (long long)n, (long long)h->w.n_cap);
    h->have_terms = h->have_loo_terms = h->ard.have_terms = false;
    h->loo_get = 0;
    NNGP_TRY(launch_row_sqnorm(x, n, h->w.d, h->q, s));  // from the caller's x: ws_set_train's synchronise covers it
    return ws_set_train(&h->w, x, y, hipMemcpyDeviceToDevice, n, s);
}

int nngp_mll_evaluate(nngp_mll* h, const nngp_arch_act* arch_in, double diag_reg, int32_t absolute, double* nlml, double* grad,
                      void* stream) {
    return mll_evaluate_core(h, arch_in, diag_reg, absolute, nlml, grad, nullptr, nullptr, "mll_evaluate", (hipStream_t)stream);
}

int nngp_mll_terms(const nngp_mll* h, double* out, int32_t count) {
    NNGP_REQUIRE(h != nullptr && out != nullptr, "mll_terms: NULL argument");
    NNGP_REQUIRE(h->have_terms, "mll_terms: no gradient evaluation yet");
    NNGP_REQUIRE(count >= h->n_terms, "mll_terms: count=%d, the last evaluation has %d terms", count, h->n_terms);
    for (int i = 0; i < h->n_terms; ++i) out[i] = h->terms[i];
    return 0;
}

int nngp_mll_factor_buffer(const nngp_mll* h, double** l, int64_t* ld, int64_t* n_padded) {
    NNGP_REQUIRE(h != nullptr && l != nullptr && ld != nullptr, "mll_factor_buffer: NULL argument");
    NNGP_REQUIRE(h->w.factored, "mll_factor_buffer: no factor (nngp_mll_evaluate)");
    *l = h->w.a;
    *ld = h->w.np;
    if (n_padded) *n_padded = h->w.np;
    return 0;
}

}  // extern "C"
