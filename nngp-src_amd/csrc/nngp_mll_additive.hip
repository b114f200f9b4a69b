// Marginal likelihood of the additive NNGP kernel over feature groups and its gradient, the term weights included
// (include/nngp_additive_mll.h), on the handle and in the evaluation sequence of nngp_mll.hip (mll_evaluate_core).
//
// A = sum_t w_t K^(t) + r I comes from the additive kernel build (ArchDev::groups: the groups with w_g > 0, as every other user
// of that build), so tr K and r are the fitted model's.  Then
//   k_mll_add_partial    adjoint_tile with ADD set (nngp_adjoint.h): one 256-thread workgroup per lower 64 x 64 tile, the terms
//                        walked in the table's order.  Per term: Gram tile and, for a group, both slices' |x_t|^2 from row slices
//                        staged in LDS (float64 VALU: a group's inner dimension is as small as 1); forward recursion; the term's
//                        value times both seeds into the term's two halves; unless w_t == 0 the reverse sweep from the seeds
//                        times w_t into the 2 n_dense accumulators of either seed, shared by all terms.  The term halves are
//                        reduced in the workgroup and written one slot per (term, tile) over L^-T, which is dead by then.
//   k_mll_add_finish     one workgroup per sum, each in the order of k_mll_finish: the four scalar sums, the 4 n_dense layer
//                        partials (with one term of weight 1 the bits of the plain evaluation) and the 2 T term halves
//   k_mll_add_qsums      one workgroup per term: sum_i z_l,i of the term's diagonal q chain, from which tr K^(t) and
//                        tr dK^(t)/dtheta follow in closed form (trace_dk)
// No atomics and no device-side waits; nothing is allocated after nngp_mll_reserve_additive.
#include "nngp_adjoint.h"
#include "../../include/nngp_additive_mll.h"

namespace nngp {

namespace {

template <int NLC>
__global__ __launch_bounds__(256) void k_mll_add_partial(MllArgs a, ArchDev arch, AddTerms add) {
    adjoint_tile<NLC, false, false, true>(a, arch, add);
}

// Workgroup 0: out[0 .. 3] as k_mll_finish.  Workgroups 1 .. 4 n_dense: out[4 + n_dense + c], layer partial c summed over the
// tiles.  The 2 T after them: tred[c], term half c summed over the tiles.
__global__ __launch_bounds__(256) void k_mll_add_finish(const double* l, int64_t ldl, int64_t n, const double* w, const double* part,
                                                        const double* tpart, int64_t nparts, const double* alpha,
                                                        const double* ainv, int nd, double* out, double* tred) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    if (b == 0) {
        double s[4];
        finish_sums(l, ldl, n, w, alpha, ainv, red, s);
        if (threadIdx.x == 0)
            for (int c = 0; c < 4; ++c) out[c] = s[c];
    } else if (b <= 4 * nd) {
        const double r = finish_part(part, nparts, b - 1, red);
        if (threadIdx.x == 0) out[4 + nd + b - 1] = r;
    } else {
        const int c = b - 1 - 4 * nd;
        const double r = finish_part(tpart, nparts, c, red);
        if (threadIdx.x == 0) tred[c] = r;
    }
}

// out[t][l] = sum_i z_l,i of term t (workgroup t): q_i = |x_i|^2 / d for the whole input, the slice's for a group
__global__ __launch_bounds__(256) void k_mll_add_qsums(const double* x, const double* q, int64_t n, int d, const int* gbegin,
                                                       const int* gend, ArchDev arch, double* out) {
    __shared__ double red[256];
    const int t = blockIdx.x;
    double* o = out + (int64_t)t * NNGP_MAX_DENSE;
    if (t == 0) {
        finish_qsums(q, n, arch, red, o);
        return;
    }
    const int kb = gbegin[t - 1], ke = gend[t - 1];
    const double inv_d = 1.0 / (double)(ke - kb);
    finish_qsums_of(
        [=](int64_t i) {
            double s = 0.0;
            for (int k = kb; k < ke; ++k) s = fma(x[i * d + k], x[i * d + k], s);
            return s * inv_d;
        },
        n, arch, red, o);
}

}  // namespace

int add_begin(nngp_mll* h, const double* weights, const char* who, const GroupsDev** groups, hipStream_t s) {
    AddBuffers& a = h->add;
    NNGP_REQUIRE(a.reserved, "%s: the additive evidence needs nngp_mll_reserve_additive first", who);
    const int T = a.n_terms, G = T - 1;
    bool any = false;
    for (int t = 0; t < T; ++t) {
        NNGP_REQUIRE(std::isfinite(weights[t]) && weights[t] >= 0.0, "%s: weight %d must be finite and >= 0 (%g)", who, t, weights[t]);
        any = any || weights[t] > 0.0;
    }
    NNGP_REQUIRE(any, "%s: all weights are zero", who);
    // every weight for the adjoint pass; behind them the build's table: the groups with a non-zero weight, in the caller's order
    int n = 0;
    for (int t = 0; t < T; ++t) a.weight_host[t] = weights[t];
    for (int g = 0; g < G; ++g)
        if (weights[1 + g] > 0.0) {
            a.weight_host[T + n] = weights[1 + g];
            a.range_host[2 * G + n] = a.range_host[g];
            a.range_host[3 * G + n] = a.range_host[G + g];
            ++n;
        }
    NNGP_HIP_CHECK(hipMemcpyAsync(a.weight, a.weight_host.data(), sizeof(double) * (T + G), hipMemcpyHostToDevice, s));
    if (G > 0) NNGP_HIP_CHECK(hipMemcpyAsync(a.range, a.range_host.data(), sizeof(int) * 4 * G, hipMemcpyHostToDevice, s));
    a.dev.n_groups = n;
    a.dev.full_weight = weights[0];
    a.dev.weight = a.weight + T;
    a.dev.begin = a.range + 2 * G;
    a.dev.end = a.range + 3 * G;
    *groups = (n == 0 && weights[0] == 1.0) ? nullptr : &a.dev;  // no group and w0 = 1: the plain kernel (groups_create's rule)
    return 0;
}

int launch_add_partial(nngp_mll* h, const MllArgs& a, const ArchDev& arch, hipStream_t s) {
    const AddBuffers& b = h->add;
    const int G = b.n_terms - 1;
    NNGP_REQUIRE(2 * (int64_t)b.n_terms * a.nparts <= h->w.np * h->w.np, "mll: the term partials do not fit the L^-T storage");
    const AddTerms add{b.n_terms, b.range, b.range + G, b.weight, h->w.zt};
    return launch_by_nlc(arch, a.nparts, "mll", [&](auto nlc, dim3 grid) {
        hipLaunchKernelGGL(k_mll_add_partial<decltype(nlc)::value>, grid, dim3(256), 0, s, a, arch, add);
    });
}

int launch_add_finish(nngp_mll* h, const ArchDev& arch, int64_t nparts, hipStream_t s) {
    AddBuffers& a = h->add;
    const GpWorkspace& w = h->w;
    const int T = a.n_terms, nd = arch.n_dense;
    hipLaunchKernelGGL(k_mll_add_finish, dim3((unsigned)(1 + 4 * nd + 2 * T)), dim3(256), 0, s, w.a, w.np, w.n, w.wrow, w.part, w.zt,
                       nparts, w.alpha, w.ainv, nd, w.red + kRed, a.red);
    hipLaunchKernelGGL(k_mll_add_qsums, dim3((unsigned)T), dim3(256), 0, s, w.x, h->q, w.n, w.d, a.range, a.range + (T - 1), arch,
                       a.red + 2 * T);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_HIP_CHECK(hipMemcpyAsync(a.red_host.data(), a.red, sizeof(double) * a.red_host.size(), hipMemcpyDeviceToHost, s));
    return 0;
}

void add_trace_dk(const nngp_mll* h, const ArchDev& arch, double dn, double* trdk) {
    const AddBuffers& a = h->add;
    const int T = a.n_terms, nd = arch.n_dense;
    for (int p = 0; p < 2 * nd; ++p) trdk[p] = 0.0;
    for (int t = 0; t < T; ++t) {
        const double wt = a.weight_host[t];
        if (wt == 0.0) continue;
        double one[kMaxComp];
        trace_dk(arch, a.red_host.data() + 2 * T + (size_t)t * NNGP_MAX_DENSE, dn, one);
        for (int p = 0; p < 2 * nd; ++p) trdk[p] += wt * one[p];
    }
}

void add_finish_host(nngp_mll* h, const ArchDev& arch, double diag_reg, int absolute, double aa, double tr_ainv, double* grad_w) {
    AddBuffers& a = h->add;
    const int T = a.n_terms, nd = arch.n_dense;
    const double dn = (double)h->w.n;
    for (int t = 0; t < T; ++t) {
        // K^(t)_ii = v_last z_last,i + c_last
        const double tr_kt = arch.w2[nd - 1] * a.red_host[2 * T + (size_t)t * NNGP_MAX_DENSE + nd - 1] + arch.b2[nd - 1] * dn;
        const double ci = absolute ? 0.0 : diag_reg * (tr_kt / dn);
        const double h1 = a.red_host[2 * t] + ci * aa, h2 = a.red_host[2 * t + 1] + ci * tr_ainv;
        a.terms[2 * t] = h1;
        a.terms[2 * t + 1] = h2;
        a.terms[2 * T + t] = tr_kt;
        grad_w[t] = -0.5 * h1 + 0.5 * h2;
    }
    a.have_terms = true;
}

void add_free(nngp_mll* h) {
    AddBuffers& a = h->add;
    dev_free(a.range);
    dev_free(a.weight);
    dev_free(a.red);
    a.dev = GroupsDev{};
    a.reserved = a.have_terms = false;
    a.n_terms = 0;
}

}  // namespace nngp

using namespace nngp;

extern "C" {

int nngp_mll_reserve_additive(nngp_mll* h, const nngp_groups* g) {
    NNGP_REQUIRE(h != nullptr, "mll_reserve_additive: NULL argument");
    NNGP_REQUIRE(!h->ard.reserved, "mll_reserve_additive: the handle has relevances (nngp_mll_reserve_ard); relevances together "
                                   "with groups are not covered");
    NNGP_REQUIRE(g != nullptr, "groups: the group table is NULL");
    NNGP_REQUIRE(g->n_groups >= 0 && g->n_groups <= NNGP_MAX_GROUPS, "groups: n_groups must be in [0, %d] (got %d)", NNGP_MAX_GROUPS,
                 g->n_groups);
    NNGP_REQUIRE(g->n_groups == 0 || (g->begin != nullptr && g->end != nullptr), "groups: begin / end is NULL");
    const int G = g->n_groups, T = G + 1, d = h->w.d;
    for (int i = 0; i < G; ++i)
        NNGP_REQUIRE(0 <= g->begin[i] && g->begin[i] < g->end[i] && g->end[i] <= d,
                     "groups: group %d has the range [%d, %d), outside 0 <= begin < end <= d = %d", i, g->begin[i], g->end[i], d);
    (void)hipDeviceSynchronize();  // a second call replaces the table: nothing may still read the old one
    add_free(h);
    AddBuffers& a = h->add;
    int rc = dev_alloc(&a.range, 4 * G);
    if (rc == 0) rc = dev_alloc(&a.weight, T + G);
    if (rc == 0) rc = dev_alloc(&a.red, (int64_t)T * (2 + NNGP_MAX_DENSE));
    if (rc != 0) {
        add_free(h);
        return rc;
    }
    a.range_host.assign((size_t)(4 * G), 0);
    for (int i = 0; i < G; ++i) {
        a.range_host[i] = g->begin[i];
        a.range_host[G + i] = g->end[i];
    }
    a.weight_host.assign((size_t)(T + G), 0.0);
    a.red_host.assign((size_t)T * (2 + NNGP_MAX_DENSE), 0.0);
    a.terms.assign((size_t)(3 * T), 0.0);
    a.n_terms = T;
    a.reserved = true;
    h->have_terms = false;
    return 0;
}

int nngp_mll_evaluate_additive(nngp_mll* h, const nngp_arch_act* arch, const double* weights, double diag_reg, int32_t absolute,
                               double* nlml, double* grad, double* grad_w, void* stream) {
    NNGP_REQUIRE(weights != nullptr, "mll_evaluate_additive: NULL argument");
    return mll_evaluate_core(h, arch, diag_reg, absolute, nlml, grad, nullptr, nullptr, "mll_evaluate_additive", (hipStream_t)stream,
                             weights, grad_w);
}

int nngp_mll_additive_terms(const nngp_mll* h, double* out, int32_t count) {
    NNGP_REQUIRE(h != nullptr && out != nullptr, "mll_additive_terms: NULL argument");
    NNGP_REQUIRE(h->add.have_terms, "mll_additive_terms: no evaluation with grad_w yet");
    const int n_terms = 3 * h->add.n_terms;
    NNGP_REQUIRE(count >= n_terms, "mll_additive_terms: count=%d, the last evaluation has %d terms", count, n_terms);
    for (int i = 0; i < n_terms; ++i) out[i] = h->add.terms[i];
    return 0;
}

}  // extern "C"
