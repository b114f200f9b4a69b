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
#include "gp_f64.h"
#include "f64_math.h"
#include "trig_tab.h"

#include <cmath>
#include <vector>

namespace nngp {

namespace {

constexpr int MT = kGpTile;    // tile edge of the fused gradient pass
constexpr int MKC = 32;        // feature chunk staged in LDS
constexpr int MLD = MKC + 1;   // LDS row stride (odd: the 16 rows a wave reads sit in different banks)
constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxComp = 2 * NNGP_MAX_DENSE;  // gradient components of K
constexpr int kRed = 8;                       // scalar sums of k_mll_diag / k_mll_finish (see nngp_mll::red)

struct MllArgs {
    const double* x;      // [n, d]
    const double* q;      // [n]: |x_i|^2 / d
    int64_t n;
    int d;
    const double* ainv;   // [Np, ld]: A^-1
    int64_t ld;
    const double* alpha;  // [Np]
    double* part;         // [2 ncomp][nparts]: the alpha alpha^T half of every component, then the A^-1 half
    int64_t nparts;
};

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

// NLC: room for n_dense <= NLC layers (the per-entry state lives in registers, so its size must be known at compile time).
template <int NLC>
__global__ __launch_bounds__(256) void k_nngp_mll_partial(MllArgs a, ArchDev arch) {
    __shared__ __attribute__((aligned(16))) double sm[2 * MT * MLD];  // the two row panels, then the Gram tile [MT][MT + 1]
    __shared__ double qs[NLC][2 * MT];  // rows | columns: q at the input of Dense layer l
    __shared__ double rq[NLC][2 * MT];  // 1 / (4 pi q') with q' after Dense layer l; 0 where q' = 0 (the q = 0 rule)
    __shared__ __attribute__((aligned(16))) double tab[65 * 4];
    __shared__ double red[256];
    static_assert(MT * (MT + 1) <= 2 * MT * MLD, "the Gram tile aliases the panels");
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    const int nd = arch.n_dense;
    const int64_t tn = (a.n + MT - 1) / MT;
    int64_t ti, tj;
    lower_tile(xcd_tile(blockIdx.x, tn * (tn + 1) / 2), &ti, &tj);
    const int64_t i0 = ti * MT, j0 = tj * MT;
    for (int e = tid; e < 65 * 4; e += 256) tab[e] = kTrigTab[e >> 2][e & 3];
    if (tid < 2 * MT) {  // the q chain of the tile's rows and columns, in the kernel build's order of operations
        const int64_t g = tid < MT ? i0 + tid : j0 + tid - MT;
        double q = g < a.n ? a.q[g] : 0.0;
#pragma unroll
        for (int l = 0; l < NLC; ++l) {
            if (l < nd) {
                qs[l][tid] = q;
                const double qp = fma(arch.w2[l], q, arch.b2[l]);
                rq[l][tid] = qp > 0.0 ? 1.0 / (4.0 * kPi * qp) : 0.0;
                if (l < nd - 1) q = arch.act[l] == NNGP_ACT_ABRELU ? arch.ap[l][2] * qp : 0.5 * qp;
            }
        }
    }

    // ---- Gram tile: rows i0 + tr + 16 p, columns j0 + tc + 16 q, features summed in order ----
    double (*s1)[MLD] = reinterpret_cast<double (*)[MLD]>(sm);
    double (*s2)[MLD] = reinterpret_cast<double (*)[MLD]>(sm + MT * MLD);
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    for (int k0 = 0; k0 < a.d; k0 += MKC) {
        const int kc = a.d - k0 < MKC ? a.d - k0 : MKC;
        for (int e = tid; e < MT * MKC; e += 256) {
            const int r = e / MKC, k = e % MKC;
            const int64_t i = i0 + r, j = j0 + r;
            s1[r][k] = (k < kc && i < a.n) ? a.x[i * a.d + k0 + k] : 0.0;
            s2[r][k] = (k < kc && j < a.n) ? a.x[j * a.d + k0 + k] : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            double u[4], v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) u[p] = s1[tr + 16 * p][k];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = s2[tc + 16 * q][k];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(u[p], v[q], acc[p][q]);
        }
        __syncthreads();
    }
    double (*gt)[MT + 1] = reinterpret_cast<double (*)[MT + 1]>(sm);
    const double inv_d = 1.0 / (double)a.d;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) gt[tr + 16 * p][tc + 16 * q] = acc[p][q] * inv_d;
    __syncthreads();

    // ---- per entry: forward recursion, then the adjoint sweep from both seeds ----
    double ga[2 * NLC], gi[2 * NLC];
#pragma unroll
    for (int c = 0; c < 2 * NLC; ++c) ga[c] = gi[c] = 0.0;
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const int ri = tr + 16 * (e >> 2), cj = tc + 16 * (e & 3);
        const int64_t i = i0 + ri, j = j0 + cj;
        if (i >= a.n || j > i) continue;  // padding, and the upper half of a diagonal tile (j <= i < n for every other entry)
        const bool dg = i == j;
        const double w = dg ? 1.0 : 2.0;  // the lower triangle stands for the whole square
        double kb_a = w * (a.alpha[i] * a.alpha[j]);
        double kb_i = w * a.ainv[i * a.ld + j];
        double k = dg ? qs[0][ri] : gt[ri][cj];  // exact diagonal: q q' - k^2 == 0 holds exactly
        double kin[NLC], ck[NLC], cs[NLC];  // per layer: k into Dense l; dK'/dk and (b - a)^2 s of the activation after it
#pragma unroll
        for (int l = 0; l < NLC; ++l) {
            kin[l] = k;
            ck[l] = 0.0;
            cs[l] = 0.0;
            if (l < nd - 1) {
                const double v = arch.w2[l], c = arch.b2[l];
                const bool ab = arch.act[l] == NNGP_ACT_ABRELU;
                k = fma(v, k, c);
                if (dg) {  // theta = 0: K' = (a^2 + b^2) / 2 k  (1/2 for ReLU), no q dependence
                    const double kd = ab ? arch.ap[l][2] : 0.5;
                    k *= kd;
                    ck[l] = kd;
                } else {
                    const double q1 = fma(v, qs[l][ri], c), q2 = fma(v, qs[l][MT + cj], c);
                    const double rr = fma(q1, q2, -k * k);
                    const double s = rr > 0.0 ? fast_sqrt_pos(rr > 0.0 ? rr : 1.0) : 0.0;
                    const double kr = pi_minus_atan2(s, k, tab) * (0.5 / kPi);  // kdot
                    const double kk = fma(kr, k, s * (0.5 / kPi));
                    if (ab) {
                        k = fma(arch.ap[l][0], k, arch.ap[l][1] * kk);
                        ck[l] = fma(arch.ap[l][1], kr, arch.ap[l][0]);
                        cs[l] = arch.ap[l][1] * s;
                    } else {
                        k = kk;
                        ck[l] = kr;
                        cs[l] = s;
                    }
                }
            }
        }
        double q1a = 0.0, q2a = 0.0, q1i = 0.0, q2i = 0.0;
#pragma unroll
        for (int l = NLC - 1; l >= 0; --l) {
            if (l < nd) {
                if (l < nd - 1) {  // the activation after Dense layer l: dK'/dq1 = (b - a)^2 s / (4 pi q1'), q' = h q
                    const double h = arch.act[l] == NNGP_ACT_ABRELU ? arch.ap[l][2] : 0.5;
                    const double t1 = cs[l] * rq[l][ri], t2 = cs[l] * rq[l][MT + cj];
                    q1a = fma(kb_a, t1, h * q1a);
                    q2a = fma(kb_a, t2, h * q2a);
                    kb_a *= ck[l];
                    q1i = fma(kb_i, t1, h * q1i);
                    q2i = fma(kb_i, t2, h * q2i);
                    kb_i *= ck[l];
                }
                // Dense layer l: k' = v k + c (likewise q1, q2)
                const double v = arch.w2[l], x1 = qs[l][ri], x2 = qs[l][MT + cj];
                ga[2 * l] += fma(kb_a, kin[l], fma(q1a, x1, q2a * x2));
                ga[2 * l + 1] += kb_a + q1a + q2a;
                gi[2 * l] += fma(kb_i, kin[l], fma(q1i, x1, q2i * x2));
                gi[2 * l + 1] += kb_i + q1i + q2i;
                kb_a *= v;
                q1a *= v;
                q2a *= v;
                kb_i *= v;
                q1i *= v;
                q2i *= v;
            }
        }
    }
    const int ncomp = 2 * nd;
#pragma unroll
    for (int c = 0; c < 2 * NLC; ++c) {
        if (c < ncomp) {  // uniform over the workgroup
            const double ra = block_sum(ga[c], red);
            const double rb = block_sum(gi[c], red);
            if (tid == 0) {
                a.part[(int64_t)c * a.nparts + blockIdx.x] = ra;
                a.part[(int64_t)(ncomp + c) * a.nparts + blockIdx.x] = rb;
            }
        }
    }
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
    double sq[NNGP_MAX_DENSE];
#pragma unroll
    for (int e = 0; e < NNGP_MAX_DENSE; ++e) sq[e] = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        double z = q[i];
#pragma unroll
        for (int e = 0; e < NNGP_MAX_DENSE; ++e) {
            if (e < nd) {
                sq[e] += z;
                const double zp = fma(arch.w2[e], z, arch.b2[e]);
                if (e < nd - 1) z = arch.act[e] == NNGP_ACT_ABRELU ? arch.ap[e][2] * zp : 0.5 * zp;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NNGP_MAX_DENSE; ++e) {
        if (e < nd) {
            const double r = block_sum(sq[e], red);
            if (threadIdx.x == 0) out[4 + e] = r;
        }
    }
    for (int c = 0; c < 4 * nd; ++c) {
        const double r = finish_part(part, nparts, c, red);
        if (threadIdx.x == 0) out[4 + nd + c] = r;
    }
}

int launch_mll_partial(const MllArgs& a, const ArchDev& arch, hipStream_t s) {
    NNGP_REQUIRE(a.nparts < 2147483647LL, "mll: gradient grid too large");
    const dim3 grid((unsigned)a.nparts), block(256);
    if (arch.n_dense <= 2) hipLaunchKernelGGL(k_nngp_mll_partial<2>, grid, block, 0, s, a, arch);
    else if (arch.n_dense <= 4) hipLaunchKernelGGL(k_nngp_mll_partial<4>, grid, block, 0, s, a, arch);
    else if (arch.n_dense <= 8) hipLaunchKernelGGL(k_nngp_mll_partial<8>, grid, block, 0, s, a, arch);
    else hipLaunchKernelGGL(k_nngp_mll_partial<NNGP_MAX_DENSE>, grid, block, 0, s, a, arch);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

}  // namespace nngp

using namespace nngp;

// ---------------------------------------------------------------------------------------------------------------------------
// C ABI (include/nngp_mll.h)

struct nngp_mll {
    GpWorkspace w;            // part: 2 kMaxComp per tile; red: [0, 2) tr K, r; [kRed, ...) k_mll_finish's sums
    double* q = nullptr;      // n_cap: |x_i|^2 / d
    int n_dense = 0;
    bool have_terms = false;
    double terms[2 * (kMaxComp + 1) + 5 + kMaxComp] = {};
    int n_terms = 0;
};

static void mll_free(nngp_mll* h) {
    dev_free(h->q);
    ws_free(&h->w);
}

extern "C" {

int nngp_mll_create(nngp_mll** out, int64_t n_cap, int32_t d) {
    NNGP_REQUIRE(out != nullptr && n_cap > 0 && d >= 1, "mll_create: bad arguments (n_cap=%lld, d=%d)", (long long)n_cap, d);
    *out = nullptr;
    nngp_mll* h = new (std::nothrow) nngp_mll();
    NNGP_REQUIRE(h != nullptr, "mll_create: out of host memory");
    int rc = dev_alloc(&h->q, n_cap);
    if (rc == 0) rc = ws_alloc(&h->w, n_cap, d, 2 * kMaxComp, kRed + 4 + NNGP_MAX_DENSE + 2 * kMaxComp, round_up(n_cap, TB));
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
    h->have_terms = false;
    NNGP_TRY(launch_row_sqnorm(x, n, h->w.d, h->q, s));  // from the caller's x: ws_set_train's synchronise covers it
    return ws_set_train(&h->w, x, y, hipMemcpyDeviceToDevice, n, s);
}

int nngp_mll_evaluate(nngp_mll* h, const nngp_arch_act* arch_in, double diag_reg, int32_t absolute, double* nlml, double* grad,
                      void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && arch_in != nullptr && nlml != nullptr, "mll_evaluate: NULL argument");
    NNGP_REQUIRE(h->w.n > 0, "mll_evaluate: no training data (nngp_mll_set_train)");
    ArchDev arch{};
    NNGP_TRY(make_arch_dev_act(arch_in, &arch));
    const int nd = arch.n_dense;
    for (int l = 0; l < nd; ++l) {
        const double w = arch_in->base.w_std[l], b = arch_in->base.b_std[l];
        NNGP_REQUIRE(std::isfinite(w) && std::isfinite(b) && w >= 0.0 && b >= 0.0,
                     "mll_evaluate: w_std / b_std of Dense layer %d must be finite and non-negative (%g, %g)", l, w, b);
    }
    for (int l = 0; l < nd - 1; ++l)
        NNGP_REQUIRE(arch.act[l] != NNGP_ACT_ERF, "mll_evaluate: hidden layer %d is Erf; the gradient covers ReLU and ABRelu only", l);
    NNGP_REQUIRE(std::isfinite(diag_reg) && diag_reg >= 0.0, "mll_evaluate: diag_reg must be finite and non-negative (%g)", diag_reg);
    GpWorkspace& w = h->w;
    w.factored = h->have_terms = false;
    const int64_t n = w.n, np = w.np;

    // A = K + r I: K by the kernel build (per-layer recursion: no_comp), the padding the identity
    BuildArgs b{};
    b.x1 = b.x2 = w.x;
    b.q1 = b.q2 = h->q;
    b.n1 = b.n2 = n;
    b.d = w.d;
    b.row_begin = 0;
    b.row_end = n;
    b.sym = 1;
    b.nngp64 = w.a;
    b.ld64 = np;
    b.no_comp = 1;
    NNGP_TRY(launch_kernel_build(b, arch, s));
    hipLaunchKernelGGL(k_mll_pad, dim3((unsigned)np), dim3(256), 0, s, w.a, np, n, np);
    hipLaunchKernelGGL(k_mll_diag, dim3(1), dim3(256), 0, s, w.a, np, n, diag_reg, (int)(absolute != 0), w.red);
    NNGP_HIP_CHECK(hipGetLastError());
    const bool want = grad != nullptr;
    NNGP_TRY(factor_and_solve(&w, want, "mll_evaluate", s));
    const int64_t nparts = gp_lower_tiles(n);
    if (want) {
        MllArgs ma{w.x, h->q, n, w.d, w.ainv, np, w.alpha, w.part, nparts};
        NNGP_TRY(launch_mll_partial(ma, arch, s));
    }
    hipLaunchKernelGGL(k_mll_finish, dim3(1), dim3(256), 0, s, w.a, np, n, w.wrow, want ? w.part : nullptr, nparts,
                       want ? w.alpha : nullptr, w.ainv, h->q, arch, w.red + kRed);
    NNGP_HIP_CHECK(hipGetLastError());
    double r[kRed + 4 + NNGP_MAX_DENSE + 2 * kMaxComp];
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
    // tr dK / dtheta from the diagonal's closed form: K_ii = u_{nd-1}, u_l = v_l z_l + c_l, z_{l+1} = h_l u_l, so
    // dK_ii / du_l = prod_{m >= l, hidden} h_m prod_{m > l} v_m =: D_l and tr dK/dv_l = D_l sum_i z_l,i, tr dK/dc_l = D_l N
    double trdk[kMaxComp];
    double dl = 1.0;
    for (int l = nd - 1; l >= 0; --l) {
        if (l < nd - 1) dl *= arch.act[l] == NNGP_ACT_ABRELU ? arch.ap[l][2] : 0.5;
        trdk[2 * l] = dl * sq[l];
        trdk[2 * l + 1] = dl * dn;
        dl *= arch.w2[l];
    }
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
    return 0;
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
