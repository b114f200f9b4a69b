// Per-feature input relevances on the sparse NNGP and the derivative of its evidence with respect to every one of them
// (include/nngp_sparse_ard.h), all float64, on the handle of sparse_gp.hip and inside the evaluation of sparse_evidence.hip.
//
//   dK_ij/ds_k = (1/d) [ c_ij x_ik u_jk + e1_ij x_ik^2 + e2_ij u_jk^2 ]      over the rectangular block K(X_c o sqrt(s), U o sqrt(s))
// with c, e1, e2 the derivatives of the layer recursion with respect to its inputs K0_ij, q_i, q_j.  Seeded with S (beta gamma^T,
// or D_c = K_cu M'), (S o c)_ij =: kbar and the sums of S o e1 over j and of S o e2 over i are what the reverse sweep of rect_tile
// holds once it has passed Dense layer 0.  Per chunk:
//
//   k_sparse_rect_ard_partial   rect_tile with ARD set: the layer partials as ever, kbar of the dense seed in place over D_c (dead
//                               once read), kbar of the rank-one seed into a second buffer, and per tile the sums of qbar1 over its
//                               columns and of qbar2 over its rows, one slot per tile
//   k_sparse_ard_contract       the hot path, ard_contract_body of ard_contract.h (the body of k_ard_contract too) staged from the
//                               half's dense buffer: per 64-row block I of the chunk, 32 features and half, Z_I = sum_J kbar[I, J] U_J
//                               over all inducing tiles on the float64 MFMA with the RAW U, then sum_{i in I} x_ik (Z_ik + e1_i x_ik),
//                               rows in order, and sum_{i in I} x_ik^2
//   k_sparse_ard_finish         the row blocks summed in ascending order (ard_block_sum) and added to the accumulators, chunk after
//                               chunk; likewise e2_j += the chunk's row tiles in order
// and once per call: the symmetric half over K_uu (launch_ard_partial of nngp_ard.hip, k_nngp_ard_partial<NLC, false>, seeded with
// gamma and E, then launch_ard_contract with the raw U), and k_sparse_ard_cols, sum_j e2_j u_jk^2.  No float atomics, no
// device-side counter, no workgroup waits for another: launch boundaries are the only synchronisation, every slot has one writer
// and every sum a fixed order.
#include "ard_contract.h"
#include "sparse_rect.h"
#include "sparse_gp.h"
#include "../../include/nngp_sparse_ard.h"

namespace nngp {

namespace {

// xs = x o sqrt(s) on a precomputed sqrt(s): the arithmetic of k_ard_scale, one multiply per element (sqrt(s_k) = 1: the bits of x)
__global__ __launch_bounds__(256) void k_sparse_ard_scale(const double* x, const double* sq, int64_t total, int d, double* xs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) xs[e] = x[e] * sq[e % d];
}

template <int NLC>
__global__ __launch_bounds__(256) void k_sparse_rect_ard_partial(RectArgs a, ArchDev arch) {
    rect_tile<NLC, true>(a, arch);
}

// The rectangular form's staging: either half reads its own dense [c, ld] buffer, kb0 kbar of the rank-one and kb1 of the dense
// seed, every row block walking all tu inducing tiles; the B operand is the raw u.
struct RectStage {
    const double *cm, *b;
    int64_t ld, c, tu, nb;
    __device__ int64_t tiles(int64_t) const { return tu; }
    __device__ void stage(double (*ms)[MT + 1], int64_t i0, int64_t j0, int tid) const {
        for (int e = tid; e < MT * MT; e += 256) {
            const int r = e >> 6, cc = e & (MT - 1);
            const int64_t i = i0 + r, j = j0 + cc;
            ms[r][cc] = (i < c && j < nb) ? cm[i * ld + j] : 0.0;
        }
    }
};

// grid and part as ard_contract_body has them, with the chunk's tb row blocks and a half per seed.  x: [c, d] and u: [m, d] the
// raw rows; qrow: RectArgs::qrow.
__global__ __launch_bounds__(256) void k_sparse_ard_contract(const double* kb0, const double* kb1, int64_t ld, const double* x, int64_t c,
                                                             const double* u, int64_t m, int d, const double* qrow, int64_t cp,
                                                             int64_t tu, int64_t tb, double* part) {
    ard_contract_body(RectStage{blockIdx.z == 0 ? kb0 : kb1, u, ld, c, tu, m}, x, c, d, qrow, tu, cp, tb, part);
}

// acc[v * d + k] += sum over the chunk's row blocks, in order, of part[(v * tb + I) * d + k]   (v = 0, 1: the halves; 2: sum x_ik^2)
// e2[half * mpc + j] += sum over the chunk's row tiles, in order, of qcol[(half * tb + I) * mpc + j]     (j < m)
__global__ __launch_bounds__(256) void k_sparse_ard_finish(const double* part, int64_t tb, int d, const double* qcol, int64_t mpc,
                                                           int64_t m, double* acc, double* e2) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < 3 * (int64_t)d) {
        acc[e] += ard_block_sum(part, tb, d, e);
    } else if (e < 3 * (int64_t)d + 2 * m) {
        const int64_t f = e - 3 * (int64_t)d, hf = f / m, j = f % m;
        double t = 0.0;
        for (int64_t b = 0; b < tb; ++b) t += qcol[(hf * tb + b) * mpc + j];
        e2[hf * mpc + j] += t;
    }
}

// out[half * d + k] = sum_{j < m} e2[half * mpc + j] u_jk^2, rows in order (u: the raw inducing rows)
__global__ __launch_bounds__(256) void k_sparse_ard_cols(const double* e2, int64_t mpc, const double* u, int64_t m, int d, double* out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * d) return;
    const int hf = e / d, k = e % d;
    double t = 0.0;
    for (int64_t j = 0; j < m; ++j) {
        const double uv = u[j * d + k];
        t += e2[hf * mpc + j] * (uv * uv);
    }
    out[e] = t;
}

int launch_rect_ard(const RectArgs& a, const ArchDev& arch, hipStream_t s) {
    return launch_by_nlc(arch, a.nparts, "sparse_ard", [&](auto nlc, dim3 grid) {
        hipLaunchKernelGGL(k_sparse_rect_ard_partial<decltype(nlc)::value>, grid, dim3(256), 0, s, a, arch);
    });
}

// the rectangular pass with ARD set over one block, its contraction and the finish into acc [3 d] / e2 [2][mpc]
int rect_ard_block(const RectArgs& ra, const ArchDev& arch, const double* x_raw, const double* u_raw, double* part, double* acc, double* e2,
                   hipStream_t s) {
    NNGP_TRY(launch_rect_ard(ra, arch, s));
    const int d = ra.d;
    const dim3 grid((unsigned)ra.tr, (unsigned)((d + AKC - 1) / AKC), 2);
    hipLaunchKernelGGL(k_sparse_ard_contract, grid, dim3(256), 0, s, ra.kb_a, ra.kb_i, ra.ld, x_raw, ra.c, u_raw, ra.m, d, ra.qrow, ra.cp,
                       ra.tu, ra.tr, part);
    const int64_t count = 3 * (int64_t)d + 2 * ra.m;
    hipLaunchKernelGGL(k_sparse_ard_finish, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, part, ra.tr, d, ra.qcol, ra.mpc, ra.m,
                       acc, e2);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_cols(const double* e2, int64_t mpc, const double* u_raw, int64_t m, int d, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_sparse_ard_cols, dim3((unsigned)((2 * d + 255) / 256)), dim3(256), 0, s, e2, mpc, u_raw, m, d, out);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_scale(const double* x, const double* sq, int64_t rows, int d, double* out, hipStream_t s) {
    const int64_t total = rows * d;
    hipLaunchKernelGGL(k_sparse_ard_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, sq, total, d, out);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int sparse_ard_scale(const nngp_sparse* h, const double* x, int64_t rows, double* out, hipStream_t s) {
    return launch_scale(x, h->ard_s + h->d, rows, h->d, out, s);
}

int sparse_ard_begin(nngp_sparse* h, hipStream_t s) {
    NNGP_HIP_CHECK(hipMemsetAsync(h->ard_acc, 0, sizeof(double) * (8 * (int64_t)h->d + 2 * h->mp_cap), s));
    return 0;
}

int sparse_ard_uu(nngp_sparse* h, const double* seed, const double* gamma, double* cmat, hipStream_t s) {
    const int64_t m = h->m, mp = h->mp;
    const int d = h->d;
    MllArgs ma{h->u, h->uq, m, d, seed, mp, gamma, nullptr, h->ev_part, gp_lower_tiles(m), cmat, mp, h->ard_qbar, mp};
    NNGP_TRY(launch_ard_partial(ma, h->arch, false, s));
    return launch_ard_contract(cmat, mp, h->ard_u, m, d, h->ard_qbar, mp, h->ard_part, h->ard_acc + 5 * d, s);
}

int sparse_ard_chunk(nngp_sparse* h, const double* x_raw, const double* xs, int64_t c, const double* beta, const double* gamma,
                     hipStream_t s) {
    const int64_t m = h->m, mp = h->mp, tu = (m + MT - 1) / MT, tr = (c + MT - 1) / MT;
    RectArgs ra{xs, h->xq, c, h->u, h->uq, m, h->d, h->ev_d, mp, beta, gamma, h->ev_part, tr * tu, tu,
                h->ev_d, h->ard_kb, h->ard_qrow, h->chunk_rows, h->ard_qcol, tr, h->mp_cap};
    return rect_ard_block(ra, h->arch, x_raw, h->ard_u, h->ard_part, h->ard_acc, h->ard_acc + 8 * h->d, s);
}

int sparse_ard_end(nngp_sparse* h, hipStream_t s) {
    const int d = h->d;
    NNGP_TRY(launch_cols(h->ard_acc + 8 * d, h->mp_cap, h->ard_u, h->m, d, h->ard_acc + 3 * d, s));
    NNGP_HIP_CHECK(hipMemcpyAsync(h->ard_host.data(), h->ard_acc, sizeof(double) * 8 * d, hipMemcpyDeviceToHost, s));
    return 0;
}

void sparse_ard_finish_host(nngp_sparse* h, bool vfe, double s2, double ts, double bb, double gg, double* grad_s) {
    const int d = h->d;
    const double dn = (double)h->n, dm = (double)h->m, dd = (double)d, d0v0 = diag_q_slope(h->arch);
    const double* v = h->ard_host.data();
    double* t = h->ard_terms.data();
    for (int k = 0; k < d; ++k) {
        const double trdk_f = d0v0 * v[2 * d + k] / dd, trdk_u = d0v0 * v[7 * d + k] / dd;
        const double fu_q = (v[k] + v[3 * d + k]) / dd, fu_t = (v[d + k] + v[4 * d + k]) / dd;
        const double uu_q = v[5 * d + k] / dd, uu_t = v[6 * d + k] / dd;
        const double ds2 = h->absolute ? 0.0 : h->diag_reg * (trdk_f / dn);
        const double qa = 2.0 * fu_q - (uu_q + h->jitter / dm * trdk_u * gg) + bb * ds2;
        const double ta = 2.0 * fu_t + uu_t + ts * ds2 + (vfe ? trdk_f / s2 : 0.0);
        t[2 * k] = qa;
        t[2 * k + 1] = ta;
        t[2 * d + k] = trdk_f;
        t[3 * d + k] = trdk_u;
        grad_s[k] = -0.5 * qa + 0.5 * ta;
    }
    h->have_ard_terms = true;
}

int sparse_ard_full_reserve(nngp_sparse* h, int64_t cap, hipStream_t s) {
    if (cap <= h->ard_fcap) return 0;
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    dev_free(h->ard_fxs);
    h->ard_fcap = 0;
    NNGP_TRY(dev_alloc(&h->ard_fxs, cap * h->d));
    h->ard_fcap = cap;
    return 0;
}

void sparse_ard_free(nngp_sparse* h) {
    for (double** p : {&h->ard_s, &h->ard_u, &h->ard_xs, &h->ard_fxs, &h->ard_kb, &h->ard_qrow, &h->ard_qcol, &h->ard_qbar, &h->ard_part,
                       &h->ard_acc})
        dev_free(*p);
    h->ard_fcap = 0;
    h->ard_reserved = h->have_rel = h->have_ard_terms = false;
}

}  // namespace nngp

using namespace nngp;

extern "C" {

int nngp_sparse_reserve_ard(nngp_sparse* h) {
    NNGP_REQUIRE(h != nullptr, "sparse_reserve_ard: NULL argument");
    NNGP_REQUIRE(h->ev_reserved, "sparse_reserve_ard: the evidence was not reserved (nngp_sparse_reserve_evidence comes first)");
    if (h->ard_reserved) return 0;
    const int64_t d = h->d, mp = h->mp_cap, big = h->chunk_rows > h->test_cap ? h->chunk_rows : h->test_cap;
    const int64_t tu = (h->m_cap + MT - 1) / MT, tr = (h->chunk_rows + MT - 1) / MT, blocks = tu > tr ? tu : tr;
    int rc = dev_alloc(&h->ard_s, 2 * d);
    if (rc == 0) rc = dev_alloc(&h->ard_u, h->m_cap * d);
    if (rc == 0) rc = dev_alloc(&h->ard_xs, big * d);
    if (rc == 0) rc = dev_alloc(&h->ard_kb, h->chunk_rows * mp);
    if (rc == 0) rc = dev_alloc(&h->ard_qrow, 2 * tu * h->chunk_rows);
    if (rc == 0) rc = dev_alloc(&h->ard_qcol, 2 * tr * mp);
    if (rc == 0) rc = dev_alloc(&h->ard_qbar, 2 * tu * mp);
    if (rc == 0) rc = dev_alloc(&h->ard_part, 3 * blocks * d);
    if (rc == 0) rc = dev_alloc(&h->ard_acc, 8 * d + 2 * mp);
    if (rc != 0) {
        sparse_ard_free(h);
        return rc;
    }
    h->ard_host.assign((size_t)(8 * d), 0.0);
    h->ard_terms.assign((size_t)(4 * d), 0.0);
    h->ard_reserved = true;
    return 0;
}

int nngp_sparse_set_relevance(nngp_sparse* h, const double* s) {
    NNGP_REQUIRE(h != nullptr, "sparse_set_relevance: NULL argument");
    const int d = h->d;
    if (s != nullptr) {
        NNGP_REQUIRE(h->ard_reserved, "sparse_set_relevance: relevances need nngp_sparse_reserve_ard first");
        NNGP_TRY(check_relevances("sparse_set_relevance", s, d));
    }
    h->have_rel = h->have_ard_terms = false;
    sparse_drop_fit(h);
    if (s == nullptr) return 0;
    std::vector<double> both((size_t)(2 * d));
    for (int k = 0; k < d; ++k) {
        both[k] = s[k];
        both[d + k] = std::sqrt(s[k]);
    }
    NNGP_HIP_CHECK(hipDeviceSynchronize());  // earlier work may still read the old values
    NNGP_HIP_CHECK(hipMemcpy(h->ard_s, both.data(), sizeof(double) * 2 * d, hipMemcpyHostToDevice));
    h->have_rel = true;
    return 0;
}

int nngp_sparse_evidence_grad_ard(nngp_sparse* h, const double* x, const double* y, int64_t n, int32_t bound, double* nlml,
                                  double* grad, double* grad_s, void* stream) {
    NNGP_REQUIRE(h != nullptr && x != nullptr && y != nullptr && nlml != nullptr && grad_s != nullptr,
                 "sparse_evidence_grad_ard: NULL argument");
    return sparse_evidence_grad_core(h, x, y, n, bound, nlml, grad, grad_s, "sparse_evidence_grad_ard", (hipStream_t)stream);
}

int nngp_sparse_ard_terms(const nngp_sparse* h, double* out, int32_t count) {
    NNGP_REQUIRE(h != nullptr && out != nullptr, "sparse_ard_terms: NULL argument");
    NNGP_REQUIRE(h->have_ard_terms, "sparse_ard_terms: no evaluation with grad_s yet");
    const int n_terms = 4 * h->d;
    NNGP_REQUIRE(count >= n_terms, "sparse_ard_terms: count=%d, the last evaluation has %d terms", count, n_terms);
    for (int i = 0; i < n_terms; ++i) out[i] = h->ard_terms[i];
    return 0;
}

int nngp_sparse_ard_rect(const double* x, int64_t c, const double* u, int64_t m, int32_t d, const nngp_arch_act* arch,
                         const double* s_host, const double* seed, int64_t ld, const double* beta, const double* gamma, double* out,
                         void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(x != nullptr && u != nullptr && arch != nullptr && s_host != nullptr && seed != nullptr && beta != nullptr &&
                     gamma != nullptr && out != nullptr,
                 "sparse_ard_rect: NULL argument");
    NNGP_REQUIRE(c >= 1 && m >= 1 && d >= 1 && ld >= m, "sparse_ard_rect: need c, m, d >= 1 and ld >= m (c=%lld m=%lld d=%d ld=%lld)",
                 (long long)c, (long long)m, d, (long long)ld);
    NNGP_TRY(check_relevances("sparse_ard_rect", s_host, d));
    ArchDev ad{};
    NNGP_TRY(mll_make_arch(arch, 0.0, "sparse_ard_rect", &ad));
    const int64_t tu = (m + MT - 1) / MT, tr = (c + MT - 1) / MT, tiles = tr * tu, cp = tr * MT, mpc = tu * MT;
    const int64_t n4 = 4 * ad.n_dense, dd = d;
    std::vector<double> sq((size_t)d), res((size_t)(5 * dd));
    for (int k = 0; k < d; ++k) sq[k] = std::sqrt(s_host[k]);
    // kbi: the dense seed, then its kbar; kba: kbar of the rank-one seed; lpart: the layer partials; acc: the sums, then e2
    double *dsq, *xs, *us, *xq, *uq, *kbi, *kba, *qrow, *qcol, *lpart, *part, *acc;
    const auto work = [&]() -> int {
        NNGP_HIP_CHECK(hipMemcpyAsync(dsq, sq.data(), sizeof(double) * d, hipMemcpyHostToDevice, s));
        NNGP_TRY(launch_scale(x, dsq, c, d, xs, s));
        NNGP_TRY(launch_scale(u, dsq, m, d, us, s));
        NNGP_TRY(launch_row_sqnorm(xs, c, d, xq, s));
        NNGP_TRY(launch_row_sqnorm(us, m, d, uq, s));
        NNGP_HIP_CHECK(hipMemcpy2DAsync(kbi, sizeof(double) * m, seed, sizeof(double) * ld, sizeof(double) * m, (size_t)c,
                                        hipMemcpyDeviceToDevice, s));
        NNGP_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(double) * (8 * dd + 2 * mpc), s));
        RectArgs ra{xs, xq, c, us, uq, m, d, kbi, m, beta, gamma, lpart, tiles, tu, kbi, kba, qrow, cp, qcol, tr, mpc};
        NNGP_TRY(rect_ard_block(ra, ad, x, u, part, acc, acc + 8 * dd, s));
        NNGP_TRY(launch_cols(acc + 8 * dd, mpc, u, m, d, acc + 3 * dd, s));
        NNGP_HIP_CHECK(hipMemcpyAsync(res.data(), acc, sizeof(double) * 5 * dd, hipMemcpyDeviceToHost, s));
        return 0;
    };
    NNGP_TRY(with_stream_block(s, {{&dsq, dd}, {&xs, c * dd}, {&us, m * dd}, {&xq, c}, {&uq, m}, {&kbi, c * m}, {&kba, c * m},
                                   {&qrow, 2 * tu * cp}, {&qcol, 2 * tr * mpc}, {&lpart, n4 * tiles}, {&part, 3 * tr * dd},
                                   {&acc, 8 * dd + 2 * mpc}}, work));
    for (int k = 0; k < d; ++k) {
        out[k] = (res[k] + res[3 * dd + k]) / (double)d;
        out[d + k] = (res[dd + k] + res[4 * dd + k]) / (double)d;
    }
    return 0;
}

}  // extern "C"
