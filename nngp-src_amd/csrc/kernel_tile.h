// The pieces of a forward kernel tile: the one copy of every stage that the kernel build (k_build_mfma, k_build of kernel_build.hip),
// the additive build (k_build_add of kernel_build_additive.hip) and the matrix-free operator (k_kmv_f64 of kmv_f64.hip) share.
// Each is called by the whole 256-thread workgroup of a 64 x 64 tile.  The LDS arrays belong to the kernel and come in by reference,
// the per-entry state by reference to register arrays; nothing here declares __shared__.  The order of every floating-point
// operation is fixed here: the exact-diagonal rule, the rr > 0 guard and the pi_minus_atan2 call exist once for the whole family.
//
//   MFMA layout (gram_mfma_64, stage_layer_q, relu_block_map, gen_block_map): 4 waves, wave (wm, wn) = (wave >> 1, wave & 1) owns
//   the 32 x 32 block at (32 wm, 32 wn) as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64; register r of block (i, j) is the entry
//   (row 16 i + lg + 4 r, col 16 j + l16), l16 = lane & 15, lg = lane >> 4.
//   4 x 4 layout (tile_store_4x4, tile_mirror_4x4): thread (tx, ty) = (tid & 15, tid >> 4) holds rows ty + 16 r, columns 4 tx + c.
//   The group terms of the additive kernel (group_walk, group_map, affine_lo, erf_cross_comp) run in either layout: k_build_add in
//   the 4 x 4 one, the additive form of k_kmv_f64 in the MFMA one.
#pragma once
#include "gp_f64.h"
#include "trig_tab.h"
#include "f64_math.h"
#include "act_map.h"

namespace nngp {

constexpr int KT = 64;       // output tile edge
constexpr int LDP = KT + 2;  // LDS row stride of the 4 x 4 layout's tile in doubles (keeps 16-byte alignment of every row)
typedef double f64x4 __attribute__((ext_vector_type(4)));
// LDS row stride (doubles) of an X panel staged in k-chunks of mkc: rows 16-byte aligned, quarter-waves on distinct banks
constexpr int panel_ld(int mkc) { return mkc + 2; }

struct PanelRows {
    const double* p;  // [., d]
    int64_t r0;       // the tile's first row
    int64_t end;      // rows from end on read as zero
};

// The Gram block of the tile: acc = sum_k A[row][k] B[col][k] over k < k_limit (the caller divides by d).  The row panels are
// staged through LDS (smem: As | Bs, [KT][MKC + 2] each) in k-chunks of MKC, ROW-major with a 2-double pad: stores run along k
// without bank conflicts, and a lane reads the two k values it feeds to two consecutive MFMAs with one 16-byte read.
// PREFETCH: the next chunk's global loads are issued into registers before the MFMAs of the current one.  Ends with a barrier:
// the caller may reuse smem at once.
template <int MKC, bool PREFETCH, int NS>
__device__ __forceinline__ void gram_mfma_64(const PanelRows& pa, const PanelRows& pb, int d, int k_limit, double (&smem)[NS],
                                             f64x4 (&acc)[2][2]) {
    constexpr int MLD = panel_ld(MKC);
    constexpr int NLD = MKC * 64 / 256;  // doubles per thread and operand per chunk
    static_assert(2 * KT * MLD <= NS, "As | Bs");
    double* As = smem;             // [KT][MLD]
    double* Bs = smem + KT * MLD;  // [KT][MLD]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;

    double ra[NLD], rb[NLD];
    auto load_chunk = [&](int k0) {  // 64 rows x MKC k per operand, lanes along k
#pragma unroll
        for (int e = 0; e < NLD; ++e) {
            const int idx = tid + 256 * e;
            const int kk = idx & (MKC - 1), row = idx / MKC;
            const int kg = k0 + kk;
            const int64_t gi = pa.r0 + row, gj = pb.r0 + row;
            ra[e] = (kg < d && gi < pa.end) ? pa.p[gi * d + kg] : 0.0;
            rb[e] = (kg < d && gj < pb.end) ? pb.p[gj * d + kg] : 0.0;
        }
    };
    if (PREFETCH) load_chunk(0);
    for (int k0 = 0; k0 < k_limit; k0 += MKC) {
        if (!PREFETCH) load_chunk(k0);
#pragma unroll
        for (int e = 0; e < NLD; ++e) {
            const int idx = tid + 256 * e;
            const int kk = idx & (MKC - 1), row = idx / MKC;
            As[row * MLD + kk] = ra[e];
            Bs[row * MLD + kk] = rb[e];
        }
        __syncthreads();
        if (PREFETCH && k0 + MKC < d) load_chunk(k0 + MKC);
#pragma unroll
        for (int ks = 0; ks < MKC / 8; ++ks) {
            double2 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const double2*>(&As[(wm * 32 + i * 16 + l16) * MLD + ks * 8 + 2 * lg]);
                fb[i] = *reinterpret_cast<const double2*>(&Bs[(wn * 32 + i * 16 + l16) * MLD + ks * 8 + 2 * lg]);
            }
            // lane group g supplies k = 8 ks + 2 g (first MFMA) and 8 ks + 2 g + 1 (second): the sum over k does not care
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
                }
        }
        __syncthreads();
    }
}

// The other activations: the q of one of the tile's rows (tid < KT) or columns (KT <= tid < 2 KT) after each Dense layer,
// qs[layer][64 rows | 64 columns], before the activation -- once per tile instead of once per entry.  Called by threads < 2 KT
// with their q = |x|^2 / d; read after the next barrier.
template <int NQ>
__device__ __forceinline__ void stage_layer_q(double q, const ArchDev& arch, double (&qs)[NQ]) {
    static_assert(NQ == (NNGP_MAX_DENSE - 1) * 2 * KT, "qs[layer][2 KT]");
    const int tid = threadIdx.x;
    for (int l = 0; l < arch.n_dense - 1; ++l) {
        double unused;
        q = fma(arch.w2[l], q, arch.b2[l]);
        qs[l * 2 * KT + tid] = q;
        act_diag(arch.act[l], arch.ap[l], q, &kTrigTab[0][0], q, unused);
    }
}

// Entries r in [R0, R0 + RN) of one 16 x 16 accumulator block through Dense, (Relu, Dense)*: kv = the normalised Gram entries (q
// itself where dg: q q' - k^2 == 0 must hold exactly), q1v / q2v the rows' / the column's q, tv = 0 on entry.  dg: entry (i, i)
// of a symmetric tile, theta = 0 exactly.  relu_on = false: the Dense layers alone (a timing ablation).  NTK = false: no t chain
// (tv is not touched).  Arch: ArchDev or its all-ReLU head.
template <bool NTK, int R0, int RN, typename Arch>
__device__ __forceinline__ void relu_block_map(const Arch& arch, bool relu_on, const double (&tab)[65 * 4], double (&kv)[4],
                                               double (&tv)[4], double (&q1v)[4], double q2v, const bool (&dg)[4]) {
    for (int l = 0; l < arch.n_dense; ++l) {
        const double w2 = arch.w2[l], b2 = arch.b2[l];
        const bool relu = l < arch.n_dense - 1 && relu_on;
        q2v = fma(w2, q2v, b2);
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            q1v[r] = fma(w2, q1v[r], b2);
            double k = fma(w2, kv[r], b2);
            [[maybe_unused]] double t = NTK ? fma(w2, tv[r], k) : 0.0;
            if (relu) {
                const double rr = dg[r] ? 0.0 : fma(q1v[r], q2v, -k * k);
                const double s = rr > 0.0 ? fast_sqrt_pos(rr > 0.0 ? rr : 1.0) : 0.0;
                double kd = pi_minus_atan2(s, k, tab) * (0.5 / kPi);
                kd = dg[r] ? 0.5 : kd;  // theta = 0 on the diagonal, exactly
                k = fma(kd, k, s * (0.5 / kPi));
                if (NTK) t *= kd;
            }
            kv[r] = k;
            if (NTK) tv[r] = t;
            q1v[r] *= 0.5;
        }
        q2v *= 0.5;
    }
}

// The same for the other activations (act_cross / act_diag of act_map.h).  The rows' and the column's q come from qs
// (stage_layer_q): row0 = the block's row of entry 0 within the tile (entry r: row0 + 4 r), col = KT + its column.
template <bool NTK, int R0, int RN, int NQ>
__device__ __forceinline__ void gen_block_map(const ArchDev& arch, const double (&tab)[65 * 4], const double (&qs)[NQ], int row0,
                                              int col, double (&kv)[4], double (&tv)[4], const bool (&dg)[4]) {
    for (int l = 0; l < arch.n_dense; ++l) {
        const double w2 = arch.w2[l], b2 = arch.b2[l];
        const bool hidden = l < arch.n_dense - 1;
        const int code = hidden ? arch.act[l] : NNGP_ACT_RELU;
        const double* ap = arch.ap[hidden ? l : 0];
        const double q2l = hidden ? qs[l * 2 * KT + col] : 0.0;
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            double k = fma(w2, kv[r], b2);
            [[maybe_unused]] double t = NTK ? fma(w2, tv[r], k) : 0.0;
            if (hidden) {
                double kd;
                if (dg[r]) act_diag(code, ap, k, tab, k, kd);  // theta = 0 exactly, as in diag_chain_act
                else act_cross(code, ap, k, qs[l * 2 * KT + row0 + 4 * r], q2l, tab, k, kd);
                if (NTK) t *= kd;
            }
            kv[r] = k;
            if (NTK) tv[r] = t;
        }
    }
}

// One diagonal entry through Dense, (act, Dense)* at theta = 0: k = q on entry, t = 0.
__device__ __forceinline__ void diag_chain_act(const ArchDev& arch, const double* __restrict__ tab, double& k, double& t) {
    for (int l = 0; l < arch.n_dense; ++l) {
        k = fma(arch.w2[l], k, arch.b2[l]);
        t = fma(arch.w2[l], t, k);
        if (l < arch.n_dense - 1) {
            double kd;
            act_diag(arch.act[l], arch.ap[l], k, tab, k, kd);
            t *= kd;
        }
    }
}

// ---- the group terms of an additive kernel (include/nngp_additive.h): k_build_add and the additive form of k_kmv_f64 ----
constexpr int GKC = 8;  // features of a group staged per step

// lo with hi + lo = w2 * x + b2 to twice the working precision, for hi = fma(w2, x, b2): the product's and the sum's rounding
// errors, exactly (two-product by fma, two-sum), plus what the fma's single rounding left of them.
__device__ __forceinline__ double affine_lo(double w2, double x, double b2, double hi) {
    const double p = w2 * x, ep = fma(w2, x, -p);
    const double s = p + b2, bb = s - p;
    const double es = (p - (s - bb)) + (b2 - bb);
    return (s - hi) + (ep + es);
}

// act_cross of an Erf layer (act_map.h) with the bracket q1 q2 - k^2 taken from k, q1, q2 as hi + lo pairs.  A group's slices are
// nearly parallel far more often than whole rows are, and then r = 1 + 2 b^2 (q1 + q2) + 4 b^4 (q1 q2 - k^2) is left with
// r ~ 4 b^2 q while one rounding of the Dense layer's affine map is worth 4 b^4 u q^2 of it: at raw forest norms (q ~ 6e5) that is
// 5e-11 of Theta.  The first-order terms of the lo parts remove it (the operations on the hi parts are act_cross's own).
__device__ __forceinline__ void erf_cross_comp(const double* ap, double k, double kl, double q1, double q1l, double q2, double q2l,
                                               const double* __restrict__ tab, double& ko, double& kd) {
    const double kk = k * k;
    const double lo = fma(q1, q2l, fma(q2, q1l, -2.0 * (k * kl)));
    const double br = fmax((fma(q1, q2, -kk) + fma(-k, k, kk)) + lo, 0.0);
    const double w = fast_sqrt_pos(fma(ap[1] * ap[1], br, fma(ap[1], q1 + q2, 1.0)));
    ko = fma(ap[0], pi_minus_atan2(w, ap[1] * k, tab) - 0.5 * kPi, ap[2]);
    kd = ap[3] * fast_rcp(w);
}

// A thread's NR x NC entries of the tile in the group walk, and how it reads its rows' / columns' values of one staged feature
// (As / Bs: that feature's 64 rows / columns).  The 4 x 4 layout of the additive build:
struct GroupLay4x4 {
    static constexpr int NR = 4, NC = 4;
    __device__ __forceinline__ void rows(const double* As, double (&av)[4]) const {
        const int ty = threadIdx.x >> 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = As[ty + 16 * r];
    }
    __device__ __forceinline__ void cols(const double* Bs, double (&bv)[4]) const {
        const int tx = threadIdx.x & 15;
        const double2 b01 = *reinterpret_cast<const double2*>(&Bs[tx * 4]);
        const double2 b23 = *reinterpret_cast<const double2*>(&Bs[tx * 4 + 2]);
        bv[0] = b01.x; bv[1] = b01.y; bv[2] = b23.x; bv[3] = b23.y;
    }
};
// The MFMA layout: row 4 i + r of the thread is register r of its blocks (i, .), column j the column of its blocks (., j).
struct GroupLayMfma {
    static constexpr int NR = 8, NC = 2;
    __device__ __forceinline__ void rows(const double* As, double (&av)[8]) const {
        const int wm = threadIdx.x >> 7, lg = (threadIdx.x & 63) >> 4;
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = As[wm * 32 + (e >> 2) * 16 + lg + 4 * (e & 3)];
    }
    __device__ __forceinline__ void cols(const double* Bs, double (&bv)[2]) const {
        const int wn = (threadIdx.x >> 6) & 1, l16 = threadIdx.x & 15;
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[j] = Bs[wn * 32 + j * 16 + l16];
    }
};

// One group's term of a thread's NR x NC entries through Dense, (act, Dense)*: k[r][c] the Gram entries, q1[r] / q2[c] the diagonal
// entries of its rows / columns, all already normalised.  The layers are the outer loop, so a layer's map of the NR + NC diagonal
// entries runs once per thread and not once per entry.  same: k == q1 == q2 bit for bit (identical slices) -- the diagonal form.
template <bool NTK, int NR, int NC>
__device__ __forceinline__ void group_map(double (&k)[NR][NC], double (&q1)[NR], double (&q2)[NC], const ArchDev& arch,
                                          const double* __restrict__ tab, double (&t)[NR][NC]) {
    bool same[NR][NC];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            same[r][c] = (q1[r] == k[r][c]) && (q2[c] == k[r][c]);
            t[r][c] = 0.0;
        }
    for (int l = 0; l < arch.n_dense; ++l) {
        const double w2 = arch.w2[l], b2 = arch.b2[l];
        const bool hidden = l < arch.n_dense - 1;
        const int code = hidden ? arch.act[l] : NNGP_ACT_RELU;
        const bool erf = hidden && code == NNGP_ACT_ERF;
        const double* ap = arch.ap[hidden ? l : 0];
        double q1l[NR], q2l[NC];
#pragma unroll
        for (int e = 0; e < NR; ++e) {
            const double a = q1[e];
            q1[e] = fma(w2, a, b2);
            q1l[e] = erf ? affine_lo(w2, a, b2, q1[e]) : 0.0;
        }
#pragma unroll
        for (int e = 0; e < NC; ++e) {
            const double b = q2[e];
            q2[e] = fma(w2, b, b2);
            q2l[e] = erf ? affine_lo(w2, b, b2, q2[e]) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double kk = fma(w2, k[r][c], b2);
                double tt = NTK ? fma(w2, t[r][c], kk) : 0.0;
                if (hidden) {
                    double kd;
                    if (same[r][c]) act_diag(code, ap, kk, tab, kk, kd);
                    else if (erf) erf_cross_comp(ap, kk, affine_lo(w2, k[r][c], b2, kk), q1[r], q1l[r], q2[c], q2l[c], tab, kk, kd);
                    else act_cross(code, ap, kk, q1[r], q2[c], tab, kk, kd);
                    tt *= kd;
                }
                k[r][c] = kk;
                t[r][c] = tt;
            }
        if (hidden) {
            double unused;
#pragma unroll
            for (int e = 0; e < NR; ++e) act_diag(code, ap, q1[e], tab, q1[e], unused);
#pragma unroll
            for (int e = 0; e < NC; ++e) act_diag(code, ap, q2[e], tab, q2[e], unused);
        }
    }
}

// The walk over the groups of the table, in its order, for the tile of row panel pa and column panel pb.  The (group, k-chunk)
// steps form one flat sequence; the slices are staged through LDS (smem: As | Bs, [GKC][LDP] each) and the global loads of step
// s + 1 are issued into registers before step s is consumed, so their latency hides behind the FMAs and the layer map of the group
// that has just ended.  A group's Gram entries and its diagonal entries come from the same staged values by fma chains in feature
// order, times 1.0 / width.  At the end of each group sink(w_g, k, t) receives the thread's mapped entries (t: the NTK chain,
// meaningful with NTK).  Contains at least one barrier (the caller's LDS writes before the call are visible to what follows it)
// and ends with one: the caller may reuse smem at once.
template <bool NTK, typename Lay, int NS, typename Sink>
__device__ __forceinline__ void group_walk(const Lay& lay, const PanelRows& pa, const PanelRows& pb, int d, const GroupsDev& gr,
                                           const ArchDev& arch, const double* __restrict__ tab, double (&smem)[NS], Sink&& sink) {
    constexpr int NR = Lay::NR, NC = Lay::NC;
    static_assert(2 * GKC * LDP <= NS, "As | Bs");
    double* As = smem;              // [GKC][LDP]
    double* Bs = smem + GKC * LDP;  // [GKC][LDP]
    const int tid = threadIdx.x;
    double acc[NR][NC], qa[NR], qb[NC];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        qa[r] = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[r][c] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) qb[c] = 0.0;

    const int G = gr.n_groups;
    double ra[2], rb[2];
    auto load_chunk = [&](int k0, int k_end) {  // 64 rows x GKC features per operand; features past the group's end are zero
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 256 * e;
            const int kk = idx & (GKC - 1), row = idx >> 3;
            const int kg = k0 + kk;
            const int64_t gi = pa.r0 + row, gj = pb.r0 + row;
            ra[e] = (kg < k_end && gi < pa.end) ? pa.p[gi * d + kg] : 0.0;
            rb[e] = (kg < k_end && gj < pb.end) ? pb.p[gj * d + kg] : 0.0;
        }
    };
    int g = 0, k0 = 0, k_begin = 0, k_end = 0;
    if (G > 0) {
        k_begin = gr.begin[0];
        k_end = gr.end[0];
        k0 = k_begin;
        load_chunk(k0, k_end);
    } else {
        __syncthreads();
    }
    while (g < G) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 256 * e;
            const int kk = idx & (GKC - 1), row = idx >> 3;
            As[kk * LDP + row] = ra[e];
            Bs[kk * LDP + row] = rb[e];
        }
        __syncthreads();
        // the step after this one
        int ng = g, nk0 = k0 + GKC, nk_begin = k_begin, nk_end = k_end;
        if (nk0 >= k_end) {
            ng = g + 1;
            if (ng < G) {
                nk_begin = gr.begin[ng];
                nk_end = gr.end[ng];
                nk0 = nk_begin;
            }
        }
        if (ng < G) load_chunk(nk0, nk_end);
        const int kn = (k_end - k0) < GKC ? (k_end - k0) : GKC;
        for (int kk = 0; kk < kn; ++kk) {
            double av[NR], bv[NC];
            lay.rows(As + kk * LDP, av);
            lay.cols(Bs + kk * LDP, bv);
#pragma unroll
            for (int c = 0; c < NC; ++c) qb[c] = fma(bv[c], bv[c], qb[c]);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                qa[r] = fma(av[r], av[r], qa[r]);
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[r][c] = fma(av[r], bv[c], acc[r][c]);
            }
        }
        __syncthreads();
        if (ng != g) {  // the group is complete: its term of every entry
            const double inv_dg = 1.0 / (double)(k_end - k_begin);
            const double wg = gr.weight[g];
            double tv[NR][NC];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                qa[r] *= inv_dg;
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[r][c] *= inv_dg;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) qb[c] *= inv_dg;
            group_map<NTK>(acc, qa, qb, arch, tab, tv);
            sink(wg, acc, tv);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                qa[r] = 0.0;
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[r][c] = 0.0;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) qb[c] = 0.0;
        }
        g = ng; k0 = nk0; k_begin = nk_begin; k_end = nk_end;
    }
}

// ---- the 4 x 4-per-thread output block of k_build and k_build_add ----
template <typename T>
__device__ __forceinline__ void store4(T* base, int64_t ld, int64_t i, int64_t j, int64_t i_end, int64_t j_end,
                                       const double v[4], bool vec_ok) {
    if (base == nullptr || i >= i_end) return;
    T* p = base + i * ld + j;
    if (vec_ok && j + 3 < j_end) {
        if constexpr (sizeof(T) == 8) {
            reinterpret_cast<double2*>(p)[0] = make_double2(v[0], v[1]);
            reinterpret_cast<double2*>(p)[1] = make_double2(v[2], v[3]);
        } else {
            reinterpret_cast<float4*>(p)[0] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (j + c < j_end) p[c] = (T)v[c];
    }
}

// Row r of the tile at (i0, j0) from kn / kt: the float64 outputs, then the float32 copies (factorisation input) with the
// regulariser on the diagonal.  NTK = false: the Theta outputs are not wanted (kt is not read).
template <bool NTK>
__device__ __forceinline__ void tile_store_4x4(const BuildArgs& a, int64_t i0, int64_t j0, int r, const double (&kn)[4][4],
                                               const double (&kt)[4][4], bool vec) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t i_end = a.row_end, j_end = a.n2;
    const int64_t gi = i0 + ty + 16 * r, gj = j0 + tx * 4;
    store4(a.nngp64, a.ld64, gi, gj, i_end, j_end, kn[r], vec);
    if (NTK) store4(a.ntk64, a.ld64, gi, gj, i_end, j_end, kt[r], vec);
    if (a.nngp32 != nullptr || (NTK && a.ntk32 != nullptr)) {
        double vn[4], vt[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool diag = a.sym && gi == gj + c;
            vn[c] = kn[r][c] + (diag ? a.diag_add_nngp32 : 0.0);
            vt[c] = NTK ? kt[r][c] + (diag ? a.diag_add_ntk32 : 0.0) : 0.0;
        }
        store4(a.nngp32, a.ld32, gi, gj, i_end, j_end, vn, vec);
        if (NTK) store4(a.ntk32, a.ld32, gi, gj, i_end, j_end, vt, vec);
    }
}

// The mirror image of an off-diagonal tile of a symmetric build, transposed through LDS (smem: [KT][LDP]) and written with the same
// coalesced 16-byte stores; the float32 copies only without lower32.
template <bool NTK>
__device__ __forceinline__ void tile_mirror_4x4(const BuildArgs& a, int64_t i0, int64_t j0, double (&smem)[KT * LDP],
                                                const double (&kn)[4][4], const double (&kt)[4][4], bool vec) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t i_end = a.row_end, j_end = a.n2;
    for (int which = 0; which < (NTK ? 2 : 1); ++which) {
        if (which == 0 && a.nngp64 == nullptr && a.nngp32 == nullptr) continue;
        if (which == 1 && a.ntk64 == nullptr && a.ntk32 == nullptr) continue;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) smem[(tx * 4 + c) * LDP + ty + 16 * r] = which == 0 ? kn[r][c] : kt[r][c];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v[4];
            const double2 v01 = *reinterpret_cast<const double2*>(&smem[(ty + 16 * r) * LDP + tx * 4]);
            const double2 v23 = *reinterpret_cast<const double2*>(&smem[(ty + 16 * r) * LDP + tx * 4 + 2]);
            v[0] = v01.x; v[1] = v01.y; v[2] = v23.x; v[3] = v23.y;
            // element (j0 + ty + 16 r, i0 + tx * 4 + c); rows bounded by n2 (= n1), columns by row_end
            const int64_t mi = j0 + ty + 16 * r, mj = i0 + tx * 4;
            if (which == 0) {
                store4(a.nngp64, a.ld64, mi, mj, j_end, i_end, v, vec);
                if (!a.lower32) store4(a.nngp32, a.ld32, mi, mj, j_end, i_end, v, vec);
            } else {
                store4(a.ntk64, a.ld64, mi, mj, j_end, i_end, v, vec);
                if (!a.lower32) store4(a.ntk32, a.ld32, mi, mj, j_end, i_end, v, vec);
            }
        }
    }
}

}  // namespace nngp
