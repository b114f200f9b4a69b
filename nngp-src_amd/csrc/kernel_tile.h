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
