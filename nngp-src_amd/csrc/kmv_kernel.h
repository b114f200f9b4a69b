// The tile loop of the matrix-free operator (kmv_f64.hip has the description): the kernel template and its arguments.  The plain
// forms are instantiated by kmv_f64.hip and the additive forms by kmv_additive_f64.hip -- two translation units, so that the plain
// forms' code does not move with the additive ones beside them (the compiler's decisions for a kernel depend on what else its
// module holds: with all eight in one file the two general plain forms came out at 249 / 180 registers instead of 251 / 179).
#pragma once
#include "sparse_gp.h"
#include "kernel_tile.h"
#include "kmv_f64.h"

#include <type_traits>

namespace nngp {

struct KmvArgs {
    const double* x;
    const double* q;   // |x_i|^2 / d
    int64_t n;
    int d;
    const double* v;   // first vector of the pass
    int64_t ldv;
    int rc;            // live vectors of the pass (<= 16 RB); the others are zero in registers, never read
    double* part;      // [nsplit][nb][16 RB][64]
    int64_t nb;        // column blocks = row tiles
    int64_t per;       // row tiles per split
    int nsplit;
};
struct KmvAddArgs : KmvArgs {
    GroupsDev g;  // the additive form's group table
};

namespace {

constexpr int MKC = 16;        // k-chunk of the Gram product
constexpr int MLD = panel_ld(MKC);
constexpr int VLD = KT + 2;    // LDS row stride of the V tile: lanes (l16, lg) read word 2 l16 + lg -- distinct banks per half-wave

// ADD: the additive form (include/nngp_matfree_additive.h).  Per tile, before the Gram MFMA, the groups are walked as in
// k_build_add (group_walk of kernel_tile.h in the MFMA layout: a thread's 8 rows x 2 columns are the entries of its four
// accumulator blocks) and the sum is carried in registers; the whole-input map then takes it in with the build's last operation,
// fma(w0, k, sum).  The group map of 16 entries does not fit beside the output accumulators in 256 registers, so this form is
// built for one workgroup per compute unit and the whole unified register file.
template <int RB, bool GEN, bool ADD>
__global__ __launch_bounds__(256, ADD ? 1 : 2) void k_kmv_f64(std::conditional_t<ADD, KmvAddArgs, KmvArgs> a, ArchDev arch) {
    constexpr int W = 16 * RB;
    constexpr int RI = RB == 1 ? 4 : 2;  // entries of a block whose maps are evaluated side by side (the wide form has fewer registers to spare)
    __shared__ __attribute__((aligned(16))) double smem[2 * KT * MLD + W * VLD];  // As | Bs | Vs; the wave sums afterwards
    __shared__ __attribute__((aligned(16))) double tab[65 * 4];
    __shared__ double qs[GEN ? (NNGP_MAX_DENSE - 1) * 2 * KT : 1];  // stage_layer_q
    static_assert(RB * 1024 <= 2 * KT * MLD + W * VLD, "the wave sums alias the staging buffers");
    static_assert(!ADD || 2 * GKC * LDP <= 2 * KT * MLD, "the group walk stages in As | Bs while V stands in Vs");
    double* Vs = smem + 2 * KT * MLD;  // [W][VLD]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, lg = lane >> 4;

    // column block fast, split slow: the workgroups of one XCD walk the same row tiles at about the same time
    const int64_t g = xcd_tile(blockIdx.x, a.nb * a.nsplit);
    const int64_t cb = g % a.nb, sp = g / a.nb;
    const int64_t j0 = cb * KT, n = a.n;
    const int64_t t0 = sp * a.per, t1 = (t0 + a.per < a.nb) ? t0 + a.per : a.nb;
    for (int i = tid; i < 65 * 4; i += 256) tab[i] = kTrigTab[i >> 2][i & 3];

    f64x4 oacc[2][RB];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < RB; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[j][c][r] = 0.0;

    const double inv_d = 1.0 / (double)a.d;
    const int64_t wj0 = j0 + wn * 32;
    double q2in[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t gj = wj0 + j * 16 + l16;
        q2in[j] = gj < n ? a.q[gj] : 0.0;
    }

#pragma unroll 1
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t i0 = t * KT;
        // the V tile: vector c along the tile's rows (contiguous in memory); rows beyond n and vectors beyond rc are zero
#pragma unroll 4
        for (int e = 0; e < W * KT / 256; ++e) {
            const int idx = tid + 256 * e;
            const int c = idx >> 6, row = idx & 63;
            const int64_t gi = i0 + row;
            Vs[c * VLD + row] = (c < a.rc && gi < n) ? a.v[(int64_t)c * a.ldv + gi] : 0.0;
        }
        if constexpr (GEN) {  // read after the k-loop's first barrier
            if (tid < 2 * KT) {
                const int64_t gq = tid < KT ? i0 + tid : j0 + tid - KT;
                stage_layer_q(gq < n ? a.q[gq] : 0.0, arch, qs);
            }
        }

        // ---- the group sum of k_build_add (As | Bs are free; V and qs are staged beside them) ----
        [[maybe_unused]] double gs[8][2], w0;
        if constexpr (ADD) {
            w0 = a.g.full_weight;
#pragma unroll
            for (int e = 0; e < 8; ++e) gs[e][0] = gs[e][1] = 0.0;
            group_walk<false>(GroupLayMfma{}, PanelRows{a.x, i0, n}, PanelRows{a.x, j0, n}, a.d, a.g, arch, tab, smem,
                              [&](double wg, const double (&k)[8][2], const double (&)[8][2]) {
#pragma unroll
                                  for (int e = 0; e < 8; ++e)
#pragma unroll
                                      for (int j = 0; j < 2; ++j) gs[e][j] = fma(wg, k[e][j], gs[e][j]);
                              });
        }

        // ---- the Gram block of k_build_mfma<16, true, ...> ----
        f64x4 acc[2][2];
        if constexpr (!ADD) gram_mfma_64<MKC, true>(PanelRows{a.x, i0, n}, PanelRows{a.x, j0, n}, a.d, a.d, smem, acc);
        else if (w0 != 0.0) gram_mfma_64<MKC, true>(PanelRows{a.x, i0, n}, PanelRows{a.x, j0, n}, a.d, a.d, smem, acc);

        // ---- layer recursion in the accumulator layout, then the product: entry (row 16 i + lg + 4 r, col 16 j + l16) ----
        const int64_t wi0 = i0 + wm * 32;
        const bool diag_tile = t == cb && wm == wn;  // entries (i, i) exist only in these blocks
#pragma unroll 1
        for (int i = 0; i < 2; ++i) {
            double q1in[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gi = wi0 + i * 16 + lg + 4 * r;
                q1in[r] = gi < n ? a.q[gi] : 0.0;
            }
            double kv[2][4];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (ADD) {
                    if (w0 == 0.0) {  // no whole-input term: the group sum alone, inside the matrix
                        const bool in_col = wj0 + j * 16 + l16 < n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double sum = i == 0 ? gs[r][j] : gs[4 + r][j];
                            kv[j][r] = (in_col && wi0 + i * 16 + lg + 4 * r < n) ? sum : 0.0;
                        }
                        continue;
                    }
                }
                const f64x4 av = i == 0 ? acc[0][j] : acc[1][j];
                double q1v[4];
                bool dg[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    q1v[r] = q1in[r];
                    dg[r] = diag_tile && i == j && lg + 4 * r == l16;
                    kv[j][r] = dg[r] ? q1v[r] : av[r] * inv_d;  // exact diagonal: q q' - k^2 == 0 must hold exactly
                }
                // the build's maps without the NTK chain (tnone is never touched), RI entries side by side
                double tnone[4];
                if constexpr (GEN) {
                    const int row0 = wm * 32 + i * 16 + lg, col = KT + wn * 32 + j * 16 + l16;
                    gen_block_map<false, 0, RI>(arch, tab, qs, row0, col, kv[j], tnone, dg);
                    if constexpr (RI == 2) gen_block_map<false, 2, 2>(arch, tab, qs, row0, col, kv[j], tnone, dg);
                } else {
                    relu_block_map<false, 0, RI>(arch, true, tab, kv[j], tnone, q1v, q2in[j], dg);
                    if constexpr (RI == 2) relu_block_map<false, 2, 2>(arch, true, tab, kv[j], tnone, q1v, q2in[j], dg);
                }
                if constexpr (ADD) {  // the whole-input term last, as in k_build_add
#pragma unroll
                    for (int r = 0; r < 4; ++r) kv[j][r] = fma(w0, kv[j][r], i == 0 ? gs[r][j] : gs[4 + r][j]);
                }
                // entries outside the matrix take no part (their V is zero, but the map of a zero row need not be finite)
                const bool col_ok = wj0 + j * 16 + l16 < n;
#pragma unroll
                for (int r = 0; r < 4; ++r) kv[j][r] = (col_ok && wi0 + i * 16 + lg + 4 * r < n) ? kv[j][r] : 0.0;
            }
            // register r of block (i, j) is B[k = lg][col = l16] = K[wi0 + 16 i + 4 r + k][col]; A[c = l16][k = lg] from the V tile
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < RB; ++c) {
                    const double fv = Vs[(c * 16 + l16) * VLD + wm * 32 + i * 16 + 4 * r + lg];
#pragma unroll
                    for (int j = 0; j < 2; ++j) oacc[j][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fv, kv[j][r], oacc[j][c], 0, 0, 0);
                }
        }
        __syncthreads();  // Vs / qs are rewritten by the next tile
    }

    // ---- the two row halves of each column half, upper + lower, then the partial: OUT^T entry (c = 16 cb' + lg + 4 r, col l16) ----
    __syncthreads();
    double* red = smem;
    if (wm == 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < RB; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(((wn * 2 + j) * RB + c) * 4 + r) * 64 + lane] = oacc[j][c][r];
    }
    __syncthreads();
    if (wm == 0) {
        double* P = a.part + (sp * a.nb + cb) * (int64_t)(W * KT);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < RB; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    P[(c * 16 + lg + 4 * r) * KT + wn * 32 + j * 16 + l16] =
                        oacc[j][c][r] + red[(((wn * 2 + j) * RB + c) * 4 + r) * 64 + lane];
    }
}

}  // namespace

}  // namespace nngp
