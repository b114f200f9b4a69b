// The matrix-free NNGP operator: OUT = (K(X, X) + diag_add I) V for a block of r vectors, K never written to memory.
//
//   k_kmv_f64      one workgroup owns a 64-column block of K and a contiguous range of 64-row tiles.  Per tile it calls the pieces
//                  of the kernel build (kernel_tile.h, the ones k_build_mfma of kernel_build.hip is made of: gram_mfma_64 stages
//                  the X panels through LDS in k-chunks of 16 and forms the Gram block on v_mfma_f64_16x16x4_f64; relu_block_map /
//                  gen_block_map run the layer recursion in the accumulator layout, without the NTK chain; stage_layer_q) and then
//                  multiplies the finished block into the vectors without moving it: the C/D layout of the float64 MFMA is
//                  col = lane & 15, row = (lane >> 4) + 4 reg, and its B operand is one value per lane at (k = lane >> 4,
//                  col = lane & 15), so register `reg` of a finished 16 x 16 block IS the operand B[k][j] = K[4 reg + k][j].  With
//                  A[c][k] = V[c][i0 + 4 reg + k] (the V tile staged through LDS: the lanes of that operand read 16 different
//                  vectors) the second MFMA accumulates OUT^T[c, j] += sum_i V[c, i] K[i, j] -- row block i's contribution to the
//                  output rows of COLUMN block j, the whole product because K is symmetric.
//                  The two waves that share a column half are summed through LDS (upper rows + lower rows, fixed), and the
//                  workgroup writes one partial [16 RB vectors][64 columns].
//   k_kmv_reduce   OUT[c, j] = sum over the row splits in ascending order + diag_add V[c, j].
// No atomics, no counters, no cooperative launch: the launch boundary is the only synchronisation (as in k_syrk_tn_f64).  The
// split is a function of n alone, each vector's sums never see another vector (one MFMA output column each), so a vector's result
// does not depend on r, on its position in the block or on the pass width, and two calls give the same bytes.
#include "sparse_gp.h"
#include "kernel_tile.h"
#include "kmv_f64.h"

#include <cmath>

namespace nngp {

namespace {

constexpr int MKC = 16;        // k-chunk of the Gram product
constexpr int MLD = panel_ld(MKC);
constexpr int VLD = KT + 2;    // LDS row stride of the V tile: lanes (l16, lg) read word 2 l16 + lg -- distinct banks per half-wave
constexpr int kKmvTargetGroups = 2048;  // workgroups wanted when the column blocks alone are fewer

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

template <int RB, bool GEN>
__global__ __launch_bounds__(256, 2) void k_kmv_f64(KmvArgs a, ArchDev arch) {
    constexpr int W = 16 * RB;
    constexpr int RI = RB == 1 ? 4 : 2;  // entries of a block whose maps are evaluated side by side (the wide form has fewer registers to spare)
    __shared__ __attribute__((aligned(16))) double smem[2 * KT * MLD + W * VLD];  // As | Bs | Vs; the wave sums afterwards
    __shared__ __attribute__((aligned(16))) double tab[65 * 4];
    __shared__ double qs[GEN ? (NNGP_MAX_DENSE - 1) * 2 * KT : 1];  // stage_layer_q
    static_assert(RB * 1024 <= 2 * KT * MLD + W * VLD, "the wave sums alias the staging buffers");
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

        // ---- the Gram block of k_build_mfma<16, true, ...> ----
        f64x4 acc[2][2];
        gram_mfma_64<MKC, true>(PanelRows{a.x, i0, n}, PanelRows{a.x, j0, n}, a.d, a.d, smem, acc);

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

// one workgroup per column block: OUT[c, j] = sum over the splits, ascending, + diag_add V[c, j]
__global__ __launch_bounds__(256) void k_kmv_reduce(double* __restrict__ out, int64_t ldo, const double* __restrict__ v, int64_t ldv,
                                                    int rc, int w, int64_t n, int64_t nb, int nsplit, const double* __restrict__ part,
                                                    double diag_add) {
    const int64_t cb = blockIdx.x;
    for (int e = threadIdx.x; e < rc * KT; e += 256) {
        const int c = e >> 6, col = e & 63;
        const int64_t gj = cb * KT + col;
        if (gj >= n) continue;
        double s = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) s += part[(((int64_t)sp * nb + cb) * w + c) * KT + col];
        out[(int64_t)c * ldo + gj] = s + diag_add * v[(int64_t)c * ldv + gj];
    }
}

// the row tiles are cut into nsplit runs of `per`; a function of n alone
int kmv_splits(int64_t n, int64_t* per) {
    const int64_t nb = (n + KT - 1) / KT;
    int64_t want = (kKmvTargetGroups + nb - 1) / nb;
    if (want > nb) want = nb;
    *per = (nb + want - 1) / want;
    return (int)((nb + *per - 1) / *per);
}

}  // namespace

int64_t kmv_ws_doubles(int64_t n, int r) {
    int64_t per;
    const int64_t nb = (n + KT - 1) / KT, ns = kmv_splits(n, &per);
    return ns * nb * KT * (r > 16 ? 64 : 16);
}

int kmv_check(const double* out, int64_t ldo, const double* v, int64_t ldv, int r, const double* x, int64_t n, int d, const ArchDev& arch,
              double diag_add) {
    NNGP_REQUIRE(out != nullptr && v != nullptr && x != nullptr && out != v, "kmv_f64: NULL argument, or out aliases v");
    NNGP_REQUIRE(n >= 1 && n <= ((int64_t)1 << 26) && d >= 1 && r >= 1 && r <= 65536,
                 "kmv_f64: need 1 <= n <= 2^26, d >= 1 and 1 <= r <= 65536 (n=%lld, d=%d, r=%d)", (long long)n, d, r);
    NNGP_REQUIRE(ldo >= n && ldv >= n, "kmv_f64: leading dimensions must be >= n (ldo=%lld, ldv=%lld, n=%lld)", (long long)ldo,
                 (long long)ldv, (long long)n);
    NNGP_REQUIRE(std::isfinite(diag_add), "kmv_f64: diag_add must be finite");
    NNGP_REQUIRE(arch.groups == nullptr, "kmv_f64: additive kernels are not supported by the fused operator");
    return 0;
}

int launch_kmv_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int r, const double* x, const double* q, int64_t n, int d,
                   const ArchDev& arch, double diag_add, double* ws, int64_t ws_doubles, hipStream_t s) {
    NNGP_TRY(kmv_check(out, ldo, v, ldv, r, x, n, d, arch, diag_add));
    NNGP_REQUIRE(q != nullptr && ws != nullptr && ws_doubles >= kmv_ws_doubles(n, r), "kmv_f64: workspace missing or too small");
    KmvArgs a{};
    a.x = x;
    a.q = q;
    a.n = n;
    a.d = d;
    a.ldv = ldv;
    a.part = ws;
    a.nb = (n + KT - 1) / KT;
    a.nsplit = kmv_splits(n, &a.per);
    const unsigned grid = (unsigned)(a.nb * a.nsplit);
    // passes of 64 vectors while more than 16 remain, one of 16 for a short tail: each pass builds K once
    for (int c0 = 0; c0 < r;) {
        const int rem = r - c0, w = rem > 16 ? 64 : 16;
        a.v = v + (int64_t)c0 * ldv;
        a.rc = rem < w ? rem : w;
        if (w == 64) {
            if (arch.general) hipLaunchKernelGGL((k_kmv_f64<4, true>), dim3(grid), dim3(256), 0, s, a, arch);
            else hipLaunchKernelGGL((k_kmv_f64<4, false>), dim3(grid), dim3(256), 0, s, a, arch);
        } else {
            if (arch.general) hipLaunchKernelGGL((k_kmv_f64<1, true>), dim3(grid), dim3(256), 0, s, a, arch);
            else hipLaunchKernelGGL((k_kmv_f64<1, false>), dim3(grid), dim3(256), 0, s, a, arch);
        }
        hipLaunchKernelGGL(k_kmv_reduce, dim3((unsigned)a.nb), dim3(256), 0, s, out + (int64_t)c0 * ldo, ldo, a.v, ldv, a.rc, w, n, a.nb,
                           a.nsplit, a.part, diag_add);
        NNGP_HIP_CHECK(hipGetLastError());
        c0 += a.rc;
    }
    return 0;
}

}  // namespace nngp

using namespace nngp;

extern "C" int nngp_kmv_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int32_t r, const double* x, int64_t n, int32_t d,
                            const nngp_arch_act* arch, double diag_add, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    NNGP_TRY(kmv_check(out, ldo, v, ldv, r, x, n, d, ad, diag_add));
    const int64_t wsd = kmv_ws_doubles(n, r);
    double* q = nullptr;
    double* ws = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&q), sizeof(double) * (size_t)n, s));
    if (hipMallocAsync(reinterpret_cast<void**>(&ws), sizeof(double) * (size_t)wsd, s) != hipSuccess) {
        (void)hipFreeAsync(q, s);
        set_error("kmv_f64: no room for %lld doubles of partials", (long long)wsd);
        return -1;
    }
    int rc = launch_row_sqnorm(x, n, d, q, s);
    if (rc == 0) rc = launch_kmv_f64(out, ldo, v, ldv, r, x, q, n, d, ad, diag_add, ws, wsd, s);
    (void)hipFreeAsync(ws, s);
    (void)hipFreeAsync(q, s);
    return rc;
}
