// The sparse (inducing-point, DTC) NNGP posterior (include/nngp_sparse.h), all float64.
//
// The pieces it shares with the exact float64 models: the kernel build (launch_kernel_build, rectangular and symmetric, with
// activations and groups), the blocked Cholesky and the right-side triangular solve of gp_f64.h.  New here:
//
//   k_syrk_tn_f64     the hot loop: C_lower += A^T A and, fused, R += A^T Y for a tall row-major A [rows, mp] -- the Gram matrix
//                     over the ROWS of A.  The contraction index is A's slow index, so a 16-row slab of two 128-column panels is
//                     copied to LDS as it lies in memory ([k][i], 16-byte loads along the rows) and the float64 MFMA's operands
//                     (lane l: A[i = l & 15][k = l >> 4]) are read from it with 8-byte reads: the 16 lanes of a k are 128
//                     contiguous bytes, and the row stride of 144 doubles puts the k + 1 lanes of the same 32-lane half on the
//                     other 32 banks, so the reads are conflict-free.  No transposed copy of A exists anywhere.
//                     128 x 128 tiles on or below the diagonal only, 4 waves of 64 x 64 (4 x 4 accumulators of
//                     v_mfma_f64_16x16x4_f64), double-buffered register staging as in gemm_f64.hip.  The tiles of block column 0
//                     also form their 128 rows of A^T Y (Y as a 16-column B operand, zero beyond ny).
//                     The rows are split over workgroups (few tiles, many rows): split s of tile t writes its partial tile to
//                     ws[s][t]; nothing is accumulated in place.
//   k_syrk_reduce     C = beta C + sum_s ws[s][t] in ascending s (and the same for R): fixed order, no atomics -- two runs give
//                     the same bits.  The launch boundary between the two kernels is the only synchronisation: no workgroup
//                     waits for another, there is no counter and no cooperative launch, so nothing here can hang.
//   k_sparse_*        the small passes of the model: jitter and padding of K_uu, the trace, B = sigma2 I + G, R^T, the predict finish.
// The handle itself is in sparse_gp.h: the model's evidence (sparse_evidence.hip) works on it too, and add_rows keeps the sums the
// evidence needs (y^T y, the per-layer sums of q) beside its own.
#include "sparse_gp.h"

#include <algorithm>
#include <vector>

namespace nngp {

namespace {

constexpr int ST = 128;            // tile edge
constexpr int SK = 16;             // rows of A per step
constexpr int SLD = 144;           // LDS row stride in doubles: 128 + 16, so that consecutive k fall on opposite bank halves
constexpr int SYMAX = 16;          // columns of Y (ny <= 16), one MFMA column block
constexpr int SPANEL = SK * SLD;   // doubles of one staged panel
constexpr int SSTAGE = 2 * SPANEL + SK * SYMAX;
constexpr size_t kSyrkLds = sizeof(double) * 2 * SSTAGE;  // 77 824 bytes: two workgroups per compute unit
constexpr int kSyrkMinSteps = 32;  // a split has at least 512 rows: its partial tile costs a write and a read of 128 KiB
constexpr int kSyrkTargetGroups = 2048;  // workgroups wanted when the tiles alone are fewer (8 per compute unit)
constexpr int kSyrkMaxSplits = 64;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct SyrkArgs {
    const double* a;
    int64_t lda;
    const double* y;   // NULL: no R
    int ny;
    int64_t rows;
    int mt;            // tiles per side
    int nsplit;
    int64_t split_rows;  // rows per split, a multiple of SK
    double* part;      // [nsplit][tiles][128 * 128]
    double* part_r;    // [nsplit][mp][SYMAX]
};

// rows are cut into nsplit pieces of split_rows (the last one shorter); depends on (rows, mp) only
int syrk_splits(int64_t rows, int64_t mp, int64_t* split_rows) {
    const int64_t mt = mp / ST, tiles = mt * (mt + 1) / 2;
    int64_t want = (kSyrkTargetGroups + tiles - 1) / tiles;
    if (want > kSyrkMaxSplits) want = kSyrkMaxSplits;
    const int64_t steps = (rows + SK - 1) / SK;
    int64_t per = (steps + want - 1) / want;
    if (per < kSyrkMinSteps) per = kSyrkMinSteps;
    *split_rows = per * SK;
    return (int)((steps + per - 1) / per);
}

__global__ __launch_bounds__(256, 2) void k_syrk_tn_f64(SyrkArgs p) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t tiles = (int64_t)p.mt * (p.mt + 1) / 2;
    // tile fast, split slow: the neighbours of one XCD's range share the row range and, along a tile row, the panel bi
    const int64_t g_ = xcd_tile(blockIdx.x, tiles * p.nsplit);
    const int64_t tile = g_ % tiles, sp = g_ / tiles;
    int64_t bi, bj;
    lower_tile(tile, &bi, &bj);
    const bool diag = bi == bj;
    const bool with_r = p.y != nullptr && bj == 0;
    const int64_t r0 = sp * p.split_rows;
    const int64_t r1 = (r0 + p.split_rows < p.rows) ? r0 + p.split_rows : p.rows;
    const int nk = (int)((r1 - r0 + SK - 1) / SK);
    const double* Ai = p.a + bi * ST;
    const double* Aj = p.a + bj * ST;

    f64x2 ga[4], gb[4];
    double gy = 0.0;
    const int ld_row = tid >> 6, ld_c2 = (tid & 63) * 2;  // 64 threads copy one row of a panel: 1 KiB contiguous
    const int y_row = tid >> 4, y_col = tid & 15;
    auto load_tile = [&](int t) {
        const int64_t k0 = r0 + (int64_t)t * SK;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = k0 + ld_row + 4 * e;
            const bool live = row < r1;  // the tail rows of the last step count as zero
            const f64x2 zero = {0.0, 0.0};
            ga[e] = live ? *reinterpret_cast<const f64x2*>(Ai + row * p.lda + ld_c2) : zero;
            if (!diag) gb[e] = live ? *reinterpret_cast<const f64x2*>(Aj + row * p.lda + ld_c2) : zero;
        }
        if (with_r) gy = (y_col < p.ny && k0 + y_row < r1) ? p.y[(k0 + y_row) * p.ny + y_col] : 0.0;
    };
    auto store_tile = [&](int buf) {
        double* sa_ = smem + buf * SSTAGE;
        double* sb_ = sa_ + SPANEL;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            *reinterpret_cast<f64x2*>(sa_ + (ld_row + 4 * e) * SLD + ld_c2) = ga[e];
            if (!diag) *reinterpret_cast<f64x2*>(sb_ + (ld_row + 4 * e) * SLD + ld_c2) = gb[e];
        }
        if (with_r) sa_[2 * SPANEL + y_row * SYMAX + y_col] = gy;
    };

    f64x4 acc[4][4], accr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) accr[i][r] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
    }

    const int r16 = lane & 15, g = lane >> 4;
    if (nk > 0) {
        load_tile(0);
        store_tile(0);
    }
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        if (t + 1 < nk) load_tile(t + 1);
        const double* sa_ = smem + (t & 1) * SSTAGE;
        const double* sb_ = diag ? sa_ : sa_ + SPANEL;
        const double* sy_ = sa_ + 2 * SPANEL;
#pragma unroll
        for (int s = 0; s < SK / 4; ++s) {
            const int k = 4 * s + g;
            double fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fa[i] = sa_[k * SLD + wm * 64 + i * 16 + r16];
                fb[i] = sb_[k * SLD + wn * 64 + i * 16 + r16];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
            if (with_r && wn == 0) {  // uniform over the wave
                const double fy = sy_[k * SYMAX + r16];
#pragma unroll
                for (int i = 0; i < 4; ++i) accr[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fy, accr[i], 0, 0, 0);
            }
        }
        if (t + 1 < nk) store_tile((t + 1) & 1);
        __syncthreads();
    }

    // C/D layout of the float64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
    double* P = p.part + (sp * tiles + tile) * (int64_t)(ST * ST);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(wm * 64 + i * 16 + g + 4 * r) * ST + wn * 64 + j * 16 + r16] = acc[i][j][r];
    if (with_r && wn == 0) {
        double* PR = p.part_r + (sp * p.mt + bi) * (int64_t)(ST * SYMAX);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) PR[(wm * 64 + i * 16 + g + 4 * r) * SYMAX + r16] = accr[i][r];
    }
}

// one workgroup per lower tile: C = beta C + sum over the splits, ascending; the tiles of block column 0 also reduce their rows of R
__global__ __launch_bounds__(256) void k_syrk_reduce(double* __restrict__ c, int64_t ldc, double* __restrict__ r, int ny, int mt,
                                                     int nsplit, const double* __restrict__ part, const double* __restrict__ part_r,
                                                     double beta) {
    const int64_t tiles = (int64_t)mt * (mt + 1) / 2;
    int64_t bi, bj;
    lower_tile(blockIdx.x, &bi, &bj);
    const double* p0 = part + (int64_t)blockIdx.x * (ST * ST);
    for (int e = threadIdx.x; e < ST * ST; e += 256) {
        double v = 0.0;
        for (int s = 0; s < nsplit; ++s) v += p0[(int64_t)s * tiles * (ST * ST) + e];
        double* out = c + (bi * ST + e / ST) * ldc + bj * ST + e % ST;
        *out = (beta != 0.0) ? beta * *out + v : v;
    }
    if (r == nullptr || bj != 0) return;
    for (int e = threadIdx.x; e < ST * ny; e += 256) {
        const int row = e / ny, col = e % ny;
        double v = 0.0;
        for (int s = 0; s < nsplit; ++s) v += part_r[(((int64_t)s * mt + bi) * ST + row) * SYMAX + col];
        double* out = r + (bi * ST + row) * ny + col;
        *out = (beta != 0.0) ? beta * *out + v : v;
    }
}

// ---- the model's small passes (one workgroup where a sum is involved: fixed order) ----

// K_uu [mp, mp] (zero outside [m, m]): scal[1] = jitter * trace / m, added to the diagonal; 1 on the padding diagonal
__global__ __launch_bounds__(256) void k_sparse_jitter(double* a, int64_t ld, int64_t m, int64_t mp, double jitter, double* scal) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) s += a[i * ld + i];
    const double add = jitter * (block_sum(s, red) / (double)m);
    for (int64_t i = threadIdx.x; i < mp; i += 256) a[i * ld + i] = i < m ? a[i * ld + i] + add : 1.0;
    if (threadIdx.x == 0) scal[1] = add;
}

// scal[0] += sum of the chunk's K(x_i, x_i)
__global__ __launch_bounds__(256) void k_sparse_trace(const double* kdiag, int64_t c, double* scal) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < c; i += 256) s += kdiag[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) scal[0] += s;
}

// scal[2] = sigma2 (workgroup 0 writes it; every workgroup computes the same value).  B = G + sigma2 I on the lower tiles; the
// tiles above the diagonal blocks, which the factorisation's trailing updates use as workspace, start from zero every time
__global__ __launch_bounds__(256) void k_sparse_b(const double* __restrict__ gm, double* __restrict__ b, int64_t mp, double diag_reg,
                                                  int absolute, double n, double* scal) {
    const double sigma2 = absolute ? diag_reg : diag_reg * (scal[0] / n);
    const int64_t mt = mp / ST, bi = blockIdx.x / mt, bj = blockIdx.x % mt;
    for (int e = threadIdx.x; e < ST * ST; e += 256) {
        const int64_t row = bi * ST + e / ST, col = bj * ST + e % ST;
        const double v = bj <= bi ? gm[row * mp + col] : 0.0;
        b[row * mp + col] = row == col ? v + sigma2 : v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[2] = sigma2;
}

// rt [128, mp] <- R^T [ny, mp], zero rows below
__global__ __launch_bounds__(256) void k_sparse_rt(const double* __restrict__ r, int ny, int64_t mp, double* __restrict__ rt) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y;
    if (k < mp) rt[row * mp + k] = row < ny ? r[k * ny + row] : 0.0;
}

// one workgroup per test row: mean[row, y] = q . C[:, y];  var[row] = kdiag[row] - |p|^2 + sigma2 |q|^2
__global__ __launch_bounds__(256) void k_sparse_predict_finish(const double* __restrict__ pm, const double* __restrict__ qm, int64_t mp,
                                                               const double* __restrict__ ct, int ny, const double* __restrict__ kdiag,
                                                               const double* __restrict__ scal, double* __restrict__ mean,
                                                               double* __restrict__ var) {
    __shared__ double red[256];
    const int64_t row = blockIdx.x;
    const double* pr = pm + row * mp;
    const double* qr = qm + row * mp;
    for (int y = 0; y < ny; ++y) {
        double s = 0.0;
        for (int64_t k = threadIdx.x; k < mp; k += 256) s += qr[k] * ct[(int64_t)y * mp + k];
        s = block_sum(s, red);
        if (threadIdx.x == 0) mean[row * ny + y] = s;
    }
    if (var == nullptr) return;
    double pp = 0.0, qq = 0.0;
    for (int64_t k = threadIdx.x; k < mp; k += 256) {
        pp += pr[k] * pr[k];
        qq += qr[k] * qr[k];
    }
    pp = block_sum(pp, red);
    qq = block_sum(qq, red);
    if (threadIdx.x == 0) var[row] = (kdiag[row] - pp) + scal[2] * qq;
}

}  // namespace

int64_t syrk_ws_doubles(int64_t rows, int64_t mp) {
    // the split count is not monotone in rows (it is a quotient rounded up), so size for its bound over 1 .. rows
    const int64_t mt = mp / ST, tiles = mt * (mt + 1) / 2;
    int64_t want = (kSyrkTargetGroups + tiles - 1) / tiles;
    if (want > kSyrkMaxSplits) want = kSyrkMaxSplits;
    const int64_t steps = (rows + SK - 1) / SK;
    int64_t most = (steps + kSyrkMinSteps - 1) / kSyrkMinSteps;
    if (most > want) most = want;
    if (most < 1) most = 1;
    return most * (tiles * (int64_t)(ST * ST) + mp * SYMAX);
}

int syrk_check(const double* c, int64_t ldc, const double* r, const double* a, int64_t lda, const double* y, int64_t rows, int64_t mp,
               int ny, double beta) {
    NNGP_REQUIRE(c != nullptr && a != nullptr && (r == nullptr || y != nullptr), "syrk_tn_f64: NULL argument");
    NNGP_REQUIRE(rows >= 1 && mp >= ST && mp % ST == 0 && mp <= 16384,
                 "syrk_tn_f64: need rows >= 1 and mp a multiple of %d up to 16384 (rows=%lld, mp=%lld)", ST, (long long)rows, (long long)mp);
    NNGP_REQUIRE(lda >= mp && lda % 2 == 0 && ((uintptr_t)a & 15) == 0 && ldc >= mp,
                 "syrk_tn_f64: need lda >= mp even, a 16-byte aligned and ldc >= mp (lda=%lld, ldc=%lld)", (long long)lda, (long long)ldc);
    NNGP_REQUIRE(r == nullptr || (ny >= 1 && ny <= SYMAX), "syrk_tn_f64: ny must be in 1 .. %d (ny=%d)", SYMAX, ny);
    NNGP_REQUIRE(std::isfinite(beta), "syrk_tn_f64: beta must be finite");
    return 0;
}

int launch_syrk_tn_f64(double* c, int64_t ldc, double* r, const double* a, int64_t lda, const double* y, int64_t rows, int64_t mp,
                       int ny, double beta, double* ws, int64_t ws_doubles, hipStream_t s) {
    NNGP_TRY(syrk_check(c, ldc, r, a, lda, y, rows, mp, ny, beta));
    NNGP_REQUIRE(ws != nullptr, "syrk_tn_f64: no workspace");
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_syrk_tn_f64), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSyrkLds);
    });
    NNGP_HIP_CHECK(attr);
    SyrkArgs p{};
    p.a = a;
    p.lda = lda;
    p.y = r ? y : nullptr;
    p.ny = ny;
    p.rows = rows;
    p.mt = (int)(mp / ST);
    p.nsplit = syrk_splits(rows, mp, &p.split_rows);
    const int64_t tiles = (int64_t)p.mt * (p.mt + 1) / 2;
    // the count is not monotone in mp (fewer tiles, more splits): a workspace sized for another mp may be too small for this one
    const int64_t need = (int64_t)p.nsplit * (tiles * (int64_t)(ST * ST) + mp * SYMAX);
    NNGP_REQUIRE(ws_doubles >= need, "syrk_tn_f64: the workspace holds %lld doubles, rows=%lld mp=%lld need %lld", (long long)ws_doubles,
                 (long long)rows, (long long)mp, (long long)need);
    p.part = ws;
    p.part_r = ws + (int64_t)p.nsplit * tiles * (ST * ST);
    hipLaunchKernelGGL(k_syrk_tn_f64, dim3((unsigned)(tiles * p.nsplit)), dim3(256), kSyrkLds, s, p);
    hipLaunchKernelGGL(k_syrk_reduce, dim3((unsigned)tiles), dim3(256), 0, s, c, ldc, r, ny, p.mt, p.nsplit, p.part, p.part_r, beta);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nngp

using namespace nngp;

// ---------------------------------------------------------------------------------------------------------------------------
// C ABI (include/nngp_sparse.h)

namespace {

void sparse_free(nngp_sparse* h) {
    for (double** p : {&h->u, &h->uq, &h->lu, &h->gm, &h->lb, &h->dinv_u, &h->dinv_b, &h->rm, &h->ct, &h->chunk, &h->pt, &h->qt, &h->xq,
                       &h->kd, &h->t, &h->ws, &h->scal, &h->fp, &h->fq, &h->fc, &h->fxq})
        dev_free(*p);
    sparse_evidence_free(h);
    dev_free(h->status);
    groups_destroy(&h->groups);
}

int sparse_alloc(nngp_sparse* h) {
    const int64_t mp = h->mp_cap, big = h->chunk_rows > h->test_cap ? h->chunk_rows : h->test_cap;
    NNGP_TRY(dev_alloc(&h->u, h->m_cap * h->d));
    NNGP_TRY(dev_alloc(&h->uq, h->m_cap));
    NNGP_TRY(dev_alloc(&h->lu, mp * mp));
    NNGP_TRY(dev_alloc(&h->gm, mp * mp));
    NNGP_TRY(dev_alloc(&h->lb, mp * mp));
    NNGP_TRY(dev_alloc(&h->dinv_u, mp * TB));
    NNGP_TRY(dev_alloc(&h->dinv_b, mp * TB));
    NNGP_TRY(dev_alloc(&h->rm, mp * h->ny));
    NNGP_TRY(dev_alloc(&h->ct, TB * mp));
    NNGP_TRY(dev_alloc(&h->chunk, h->chunk_rows * mp));
    NNGP_TRY(dev_alloc(&h->pt, h->test_cap * mp));
    NNGP_TRY(dev_alloc(&h->qt, h->test_cap * mp));
    NNGP_TRY(dev_alloc(&h->xq, big));
    NNGP_TRY(dev_alloc(&h->kd, big));
    NNGP_TRY(dev_alloc(&h->t, big * TB));
    h->t_rows = big;
    // set_inducing may choose any mp <= mp_cap, and a smaller mp can need more (fewer tiles, so more splits of each): the largest
    for (int64_t q = ST; q <= mp; q += ST) h->ws_doubles = std::max(h->ws_doubles, syrk_ws_doubles(h->chunk_rows, q));
    NNGP_TRY(dev_alloc(&h->ws, h->ws_doubles));
    NNGP_TRY(dev_alloc(&h->scal, kSpScal));
    NNGP_TRY(dev_alloc(&h->status, 1));
    NNGP_HIP_CHECK(hipMemset(h->scal, 0, sizeof(double) * kSpScal));
    return 0;
}

// timing study only (libnngp_hip_knobs.so, key 15 = 16 + mask): nngp_sparse_add_rows leaves out 1 = the cross build, 2 = the solve,
// 4 = the Gram kernel, so that each stage is timed on the handle's own path.  Wrong results; the constant 0 in the product library.
inline int sparse_skip() {
    const int k = NNGP_KNOB(15);
    return k >= 16 ? k - 16 : 0;
}

int sparse_full_reserve(nngp_sparse* h, int64_t mt, hipStream_t s) {
    const int64_t cap = round_up(mt, TB);
    if (cap <= h->full_cap) return 0;
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    dev_free(h->fp); dev_free(h->fq); dev_free(h->fc); dev_free(h->fxq);
    h->full_cap = 0;
    NNGP_TRY(dev_alloc(&h->fp, cap * h->mp_cap));
    NNGP_TRY(dev_alloc(&h->fq, cap * h->mp_cap));
    NNGP_TRY(dev_alloc(&h->fc, cap * cap));
    NNGP_TRY(dev_alloc(&h->fxq, cap));
    if (cap > h->t_rows) {
        dev_free(h->t);
        h->t_rows = 0;
        NNGP_TRY(dev_alloc(&h->t, cap * TB));
        h->t_rows = cap;
    }
    h->full_cap = cap;
    return 0;
}

}  // namespace

namespace nngp {
// out [rp, mp] <- K(x [rows, d], U) L_u^-T: zero, cross build, solve in place.  rp = rows rounded up to 128.
int sparse_cross(nngp_sparse* h, const double* x, const double* xq, int64_t rows, double* out, hipStream_t s, int skip) {
    const int64_t mp = h->mp, rp = round_up(rows, TB);
    NNGP_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(double) * rp * mp, s));
    BuildArgs b{};
    b.x1 = x;
    b.x2 = h->u;
    b.q1 = xq;
    b.q2 = h->uq;
    b.n1 = rows;
    b.n2 = h->m;
    b.d = h->d;
    b.row_begin = 0;
    b.row_end = rows;
    b.sym = 0;
    b.nngp64 = out;
    b.ld64 = b.ld32 = mp;
    if (!(skip & 1)) NNGP_TRY(launch_kernel_build(b, h->arch, s));
    if (skip & 2) return 0;
    return trsm_fwd_f64(out, mp, rp, h->lu, mp, h->dinv_u, mp, h->t, false, s);
}
}  // namespace nngp

extern "C" {

int nngp_sparse_create(nngp_sparse** out, int64_t m_cap, int64_t chunk_rows, int64_t test_cap, int32_t d, int32_t ny,
                       const nngp_arch_act* arch, const nngp_groups* groups, double diag_reg, int32_t diag_reg_absolute_scale,
                       double jitter) {
    NNGP_REQUIRE(out != nullptr && arch != nullptr, "sparse_create: NULL argument");
    *out = nullptr;
    NNGP_REQUIRE(m_cap >= 1 && m_cap <= 16384, "sparse_create: m_cap must be in 1 .. 16384 (m_cap=%lld)", (long long)m_cap);
    NNGP_REQUIRE(chunk_rows >= TB && chunk_rows % TB == 0, "sparse_create: chunk_rows must be a positive multiple of %d (chunk_rows=%lld)",
                 TB, (long long)chunk_rows);
    NNGP_REQUIRE(test_cap >= 1 && d >= 1, "sparse_create: need test_cap >= 1 and d >= 1 (test_cap=%lld, d=%d)", (long long)test_cap, d);
    NNGP_REQUIRE(ny >= 1 && ny <= 16, "sparse_create: ny must be in 1 .. 16 (ny=%d)", ny);
    NNGP_REQUIRE(std::isfinite(diag_reg) && diag_reg >= 0.0, "sparse_create: diag_reg must be finite and >= 0 (diag_reg=%g)", diag_reg);
    NNGP_REQUIRE(std::isfinite(jitter) && jitter >= 0.0, "sparse_create: jitter must be finite and >= 0 (jitter=%g)", jitter);
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    nngp_sparse* h = new (std::nothrow) nngp_sparse();
    NNGP_REQUIRE(h != nullptr, "sparse_create: out of host memory");
    h->m_cap = m_cap;
    h->mp_cap = round_up(m_cap, TB);
    h->chunk_rows = chunk_rows;
    h->test_cap = round_up(test_cap, TB);
    h->d = d;
    h->ny = ny;
    h->arch = ad;
    h->diag_reg = diag_reg;
    h->absolute = diag_reg_absolute_scale != 0;
    h->jitter = jitter;
    int rc = 0;
    if (groups != nullptr) {
        bool plain = false;
        rc = groups_create(groups, d, &h->groups, &plain);
        if (rc == 0 && !plain) h->arch.groups = &h->groups;
    }
    if (rc == 0) rc = sparse_alloc(h);
    if (rc != 0) {
        sparse_free(h);
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

int nngp_sparse_destroy(nngp_sparse* h) {
    if (h == nullptr) return 0;
    (void)hipDeviceSynchronize();
    sparse_free(h);
    delete h;
    return 0;
}

int nngp_sparse_set_inducing(nngp_sparse* h, const double* u, int64_t m, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && u != nullptr, "sparse_set_inducing: NULL argument");
    NNGP_REQUIRE(m >= 1 && m <= h->m_cap, "sparse_set_inducing: m=%lld outside [1, m_cap=%lld]", (long long)m, (long long)h->m_cap);
    h->m = h->mp = h->n = h->chunks = 0;
    h->finished = false;
    h->sigma2 = 0.0;
    const int64_t mp = round_up(m, TB);
    if (h->have_rel) {  // u holds raw rows: kept for the relevance gradient, scaled for everything else
        NNGP_HIP_CHECK(hipMemcpyAsync(h->ard_u, u, sizeof(double) * m * h->d, hipMemcpyDeviceToDevice, s));
        NNGP_TRY(sparse_ard_scale(h, h->ard_u, m, h->u, s));
    } else {
        NNGP_HIP_CHECK(hipMemcpyAsync(h->u, u, sizeof(double) * m * h->d, hipMemcpyDeviceToDevice, s));
    }
    NNGP_TRY(launch_row_sqnorm(h->u, m, h->d, h->uq, s));
    NNGP_HIP_CHECK(hipMemsetAsync(h->lu, 0, sizeof(double) * mp * mp, s));
    BuildArgs b = symmetric_build_args(h->u, h->uq, m, h->d);
    b.nngp64 = h->lu;
    b.ld64 = b.ld32 = mp;
    NNGP_TRY(launch_kernel_build(b, h->arch, s));
    NNGP_HIP_CHECK(hipMemsetAsync(h->scal, 0, sizeof(double) * kSpScal, s));
    hipLaunchKernelGGL(k_sparse_jitter, dim3(1), dim3(256), 0, s, h->lu, mp, m, mp, h->jitter, h->scal);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_TRY(potrf_f64(h->lu, mp, mp, h->dinv_u, h->status, s));
    NNGP_HIP_CHECK(hipMemsetAsync(h->gm, 0, sizeof(double) * mp * mp, s));
    NNGP_HIP_CHECK(hipMemsetAsync(h->rm, 0, sizeof(double) * mp * h->ny, s));
    NNGP_TRY(potrf_f64_status(h->status, s, "sparse_set_inducing: K_uu + jitter"));
    h->m = m;
    h->mp = mp;
    return 0;
}

int nngp_sparse_add_rows(nngp_sparse* h, const double* x, const double* y, int64_t n, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && x != nullptr && y != nullptr, "sparse_add_rows: NULL argument");
    NNGP_REQUIRE(h->m > 0, "sparse_add_rows: no inducing set (nngp_sparse_set_inducing)");
    NNGP_REQUIRE(n >= 1, "sparse_add_rows: n must be >= 1 (n=%lld)", (long long)n);
    const int64_t mp = h->mp;
    for (int64_t r0 = 0; r0 < n; r0 += h->chunk_rows) {
        const int64_t c = (n - r0 < h->chunk_rows) ? n - r0 : h->chunk_rows;
        const double* xc = x + r0 * h->d;
        if (h->have_rel) {
            NNGP_TRY(sparse_ard_scale(h, xc, c, h->ard_xs, s));
            xc = h->ard_xs;
        }
        NNGP_TRY(launch_row_sqnorm(xc, c, h->d, h->xq, s));
        NNGP_TRY(launch_kernel_diag(xc, h->xq, c, h->d, h->arch, h->kd, nullptr, s));
        hipLaunchKernelGGL(k_sparse_trace, dim3(1), dim3(256), 0, s, h->kd, c, h->scal);
        NNGP_HIP_CHECK(hipGetLastError());
        NNGP_TRY(sparse_evidence_sums(h, h->xq, y + r0 * h->ny, c, s));
        const int skip = sparse_skip();
        NNGP_TRY(sparse_cross(h, xc, h->xq, c, h->chunk, s, skip));
        if (!(skip & 4))
            NNGP_TRY(launch_syrk_tn_f64(h->gm, mp, h->rm, h->chunk, mp, y + r0 * h->ny, c, mp, h->ny, 1.0, h->ws, h->ws_doubles, s));
        h->finished = false;
        h->n += c;
        h->chunks += 1;
    }
    return 0;
}

int nngp_sparse_finish(nngp_sparse* h, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr, "sparse_finish: NULL argument");
    NNGP_REQUIRE(h->m > 0, "sparse_finish: no inducing set (nngp_sparse_set_inducing)");
    NNGP_REQUIRE(h->n > 0, "sparse_finish: no training rows (nngp_sparse_add_rows)");
    h->finished = false;
    const int64_t mp = h->mp, mt = mp / TB;
    hipLaunchKernelGGL(k_sparse_b, dim3((unsigned)(mt * mt)), dim3(256), 0, s, h->gm, h->lb, mp, h->diag_reg, h->absolute,
                       (double)h->n, h->scal);
    hipLaunchKernelGGL(k_sparse_rt, dim3((unsigned)((mp + 255) / 256), TB), dim3(256), 0, s, h->rm, h->ny, mp, h->ct);
    NNGP_HIP_CHECK(hipGetLastError());
    NNGP_TRY(potrf_f64(h->lb, mp, mp, h->dinv_b, h->status, s));
    NNGP_TRY(trsm_fwd_f64(h->ct, mp, TB, h->lb, mp, h->dinv_b, mp, h->t, false, s));
    NNGP_HIP_CHECK(hipMemcpyAsync(&h->sigma2, h->scal + 2, sizeof(double), hipMemcpyDeviceToHost, s));
    NNGP_TRY(potrf_f64_status(h->status, s, "sparse_finish: sigma2 I + G"));
    h->finished = true;
    return 0;
}

int nngp_sparse_predict(nngp_sparse* h, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var_or_cov,
                        void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(h != nullptr && x_test != nullptr && mean != nullptr, "sparse_predict: NULL argument");
    NNGP_REQUIRE(mt >= 1, "sparse_predict: mt must be >= 1 (mt=%lld)", (long long)mt);
    NNGP_REQUIRE(cov_mode == NNGP_COV_NONE || cov_mode == NNGP_COV_DIAG || cov_mode == NNGP_COV_FULL, "sparse_predict: bad cov_mode %d",
                 cov_mode);
    NNGP_REQUIRE(cov_mode == NNGP_COV_NONE || var_or_cov != nullptr, "sparse_predict: NULL covariance output");
    NNGP_REQUIRE(h->m > 0, "sparse_predict: no inducing set (nngp_sparse_set_inducing)");
    NNGP_REQUIRE(h->finished, "sparse_predict: no nngp_sparse_finish since the last rows were added");
    const int64_t mp = h->mp;
    const bool full = cov_mode == NNGP_COV_FULL;
    if (full) NNGP_TRY(sparse_full_reserve(h, mt, s));
    if (full && h->have_rel) NNGP_TRY(sparse_ard_full_reserve(h, round_up(mt, TB), s));
    const int64_t blk = full ? mt : h->test_cap;
    for (int64_t r0 = 0; r0 < mt; r0 += blk) {
        const int64_t rows = (mt - r0 < blk) ? mt - r0 : blk, rp = round_up(rows, TB);
        const double* xt = x_test + r0 * h->d;
        if (h->have_rel) {
            double* xs = full ? h->ard_fxs : h->ard_xs;
            NNGP_TRY(sparse_ard_scale(h, xt, rows, xs, s));
            xt = xs;
        }
        double* pm = full ? h->fp : h->pt;
        double* qm = full ? h->fq : h->qt;
        double* xq = full ? h->fxq : h->xq;
        NNGP_TRY(launch_row_sqnorm(xt, rows, h->d, xq, s));
        if (cov_mode == NNGP_COV_DIAG) NNGP_TRY(launch_kernel_diag(xt, xq, rows, h->d, h->arch, h->kd, nullptr, s));
        NNGP_TRY(sparse_cross(h, xt, xq, rows, pm, s));
        NNGP_HIP_CHECK(hipMemcpyAsync(qm, pm, sizeof(double) * rp * mp, hipMemcpyDeviceToDevice, s));
        NNGP_TRY(trsm_fwd_f64(qm, mp, rp, h->lb, mp, h->dinv_b, mp, h->t, false, s));
        hipLaunchKernelGGL(k_sparse_predict_finish, dim3((unsigned)rows), dim3(256), 0, s, pm, qm, mp, h->ct, h->ny, h->kd, h->scal,
                           mean + r0 * h->ny, cov_mode == NNGP_COV_DIAG ? var_or_cov + r0 : nullptr);
        NNGP_HIP_CHECK(hipGetLastError());
        if (!full) continue;
        // cov = K_tt - P P^T + sigma2 Q Q^T in the padded scratch, then its symmetric part to the caller's [mt, mt]
        NNGP_HIP_CHECK(hipMemsetAsync(h->fc, 0, sizeof(double) * rp * rp, s));
        BuildArgs b = symmetric_build_args(xt, xq, rows, h->d);
        b.nngp64 = h->fc;
        b.ld64 = b.ld32 = rp;
        NNGP_TRY(launch_kernel_build(b, h->arch, s));
        NNGP_TRY(launch_gemm_nt_f64(h->fc, rp, h->fc, rp, pm, mp, pm, mp, rp, rp, mp, -1.0, 1.0, s));
        NNGP_TRY(launch_gemm_nt_f64(h->fc, rp, h->fc, rp, qm, mp, qm, mp, rp, rp, mp, h->sigma2, 1.0, s));
        NNGP_TRY(launch_copy_mat_f64(h->fc, rp, var_or_cov, rows, s));
    }
    return 0;
}

int nngp_sparse_info(nngp_sparse* h, nngp_sparse_info_t* info) {
    NNGP_REQUIRE(h != nullptr && info != nullptr, "sparse_info: NULL argument");
    double sc[4] = {0.0, 0.0, 0.0, 0.0};
    NNGP_HIP_CHECK(hipDeviceSynchronize());
    NNGP_HIP_CHECK(hipMemcpy(sc, h->scal, sizeof(sc), hipMemcpyDeviceToHost));
    info->n = h->n;
    info->m = h->m;
    info->m_padded = h->mp;
    info->chunks = h->chunks;
    info->sigma2 = h->finished ? h->sigma2 : 0.0;
    info->trace_mean = h->n > 0 ? sc[0] / (double)h->n : 0.0;
    info->jitter_added = h->m > 0 ? sc[1] : 0.0;
    return 0;
}

}  // extern "C"
