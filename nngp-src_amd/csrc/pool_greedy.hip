// Greedy pool selection by conditional variance (include/nngp_pool.h: nngp_pool_select_greedy) = partial pivoted Cholesky of
// the pool's posterior covariance, left-looking: pick j reads the j earlier factor rows, never the m x m matrix again.
//
// One launch per pick, enqueued back to back.  The launch boundary is the only synchronisation: no workgroup waits for
// another, there is no counter, no atomic and no cooperative launch, so nothing here can hang.  Inside the launch for pick j
// every workgroup
//   1. finds the pivot p = argmax d_in itself (m doubles out of L2; lowest index wins, a NaN never wins, -inf = picked),
//   2. computes its 64 entries of c_j = (cov[p, :] - sum_{t<j} c_t[:] c_t[p]) / sqrt(d_in[p] + noise),
//   3. writes d_out = d_in - c_j^2 for them (d_out[p] = -inf).
// d is double-buffered between consecutive launches, so a workgroup that is still looking for the pivot never sees another
// workgroup's update.  Workgroup 0 also writes indices[j] and gains[j].
//
// The factor is stored step-major, [count][ldf]: the 64 lanes of a wave own consecutive pool indices i and read c_t[i]
// coalesced; c_t[p] is one value per t, staged in LDS in pieces of PG_PIECE so that count is not bounded by the LDS.  The four
// waves of a workgroup share the sum over t: wave w adds the terms t = w, w + 4, w + 8, ... in ascending order and the four
// partial sums are combined as (s0 + s1) + (s2 + s3).  That order depends on nothing but j, so the result is the same bits in
// every run and for every grid.  All arithmetic is float64 on the VALU (the build has -ffp-contract=off: no fused multiply-add).
#include "common.h"

#include <math.h>

namespace nngp {
namespace {

constexpr int PG_TILE = 64;      // pool indices per workgroup: one per lane
constexpr int PG_WAVES = 4;      // waves per workgroup = ways the sum over t is split
constexpr int PG_THREADS = PG_TILE * PG_WAVES;
constexpr int PG_PIECE = 1024;   // c_t[p] values staged in LDS at a time (a multiple of PG_WAVES)

// d starts as diag(cov).  -inf is the mark of a picked index, so an entry that arrives as -inf becomes NaN (never wins either)
__global__ __launch_bounds__(256) void k_greedy_init(const double* __restrict__ cov, int64_t m, int64_t ld, double* __restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double v = cov[i * ld + i];
    d[i] = (v == -INFINITY) ? (double)NAN : v;
}

// order of the pick rule: larger key first, then lower index.  NaN ranks below every number and above a picked index (-inf)
__device__ __forceinline__ double greedy_key(double v) { return (v == v) ? v : -1.7976931348623157e308; }
__device__ __forceinline__ bool greedy_better(double ka, int64_t ia, double kb, int64_t ib) { return ka > kb || (ka == kb && ia < ib); }

__global__ __launch_bounds__(PG_THREADS) void k_greedy_step(const double* __restrict__ cov, int64_t m, int64_t ld, double noise, int64_t j,
                                                            const double* __restrict__ d_in, double* __restrict__ d_out,
                                                            double* __restrict__ factor, int64_t ldf, int64_t* __restrict__ indices,
                                                            double* __restrict__ gains) {
    __shared__ double cp[PG_PIECE];
    __shared__ double part[PG_WAVES][PG_TILE];
    __shared__ double red_key[PG_WAVES];
    __shared__ int64_t red_idx[PG_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // 1. the pivot: max and tie rule are exact, so any reduction order gives the same (key, index)
    double bk = -INFINITY;
    int64_t bi = m;
    for (int64_t i = threadIdx.x; i < m; i += PG_THREADS) {
        const double k = greedy_key(d_in[i]);
        if (greedy_better(k, i, bk, bi)) { bk = k; bi = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ok = __shfl_xor(bk, off);
        const int64_t oi = __shfl_xor(bi, off);
        if (greedy_better(ok, oi, bk, bi)) { bk = ok; bi = oi; }
    }
    if (lane == 0) { red_key[wave] = bk; red_idx[wave] = bi; }
    __syncthreads();
    bk = red_key[0];
    bi = red_idx[0];
    for (int w = 1; w < PG_WAVES; ++w)
        if (greedy_better(red_key[w], red_idx[w], bk, bi)) { bk = red_key[w]; bi = red_idx[w]; }
    // bi < m always: count <= m and only picked entries are -inf (see the update of d below), so an entry that is not picked, with a
    // key above -inf, is left at every step.  The clamp only keeps every address below inside the pool whatever d_in holds.
    const int64_t p = (bi < m) ? bi : 0;
    const double gain = d_in[p];
    const double piv = gain + noise;
    const bool regular = piv > 0.0;  // false for a NaN pivot too
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        indices[j] = p;
        if (gains != nullptr) gains[j] = gain;
    }

    // 2. this workgroup's entries of the column
    const int64_t i = (int64_t)blockIdx.x * PG_TILE + lane;
    const bool live = i < m;
    double acc = 0.0;
    if (regular) {
        for (int64_t t0 = 0; t0 < j; t0 += PG_PIECE) {
            const int len = (j - t0 < PG_PIECE) ? (int)(j - t0) : PG_PIECE;
            __syncthreads();  // the previous piece has been read (and red_* above)
            for (int tt = threadIdx.x; tt < len; tt += PG_THREADS) cp[tt] = factor[(t0 + tt) * ldf + p];
            __syncthreads();
            if (live) {
                const double* col = factor + t0 * ldf + i;
#pragma unroll 4
                for (int tt = wave; tt < len; tt += PG_WAVES) acc += col[(int64_t)tt * ldf] * cp[tt];
            }
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave != 0 || !live) return;
    const double s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    const double c = regular ? (cov[p * ld + i] - s) / sqrt(piv) : 0.0;
    factor[j * ldf + i] = c;
    // 3. the conditional variances after this pick
    // -inf means "picked" and nothing else: a picked entry stays -inf whatever c is (a NaN entry of cov would make it NaN and
    // pickable again), and an entry that is not picked never becomes -inf (c * c can overflow): it becomes NaN, as in k_greedy_init
    const double di = d_in[i];
    double dn = regular ? di - c * c : di;
    if (dn == -INFINITY) dn = (double)NAN;
    d_out[i] = (i == p || di == -INFINITY) ? -INFINITY : dn;
}

}  // namespace

// ws: 2 m doubles (the two copies of d).  factor: [count, ldf], never NULL here.
int launch_pool_greedy(const double* cov, int64_t m, int64_t ld, double noise, int64_t count, int64_t* indices, double* gains,
                       double* factor, int64_t ldf, double* ws, hipStream_t s) {
    double* d0 = ws;
    double* d1 = ws + m;
    hipLaunchKernelGGL(k_greedy_init, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, cov, m, ld, d0);
    const dim3 grid((unsigned)((m + PG_TILE - 1) / PG_TILE));
    for (int64_t j = 0; j < count; ++j) {
        hipLaunchKernelGGL(k_greedy_step, grid, dim3(PG_THREADS), 0, s, cov, m, ld, noise, j, d0, d1, factor, ldf, indices, gains);
        double* t = d0;
        d0 = d1;
        d1 = t;
    }
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nngp
