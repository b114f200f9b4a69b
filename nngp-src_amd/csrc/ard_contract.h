// The contraction of the relevance gradient over a SYMMETRIC kernel, shared between the exact evidence (nngp_ard.hip) and the
// sparse evidence's K_uu half (sparse_ard.hip): what follows adjoint_tile<., ., true> of nngp_adjoint.h.
//
//   k_ard_contract       per 64-row block I, 32 features and seed, Z_I = sum_{J <= I} (S o c)[I, J] X_J on the float64 MFMA
//                        (v_mfma_f64_16x16x4: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], and D at column l & 15,
//                        row (l >> 4) + 4 reg), then sum_{i in I} x_ik (Z_ik + qbar_i x_ik), rows in order
//   k_ard_finish         the row blocks summed in order
// The kernels sit in an anonymous namespace: each file that includes this header launches its own copy.
#pragma once
#include "nngp_adjoint.h"

namespace nngp {

namespace {

constexpr int AKC = 32;  // features per workgroup of the contraction: two 16-wide MFMA column blocks per wave
typedef double v4d __attribute__((ext_vector_type(4)));

// grid (row blocks, feature chunks, 2 seeds).  cmat: seed 0 at (i, j), seed 1 at (j, i), j < i < n; x: the raw inputs.
// part[(seed * tn + I) * d + k]; seed 0 also writes part[(2 tn + I) * d + k] = sum_{i in I} x_ik^2.
__global__ __launch_bounds__(256) void k_ard_contract(const double* cmat, int64_t ldc, const double* x, int64_t n, int d,
                                                      const double* qbar, int64_t np, int64_t tn, double* part) {
    __shared__ double ms[MT][MT + 1];
    __shared__ double xt[MT][AKC + 1];
    __shared__ double qb[MT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int64_t ti = blockIdx.x, i0 = ti * MT;
    const int k0 = blockIdx.y * AKC, seed = blockIdx.z;
    if (tid < MT) {  // qbar of the block's rows: the tiles' slots in order
        double t = 0.0;
        for (int64_t sl = 0; sl < tn; ++sl) t += qbar[((int64_t)seed * tn + sl) * np + i0 + tid];
        qb[tid] = t;
    }
    v4d acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int64_t tj = 0; tj <= ti; ++tj) {
        const int64_t j0 = tj * MT;
        for (int e = tid; e < MT * MT; e += 256) {  // the fast index runs along memory for either seed
            const int r = seed == 0 ? e >> 6 : e & (MT - 1), c = seed == 0 ? e & (MT - 1) : e >> 6;
            const int64_t i = i0 + r, j = j0 + c;
            ms[r][c] = (i < n && j < i) ? (seed == 0 ? cmat[i * ldc + j] : cmat[j * ldc + i]) : 0.0;
        }
        for (int e = tid; e < MT * AKC; e += 256) {
            const int c = e / AKC, k = e % AKC;
            const int64_t j = j0 + c;
            xt[c][k] = (j < n && k0 + k < d) ? x[j * d + k0 + k] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < MT; kk += 4) {
            const double av = ms[16 * wv + lr][kk + lk];
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xt[kk + lk][lr], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xt[kk + lk][16 + lr], acc[1], 0, 0, 0);
        }
        __syncthreads();
    }
    for (int e = tid; e < MT * AKC; e += 256) {  // the block's own rows of x
        const int c = e / AKC, k = e % AKC;
        const int64_t i = i0 + c;
        xt[c][k] = (i < n && k0 + k < d) ? x[i * d + k0 + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = 16 * wv + lk + 4 * reg, c = 16 * hb + lr;
            const double xv = xt[r][c];
            ms[r][c] = xv * (acc[hb][reg] + qb[r] * xv);
        }
    __syncthreads();
    if (tid < AKC) {
        double t = 0.0;
        for (int r = 0; r < MT; ++r) t += ms[r][tid];
        if (k0 + tid < d) part[((int64_t)seed * tn + ti) * d + k0 + tid] = t;
    } else if (tid < 2 * AKC && seed == 0) {
        const int k = tid - AKC;
        double t = 0.0;
        for (int r = 0; r < MT; ++r) t += xt[r][k] * xt[r][k];
        if (k0 + k < d) part[((int64_t)2 * tn + ti) * d + k0 + k] = t;
    }
}

// out[v * d + k] = sum over the row blocks, in order, of part[(v * tn + I) * d + k]  (v = 0, 1: the seeds; 2: sum_i x_ik^2)
__global__ __launch_bounds__(256) void k_ard_finish(const double* part, int64_t tn, int d, double* out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * d) return;
    const int v = e / d, k = e % d;
    double t = 0.0;
    for (int64_t b = 0; b < tn; ++b) t += part[((int64_t)v * tn + b) * d + k];
    out[e] = t;
}

}  // namespace

}  // namespace nngp
