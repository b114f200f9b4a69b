// The contraction of the relevance gradient: the one body behind k_ard_contract (nngp_ard.hip: a SYMMETRIC kernel, what follows
// adjoint_tile<., ., true> of nngp_adjoint.h, for the exact evidence, the leave-one-out objectives and the sparse evidence's
// K_uu half) and k_sparse_ard_contract (sparse_ard.hip: the RECTANGULAR block K_fu of a chunk, what follows rect_tile<., true>).
//
//   ard_contract_body    per 64-row block I, 32 features and seed, Z_I = sum_J (S o c)[I, J] B_J on the float64 MFMA
//                        (v_mfma_f64_16x16x4: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], and D at column l & 15,
//                        row (l >> 4) + 4 reg), then sum_{i in I} x_ik (Z_ik + qbar_i x_ik), rows in order, and sum_{i in I} x_ik^2
//   ard_block_sum        the row blocks summed in order: what either finish kernel stores or adds
// A staging policy carries what the two forms do not share:
//   stage(ms, i0, j0, tid)   the 64 x 64 tile of the seeded adjoint at rows i0.., columns j0.. into LDS, zero outside
//   tiles(ti)                how many column tiles row block ti walks, from 0 upwards
//   b, nb                    the rows behind the B operand: [nb, d]
#pragma once
#include "nngp_adjoint.h"

namespace nngp {

constexpr int AKC = 32;  // features per workgroup of the contraction: two 16-wide MFMA column blocks per wave
typedef double v4d __attribute__((ext_vector_type(4)));

// grid (row blocks, feature chunks, 2 seeds), 256 threads.  x: [nx, d] the raw rows of the blocks; qslots: per seed nslots
// rows of qld, summed in order into qbar of the block's rows; part[(seed * nblocks + I) * d + k], and seed 0 also writes
// part[(2 nblocks + I) * d + k] = sum_{i in I} x_ik^2.
template <class Stage>
__device__ __forceinline__ void ard_contract_body(const Stage& st, const double* x, int64_t nx, int d, const double* qslots,
                                                  int64_t nslots, int64_t qld, int64_t nblocks, double* part) {
    __shared__ double ms[MT][MT + 1];
    __shared__ double xt[MT][AKC + 1];
    __shared__ double qb[MT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int64_t ti = blockIdx.x, i0 = ti * MT;
    const int k0 = blockIdx.y * AKC, seed = blockIdx.z;
    if (tid < MT) {
        double t = 0.0;
        for (int64_t sl = 0; sl < nslots; ++sl) t += qslots[((int64_t)seed * nslots + sl) * qld + i0 + tid];
        qb[tid] = t;
    }
    v4d acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    const int64_t ntiles = st.tiles(ti);
    for (int64_t tj = 0; tj < ntiles; ++tj) {
        const int64_t j0 = tj * MT;
        st.stage(ms, i0, j0, tid);
        for (int e = tid; e < MT * AKC; e += 256) {
            const int c = e / AKC, k = e % AKC;
            const int64_t j = j0 + c;
            xt[c][k] = (j < st.nb && k0 + k < d) ? st.b[j * d + k0 + k] : 0.0;
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
        xt[c][k] = (i < nx && k0 + k < d) ? x[i * d + k0 + k] : 0.0;
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
        if (k0 + tid < d) part[((int64_t)seed * nblocks + ti) * d + k0 + tid] = t;
    } else if (tid < 2 * AKC && seed == 0) {
        const int k = tid - AKC;
        double t = 0.0;
        for (int r = 0; r < MT; ++r) t += xt[r][k] * xt[r][k];
        if (k0 + k < d) part[((int64_t)2 * nblocks + ti) * d + k0 + k] = t;
    }
}

// sum over the row blocks, in order, of part[(v * nblocks + I) * d + k], e = v * d + k  (v = 0, 1: the seeds; 2: sum_i x_ik^2)
__device__ __forceinline__ double ard_block_sum(const double* part, int64_t nblocks, int d, int64_t e) {
    const int64_t v = e / d, k = e % d;
    double t = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) t += part[(v * nblocks + b) * d + k];
    return t;
}

}  // namespace nngp
