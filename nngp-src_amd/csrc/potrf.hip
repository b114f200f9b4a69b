// Blocked lower Cholesky in float32 for gfx950 -- replaces scipy/LAPACK cho_factor inside
// nt.predict.gradient_descent_mse_ensemble (reference train.py:171-172).
//
// Structure: a host-side recursion (potrf -> trsm -> syrk -> potrf) bottoms out at 128x128 leaves, so
// every flop above the leaves runs in the MFMA GEMM of gemm_f32.hip with a deep K.  The leaf kernel
// factors one 128x128 diagonal block in LDS *and* inverts the factor; triangular solves against a
// diagonal block then become an in-place GEMM with the inverse (no serial substitution anywhere above
// the leaf).  The look-ahead schedules that run this recursion per block column are in potrf_lookahead.hip.
//
// Leaf (one 256-thread workgroup): the block is treated as 4x4 sub-blocks of 32x32.  Per sub-block
// column: wave 0 factors the 32x32 diagonal sub-block and inverts it entirely in registers (lane = row,
// v_readlane broadcasts, no barriers), then the sub-blocks below are multiplied by the inverse and the
// trailing sub-blocks updated with v_mfma_f32_32x32x2_f32.  The 128x128 inverse is assembled from the
// 32x32 inverses by block forward substitution on the matrix cores.  LDS row stride is 129 floats, which
// makes row-wise and column-wise 4-byte fragment reads conflict free.
#include <atomic>
#include <cstdio>

#include "common.h"

namespace nngp {

#ifdef NNGP_TIMING_KNOBS
std::atomic<int> g_knobs[16];  // timing experiments only (libnngp_hip_knobs.so: nngp_debug_set); zero-initialised
#endif

namespace {

constexpr int LS = 33;            // LDS row stride of one 32x32 sub-block (odd: row- and column-wise reads conflict free)
constexpr int BLK = 32 * LS;      // floats per packed sub-block
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Only the 10 sub-blocks on or below the diagonal are kept in LDS (L and X = L^-1 are lower triangular):
// 2 x 10 x 32 x 33 floats = 84.5 KB, so the leaf co-resides with a 64 KB GEMM workgroup on the same CU.
__device__ __forceinline__ constexpr int blk(int ib, int jb) { return ib * (ib + 1) / 2 + jb; }

// acc += sign * A_blk(32x32) * op(B_blk);  NN: op(B) = B,  NT: op(B) = B^T.  Blocks live in LDS, stride LS.
template <bool NN>
__device__ __forceinline__ f32x16 blk_mma(const float* ab, const float* bb, f32x16 acc, float sign, int lane) {
    const int r = lane & 31, h = lane >> 5;
    // all 32 operand reads first, then the 16 MFMAs back to back (interleaved, each MFMA waited for its own LDS round trip)
    float av[16], bv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int k = 2 * s + h;
        av[s] = ab[r * LS + k];
        bv[s] = NN ? bb[k * LS + r] : bb[r * LS + k];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sign * av[s], bv[s], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ f32x16 blk_load(const float* p, int lane) {
    f32x16 v;
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = p[((r & 3) + 8 * (r >> 2) + 4 * h) * LS + c];
    return v;
}

__device__ __forceinline__ void blk_store(float* p, f32x16 v, int lane) {
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) p[((r & 3) + 8 * (r >> 2) + 4 * h) * LS + c] = v[r];
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.0f;
    return v;
}

template <int VARIANT>
__global__ __launch_bounds__(256) void k_potrf_leaf(float* A, int64_t ld, float* dinv, int32_t* clamped,
                                                       float pivot_floor, int dbg) {
    __shared__ float Lb[10 * BLK];
    __shared__ float Xb[10 * BLK];
    __shared__ float Tb[3 * BLK];   // scratch of the inverse assembly (one block per active wave)
    __shared__ float colbuf[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = tid >> 3, lc = (tid & 7) * 4;  // this thread's (row, first column) inside a 32x32 sub-block

    {
        // one 16-byte load per thread per lower sub-block, all 10 issued back to back
        float4 v[10];
#pragma unroll
        for (int ib = 0; ib < 4; ++ib)
#pragma unroll
            for (int jb = 0; jb <= ib; ++jb)
                v[blk(ib, jb)] = *reinterpret_cast<const float4*>(A + (int64_t)(ib * 32 + lr) * ld + jb * 32 + lc);
#pragma unroll
        for (int ib = 0; ib < 4; ++ib)
#pragma unroll
            for (int jb = 0; jb <= ib; ++jb) {
                const float4 t = v[blk(ib, jb)];
                float* lp = Lb + blk(ib, jb) * BLK + lr * LS + lc;
                float* xp = Xb + blk(ib, jb) * BLK + lr * LS + lc;
                const bool diag = (ib == jb);  // strictly-upper entries of a diagonal sub-block are not part of A
                lp[0] = (!diag || lc + 0 <= lr) ? t.x : 0.0f;
                lp[1] = (!diag || lc + 1 <= lr) ? t.y : 0.0f;
                lp[2] = (!diag || lc + 2 <= lr) ? t.z : 0.0f;
                lp[3] = (!diag || lc + 3 <= lr) ? t.w : 0.0f;
                xp[0] = xp[1] = xp[2] = xp[3] = 0.0f;
            }
    }
    __syncthreads();

    int nclamp = 0;
#pragma unroll 1
    for (int jb = 0; jb < 4; ++jb) {
        float* Djj = Lb + blk(jb, jb) * BLK;
        float* Xjj = Xb + blk(jb, jb) * BLK;
        if (wave == 0 && !(dbg & 1)) {
            // One wave factors and inverts the 32x32 diagonal sub-block.  Lane i owns row i in registers; the
            // values every lane needs (pivot, column j) travel through a 32-float LDS line read back as
            // broadcasts -- an LDS round trip per column instead of ~500 v_readlane + hazard nops.
            const int i = lane & 31;
            float a[32], x[32], pinv[32];  // pinv[j] = 1 / L[j][j] (wave-uniform), reused by the inversion
#pragma unroll
            for (int k = 0; k < 32; ++k) a[k] = Djj[i * LS + k];
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                float* col = colbuf + (j & 1) * 32;
                if (VARIANT == 0 || lane < 32) col[i] = a[j];  // current column j (rows >= j are valid)
                float d = col[j];
                asm volatile("" : "+v"(d));  // keep wave-uniform values in VGPRs (no SGPR spills / readlane traffic)
                if (!(d > pivot_floor)) {
                    d = pivot_floor > 0.0f ? pivot_floor : 1.0e-30f;
                    ++nclamp;
                }
                float inv = __builtin_amdgcn_rsqf(d);  // v_rsq_f32, ~1 ulp: ample for a preconditioner
                asm volatile("" : "+v"(inv));
                pinv[j] = inv;
                const float lij = a[j] * inv;                // L[i][j] for i > j
                a[j] = (i == j) ? d * inv : lij;
                const float t = -lij * inv;                  // a[i][k] -= L[i][j] L[k][j] = a[i][k] + t * col[k]
#pragma unroll
                for (int k = j + 1; k < 32; ++k) {
                    float ck = col[k];
                    if (VARIANT == 0) asm volatile("" : "+v"(ck));  // stay in VGPRs: scalarising 496 broadcasts spills SGPRs
                    a[k] = fmaf(t, ck, a[k]);
                }
            }
            if (lane < 32) {
#pragma unroll
                for (int k = 0; k < 32; ++k) Djj[i * LS + k] = (k <= i) ? a[k] : 0.0f;
            }
            // inverse: lane c owns column c of X = L^-1;  X[ii][c] = (delta - sum_{k<ii} L[ii][k] X[k][c]) / L[ii][ii]
            // (measured and dropped in round 2: computing row j of X inside step j of the factorisation loop above, so that the two
            // 32-step dependent passes become one -- 60 us per leaf instead of 50: the merged loop body schedules worse)
#pragma unroll
            for (int ii = 0; ii < 32; ++ii) {
                float s0 = 0.0f, s1 = 0.0f;  // two chains: the sum is latency-, not throughput-bound
#pragma unroll
                for (int k = 0; k + 1 < ii; k += 2) {
                    s0 = fmaf(Djj[ii * LS + k], x[k], s0);  // broadcast LDS reads
                    s1 = fmaf(Djj[ii * LS + k + 1], x[k + 1], s1);
                }
                if (ii & 1) s0 = fmaf(Djj[ii * LS + ii - 1], x[ii - 1], s0);
                x[ii] = (((i == ii) ? 1.0f : 0.0f) - (s0 + s1)) * pinv[ii];
            }
            if (lane < 32) {
#pragma unroll
                for (int k = 0; k < 32; ++k) Xjj[k * LS + i] = x[k];  // X[k][c = i]
            }
        }
        __syncthreads();
        // ---- sub-blocks below the diagonal: A[ib][jb] <- A[ib][jb] * Dinv^T ----
        if (!(dbg & 4)) {
            const int ib = jb + 1 + wave;
            if (ib < 4) {
                float* Aij = Lb + blk(ib, jb) * BLK;
                f32x16 acc = blk_mma<false>(Aij, Xjj, zero16(), 1.0f, lane);
                blk_store(Aij, acc, lane);
            }
        }
        __syncthreads();
        // ---- trailing sub-blocks: A[ib][kb] -= A[ib][jb] * A[kb][jb]^T, jb < kb <= ib ----
        if (!(dbg & 4)) {
            int cnt = 0;
            for (int ib = jb + 1; ib < 4; ++ib)
                for (int kb = jb + 1; kb <= ib; ++kb, ++cnt) {
                    if ((cnt & 3) != wave) continue;
                    float* Cik = Lb + blk(ib, kb) * BLK;
                    f32x16 acc = blk_load(Cik, lane);
                    acc = blk_mma<false>(Lb + blk(ib, jb) * BLK, Lb + blk(kb, jb) * BLK, acc, -1.0f, lane);
                    blk_store(Cik, acc, lane);
                }
        }
        __syncthreads();
    }

    // ---- assemble the 128x128 inverse: X[ib][jb] = -Dinv_ii * sum_{k=jb}^{ib-1} L[ib][k] X[k][jb] ----
#pragma unroll 1
    for (int dist = 1; dist < ((dbg & 2) ? 1 : 4); ++dist) {
        const int ib = dist + wave, jb = wave;  // wave w owns block (dist + w, w)
        const bool active = ib < 4;
        float* scratch = Tb + (wave < 3 ? wave : 0) * BLK;
        if (active) {
            f32x16 t = zero16();
            for (int k = jb; k < ib; ++k)
                t = blk_mma<true>(Lb + blk(ib, k) * BLK, Xb + blk(k, jb) * BLK, t, 1.0f, lane);
            blk_store(scratch, t, lane);
        }
        __syncthreads();
        if (active) {
            f32x16 xr = blk_mma<true>(Xb + blk(ib, ib) * BLK, scratch, zero16(), -1.0f, lane);
            blk_store(Xb + blk(ib, jb) * BLK, xr, lane);
        }
        __syncthreads();
    }

    // ---- write back: L into the lower triangle of A, X (with its zero upper blocks) into dinv ----
#pragma unroll 1
    for (int b = 0; b < 16; ++b) {
        const int ib = b >> 2, jb = b & 3;
        float4 xo = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jb <= ib) {
            const float* lp = Lb + blk(ib, jb) * BLK + lr * LS + lc;
            const float* xp = Xb + blk(ib, jb) * BLK + lr * LS + lc;
            xo = make_float4(xp[0], xp[1], xp[2], xp[3]);
            float* ap = A + (int64_t)(ib * 32 + lr) * ld + jb * 32 + lc;
            if (ib != jb || lc + 3 <= lr) {
                *reinterpret_cast<float4*>(ap) = make_float4(lp[0], lp[1], lp[2], lp[3]);
            } else {  // the 4-wide group straddles or lies above the diagonal: keep the caller's upper entries
                for (int k = 0; k < 4; ++k)
                    if (lc + k <= lr) ap[k] = lp[k];
            }
        }
        *reinterpret_cast<float4*>(dinv + (ib * 32 + lr) * 128 + jb * 32 + lc) = xo;
    }
    if (wave == 0 && lane == 0 && nclamp > 0 && clamped != nullptr) atomicAdd(clamped, nclamp);
}

// Panel form of the leaf (the product path; k_potrf_leaf above is kept for A/B timing, debug key 3 = 2).  In k_potrf_leaf
// three of the four waves idle while wave 0 factors AND inverts each 32x32 diagonal sub-block (two dependent 32-step passes,
// ~8 of the ~11 us a sub-block column takes), and the sub-blocks below wait for that inverse.  Here the wave that owns block
// row w eliminates its 32 rows against the diagonal sub-block's columns AS the leader (wave jb) produces them: the leader
// publishes column j of the diagonal sub-block in an LDS ring and bumps a step counter, the followers poll the counter and
// apply the same rank-1 step to their own rows (LDS operations of one wave execute in order, so the counter is visible after
// the column; no barrier inside the 32 steps).  The sub-blocks below are therefore solved by substitution when the leader
// finishes -- no inverse on the critical path -- and the four diagonal inverses are computed at the end, one per wave, in
// parallel.  Critical path per sub-block column: one 32-step pass + the MFMA updates.
#ifdef NNGP_TIMING_KNOBS
__device__ unsigned long long g_leaf_stamps[4 * 16];  // per wave: cycles from kernel start to the end of each phase (debug key 7 = 8)
#define LEAF_STAMP(idx) do { if (lane == 0) g_leaf_stamps[wave * 16 + (idx)] = __builtin_amdgcn_s_memtime() - t_start_; } while (0)
#else
#define LEAF_STAMP(idx) do { } while (0)
#endif
template <int FORM>
__global__ __launch_bounds__(256) void k_potrf_leaf_panel(float* A, int64_t ld, float* dinv, int32_t* clamped,
                                                             float pivot_floor) {
    __shared__ float Lb[10 * BLK];
    __shared__ float Xb[10 * BLK];
    __shared__ float Tb[6 * BLK];   // scratch of the inverse assembly
    // FORM 1: word (j, lane) = the A operand of step j for the followers (low half; see below) tagged with the step number (high half)
    // FORM 0: as floats, line j/2: columns j and j+1 of the current diagonal sub-block before elimination step j (layout: see rd)
    __shared__ unsigned long long ring64[32 * 64];
    __shared__ float ring_inv[32];   // FORM 1: 1 / L[j][j] of the sub-block column being eliminated
    __shared__ int step_flag;        // FORM 0: column pairs published so far: 16 jb + j/2 + 1
    float* ring = reinterpret_cast<float*>(ring64);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = tid >> 3, lc = (tid & 7) * 4;  // this thread's (row, first column) inside a 32x32 sub-block
    if (tid == 0) step_flag = 0;
    if (FORM == 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) ring64[k * 256 + tid] = 0ull;  // no stale tag may look like a published step
    }
#ifdef NNGP_TIMING_KNOBS
    const unsigned long long t_start_ = __builtin_amdgcn_s_memtime();
#endif
    {
        float4 v[10];
#pragma unroll
        for (int ib = 0; ib < 4; ++ib)
#pragma unroll
            for (int jb = 0; jb <= ib; ++jb)
                v[blk(ib, jb)] = *reinterpret_cast<const float4*>(A + (int64_t)(ib * 32 + lr) * ld + jb * 32 + lc);
#pragma unroll
        for (int ib = 0; ib < 4; ++ib)
#pragma unroll
            for (int jb = 0; jb <= ib; ++jb) {
                const float4 t = v[blk(ib, jb)];
                float* lp = Lb + blk(ib, jb) * BLK + lr * LS + lc;
                float* xp = Xb + blk(ib, jb) * BLK + lr * LS + lc;
                const bool diag = (ib == jb);  // strictly-upper entries of a diagonal sub-block are not part of A
                lp[0] = (!diag || lc + 0 <= lr) ? t.x : 0.0f;
                lp[1] = (!diag || lc + 1 <= lr) ? t.y : 0.0f;
                lp[2] = (!diag || lc + 2 <= lr) ? t.z : 0.0f;
                lp[3] = (!diag || lc + 3 <= lr) ? t.w : 0.0f;
                xp[0] = xp[1] = xp[2] = xp[3] = 0.0f;
            }
    }
    __syncthreads();
    LEAF_STAMP(0);

    int nclamp = 0;
    const int i = lane & 31, h = lane >> 5;
    // Lane (i, h) owns the entries of row i in the columns of parity h: b[m] = entry (i, 2m + h) of block (wave, jb) -- the two
    // half-waves split the rank-1 updates between them instead of duplicating them.
    float b[16], pinv[32];  // pinv[j] = 1 / L[j][j] of the sub-block this wave led (FORM 0)
    float invl = 0.0f;      // FORM 1: lane c (both halves): 1 / L[c][c] of the sub-block this wave led
    const float* rd = ring + h * 32;  // a column pair is stored by row parity: entry (k, A|B) at ((k & 1) * 16 + (k >> 1)) * 2 + (A: 0, B: 1)
#pragma unroll 1
    for (int jb = 0; jb < 4; ++jb) {
        f32x16 acc;
        if (FORM == 1 && wave >= jb) {
            // Round 5: the sub-blocks stay in the MFMA accumulator layout for the 32 steps and every step is ONE rank-1
            // v_mfma_f32_32x32x2_f32 per wave -- no LDS round trip and no per-element FMAs in the leader's chain (readlane of the
            // pivot -> v_rsq_f32 -> one multiply -> MFMA: 54 ns a step against 75 with a separate flag behind a release,
            // scripts/micro/mfma_chain.hip).  The leader holds the diagonal sub-block S as a full symmetric matrix: row j of S IS
            // column j, already one entry per lane (lanes of half hj), which is the layout of both MFMA operands; the finished
            // columns are frozen by zeroing the operand there, so at the end entry (m, c), c < m, holds L[m][c] / inv_c.  A follower
            // holds its sub-block TRANSPOSED and UNSCALED (accumulator row j = column j of the block before its division by
            // L[j][j]): that row is the B operand as it stands, the A operand is the leader's -L[.][j] / L[j][j], published as
            // ONE 8-byte word per lane {value, step number} -- value and tag arrive together, so neither side orders anything: no
            // flag, no release wait in the leader, one LDS round trip per step in the follower.
            const bool leader = (wave == jb);
            float* Bw = Lb + blk(wave, jb) * BLK;
            if (leader) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {  // the full symmetric block from its lower triangle
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                    acc[r] = Bw[(i <= row) ? row * LS + i : i * LS + row];
                }
                const float floor_eff = pivot_floor > 0.0f ? pivot_floor : 1.0e-30f;
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    const int rj = (j & 3) + 4 * (j >> 3), hj = (j >> 2) & 1;  // accumulator register / lane half that hold row j
                    const float xr = acc[rj];
                    const float xm = (h == hj && i > j) ? xr : 0.0f;  // rows below the pivot (beside the rsq, not behind it)
                    const float d_raw = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xr), 32 * hj + j));
                    const float inv = __builtin_amdgcn_rsqf(fmaxf(d_raw, floor_eff));  // v_rsq_f32, ~1 ulp: ample for a preconditioner
                    const float x = xm * inv;  // L[i][j]
                    const float xn = xm * -inv;
                    // (the publish goes in FRONT of the MFMA: behind it the LDS store waits for its data while the MFMA streams the
                    // accumulator through the register file -- 80 cycles a step against ~12)
                    if (jb < 3) {  // (the last sub-block column has no followers)
                        const float xq = xn * inv;
                        const unsigned long long word = ((unsigned long long)(unsigned)(jb * 32 + j + 1) << 32) | (unsigned long long)__builtin_bit_cast(unsigned, xq);
                        __hip_atomic_store(&ring64[j * 64 + lane], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xn, x, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // Nothing but the chain was kept per step: entry (c, c) of the accumulator was frozen at step c and IS the pivot of
                // column c as the chain read it, so every lane redoes its own column's clamp and v_rsq_f32 (same instructions on the
                // same value: the same bits) -- 1 / L[c][c] for the scaling below, for the followers and for this wave's inverse.
                float dsel = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) dsel = ((r & 3) + 8 * (r >> 2) + 4 * h == i) ? acc[r] : dsel;
                const float dother = __shfl_xor(dsel, 32);
                const float d_raw = (((i >> 2) & 1) == h) ? dsel : dother;  // the half whose rows include row i holds it
                nclamp += __builtin_popcount((unsigned)__ballot(!(d_raw > pivot_floor)));  // lanes 0 .. 31: one per column
                const float dcl = fmaxf(d_raw, floor_eff);  // (a NaN pivot is clamped as well)
                invl = __builtin_amdgcn_rsqf(dcl);
                const float diagl = dcl * invl;
                if (jb < 3 && lane < 32) ring_inv[lane] = invl;  // (the followers read it behind the barrier below)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                    Bw[row * LS + i] = (i < row) ? acc[r] * invl : (i == row ? diagl : 0.0f);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = Bw[i * LS + (r & 3) + 8 * (r >> 2) + 4 * h];  // transposed
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    const int rj = (j & 3) + 4 * (j >> 3), hj = (j >> 2) & 1;
                    const int target = jb * 32 + j + 1;
                    const float bq = (h == hj) ? acc[rj] : 0.0f;  // this wave's column j, not yet divided by L[j][j]
                    unsigned long long word;
                    for (;;) {  // every lane waits for its own word
                        word = __hip_atomic_load(&ring64[j * 64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if ((int)(word >> 32) == target) break;
                    }
                    const float a = __builtin_bit_cast(float, (unsigned)word);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq, acc, 0, 0, 0);
                }
            }
        }
        if (FORM == 1) {
            __syncthreads();  // the leader's 1 / L[j][j] are in place
            if (wave > jb) {
                float* Bw = Lb + blk(wave, jb) * BLK;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;  // column of the block
                    Bw[i * LS + row] = acc[r] * ring_inv[row];
                }
            }
        }
        if (FORM == 0 && wave >= jb) {
            const bool leader = (wave == jb);
            float* Bw = Lb + blk(wave, jb) * BLK;
#pragma unroll
            for (int m = 0; m < 16; ++m) b[m] = Bw[i * LS + 2 * m + h];
            // Two columns per LDS round trip (the round trip, ~300 cycles with its issue, is what a step costs): the leader
            // publishes columns j and j+1 as they are BEFORE step j; every lane applies step j to its copy of column j+1 itself
            // (one more FMA per element) and then both rank-1 updates to its own entries.
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int j = 2 * p;
                float* line = ring + p * 64;
                const int target = jb * 16 + p + 1;
                float d0, c10, b11;
                if (leader) {
                    // plain LDS stores kept in program order by the compiler barriers: the LDS executes one wave's operations
                    // in order, and `volatile` would make hipcc wait for each of them (770 instead of ~300 cycles a step)
                    line[((i & 1) * 16 + (i >> 1)) * 2 + h] = b[p];  // half 0: column j, half 1: column j+1 (rows >= j valid)
                    asm volatile("" ::: "memory");
                    if (lane == 0) step_flag = target;
                    asm volatile("" ::: "memory");
                    // the leader's own pivots: no LDS round trip in front of the rsq chain
                    d0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b[p]), j));
                    c10 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b[p]), j + 1));
                    b11 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b[p]), 32 + j + 1));
                } else {
                    while (__hip_atomic_load(&step_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) {}
                    asm volatile("" ::: "memory");
                    d0 = line[p * 2];              // (k = j,   A)
                    c10 = line[(16 + p) * 2];      // (k = j+1, A)
                    b11 = line[(16 + p) * 2 + 1];  // (k = j+1, B)
                }
                asm volatile("" : "+v"(d0), "+v"(c10), "+v"(b11));  // keep wave-uniform values in VGPRs (no SGPR spills / readlane traffic)
                // the columns are requested before the rsq chain below, not behind it
                float ck0[16], ck1[16];
#pragma unroll
                for (int m = p + 1; m < 16; ++m) {
                    ck0[m] = rd[p * 64 + 2 * m];
                    ck1[m] = rd[p * 64 + 2 * m + 1];
                }
                const float other = __shfl_xor(b[p], 32);  // half 0 gets its row's entry of column j+1, half 1 that of column j
                __builtin_amdgcn_sched_barrier(0);
                if (!(d0 > pivot_floor)) {
                    d0 = pivot_floor > 0.0f ? pivot_floor : 1.0e-30f;
                    if (leader) ++nclamp;
                }
                float inv0 = __builtin_amdgcn_rsqf(d0);  // v_rsq_f32, ~1 ulp: ample for a preconditioner
                asm volatile("" : "+v"(inv0));
                const float l10 = c10 * inv0;            // L[j+1][j]
                const float u10 = -l10 * inv0;           // column j+1 after step j: B[k] + u10 * A[k]
                float d1 = fmaf(u10, c10, b11);          // = A[j+1][j+1] - L[j+1][j]^2
                if (!(d1 > pivot_floor)) {
                    d1 = pivot_floor > 0.0f ? pivot_floor : 1.0e-30f;
                    if (leader) ++nclamp;
                }
                float inv1 = __builtin_amdgcn_rsqf(d1);
                asm volatile("" : "+v"(inv1));
                pinv[j] = inv0;
                pinv[j + 1] = inv1;
                const float aj0 = h ? other : b[p];          // this row's entries of columns j and j+1 (before step j)
                const float aj1p = h ? b[p] : other;
                const float lij0 = aj0 * inv0;               // L[row][j]
                const float t0 = -lij0 * inv0;
                const float aj1 = fmaf(t0, c10, aj1p);       // entry of column j+1 after step j
                const float lij1 = aj1 * inv1;               // L[row][j+1]
                const float t1 = -lij1 * inv1;
                b[p] = h ? ((leader && i == j + 1) ? d1 * inv1 : lij1) : ((leader && i == j) ? d0 * inv0 : lij0);
#pragma unroll
                for (int m = p + 1; m < 16; ++m) {
                    const float c1 = fmaf(u10, ck0[m], ck1[m]);
                    b[m] = fmaf(t1, c1, fmaf(t0, ck0[m], b[m]));
                }
            }
            {
#pragma unroll
                for (int m = 0; m < 16; ++m) Bw[i * LS + 2 * m + h] = (!leader || 2 * m + h <= i) ? b[m] : 0.0f;
            }
        }
        LEAF_STAMP(1 + 2 * jb);
        __syncthreads();
        // ---- trailing sub-blocks: A[ib][kb] -= A[ib][jb] * A[kb][jb]^T, jb < kb <= ib ----
        {
            int cnt = 0;
            for (int ib = jb + 1; ib < 4; ++ib)
                for (int kb = jb + 1; kb <= ib; ++kb, ++cnt) {
                    if ((cnt & 3) != wave) continue;
                    float* Cik = Lb + blk(ib, kb) * BLK;
                    f32x16 acc = blk_load(Cik, lane);
                    acc = blk_mma<false>(Lb + blk(ib, jb) * BLK, Lb + blk(kb, jb) * BLK, acc, -1.0f, lane);
                    blk_store(Cik, acc, lane);
                }
        }
        __syncthreads();
        LEAF_STAMP(2 + 2 * jb);
    }

    // ---- the four diagonal inverses, one per wave: lane c owns column c of X = L^-1 ----
    // Column-oriented forward substitution: once x[k] is known every later row's sum takes its term, s[r] += L[r][k] x[k] --
    // independent FMAs (the row-oriented form is a dependent chain per row and ran 7.7k-12k cycles depending on how hipcc
    // scheduled its LDS reads); the dependent chain is one FMA + one multiply per k.
    // (Measured and dropped, round 5: a second accumulator Y = I in the LEADER that takes every step like a follower's block ends as
    // L^-1 and this phase disappears -- but a second MFMA per step costs the chain-carrying wave 85 cycles of matrix pipe
    // (scripts/micro/mfma_chain.hip: 128 -> 211 cycles a step), the column phases grew by more than the 8.5k cycles saved.)
    {
        const float* Djj = Lb + blk(wave, wave) * BLK;
        float* Xjj = Xb + blk(wave, wave) * BLK;
        float x[32], sacc[32], lcol[3][32];  // lcol: columns k, k+1, k+2 of L (requested two steps ahead of their use:
                                             // left alone, hipcc reads each column right before its FMAs and waits)
#pragma unroll
        for (int r = 0; r < 32; ++r) sacc[r] = 0.0f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = c + 1; r < 32; ++r) lcol[c][r] = Djj[r * LS + c];  // broadcast LDS reads
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            if (k + 2 < 32) {
#pragma unroll
                for (int r = k + 3; r < 32; ++r) lcol[(k + 2) % 3][r] = Djj[r * LS + k + 2];
            }
            __builtin_amdgcn_sched_barrier(0);
            const float pk = FORM == 1 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, invl), k)) : pinv[k];
            x[k] = (((i == k) ? 1.0f : 0.0f) - sacc[k]) * pk;
#pragma unroll
            for (int r = k + 1; r < 32; ++r) sacc[r] = fmaf(lcol[k % 3][r], x[k], sacc[r]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (lane < 32) {
#pragma unroll
            for (int k = 0; k < 32; ++k) Xjj[k * LS + i] = x[k];  // X[k][c = i]
        }
    }
    LEAF_STAMP(9);
    __syncthreads();

    // ---- assemble the 128x128 inverse.  With 64x64 halves, X = [[X_lo, 0], [-X_hi L_hl X_lo, X_hi]]: the off-diagonal 32x32
    // blocks of X_lo and X_hi first (X10, X32), together with the terms of T = L_hl X_lo that need neither; then the rest
    // of T; then X[2..3][0..1] = -X_hi T.  Six block products on the critical path and three barriers (the block-row
    // substitution this replaces: nine and six).  A wave reads back only scratch it wrote itself inside a phase (the LDS
    // executes one wave's operations in order). ----
    {
        auto L_ = [&](int ib, int jb) { return Lb + blk(ib, jb) * BLK; };
        auto X_ = [&](int ib, int jb) { return Xb + blk(ib, jb) * BLK; };
        float* T00 = Tb + 0 * BLK; float* T01 = Tb + 1 * BLK; float* T10 = Tb + 2 * BLK; float* T11 = Tb + 3 * BLK;
        float* S0 = Tb + 4 * BLK;  float* S1 = Tb + 5 * BLK;
        // phase 1
        if (wave == 0) {
            blk_store(S0, blk_mma<true>(L_(1, 0), X_(0, 0), zero16(), 1.0f, lane), lane);
            blk_store(X_(1, 0), blk_mma<true>(X_(1, 1), S0, zero16(), -1.0f, lane), lane);
        } else if (wave == 1) {
            blk_store(S1, blk_mma<true>(L_(3, 2), X_(2, 2), zero16(), 1.0f, lane), lane);
            blk_store(X_(3, 2), blk_mma<true>(X_(3, 3), S1, zero16(), -1.0f, lane), lane);
        } else if (wave == 2) {
            blk_store(T01, blk_mma<true>(L_(2, 1), X_(1, 1), zero16(), 1.0f, lane), lane);
            blk_store(T00, blk_mma<true>(L_(2, 0), X_(0, 0), zero16(), 1.0f, lane), lane);  // + L21 X10 in phase 2
        } else {
            blk_store(T11, blk_mma<true>(L_(3, 1), X_(1, 1), zero16(), 1.0f, lane), lane);
            blk_store(T10, blk_mma<true>(L_(3, 0), X_(0, 0), zero16(), 1.0f, lane), lane);  // + L31 X10 in phase 2
        }
        __syncthreads();
        // phase 2
        if (wave == 0) {
            blk_store(T00, blk_mma<true>(L_(2, 1), X_(1, 0), blk_load(T00, lane), 1.0f, lane), lane);
        } else if (wave == 1) {
            blk_store(T10, blk_mma<true>(L_(3, 1), X_(1, 0), blk_load(T10, lane), 1.0f, lane), lane);
        } else if (wave == 2) {
            blk_store(X_(2, 1), blk_mma<true>(X_(2, 2), T01, zero16(), -1.0f, lane), lane);
        } else {
            f32x16 q = blk_mma<true>(X_(3, 2), T01, zero16(), -1.0f, lane);
            blk_store(X_(3, 1), blk_mma<true>(X_(3, 3), T11, q, -1.0f, lane), lane);
        }
        __syncthreads();
        // phase 3
        if (wave == 0) {
            blk_store(X_(2, 0), blk_mma<true>(X_(2, 2), T00, zero16(), -1.0f, lane), lane);
        } else if (wave == 1) {
            f32x16 q = blk_mma<true>(X_(3, 2), T00, zero16(), -1.0f, lane);
            blk_store(X_(3, 0), blk_mma<true>(X_(3, 3), T10, q, -1.0f, lane), lane);
        }
        __syncthreads();
    }

    LEAF_STAMP(10);
    // ---- write back: L into the lower triangle of A, X (with its zero upper blocks) into dinv ----
#pragma unroll
    for (int b = 0; b < 16; ++b) {  // (unrolled: rolled up, every block waited for its own LDS and store round trips)
        const int ib = b >> 2, jb = b & 3;
        float4 xo = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jb <= ib) {
            const float* lp = Lb + blk(ib, jb) * BLK + lr * LS + lc;
            const float* xp = Xb + blk(ib, jb) * BLK + lr * LS + lc;
            xo = make_float4(xp[0], xp[1], xp[2], xp[3]);
            float* ap = A + (int64_t)(ib * 32 + lr) * ld + jb * 32 + lc;
            if (ib != jb || lc + 3 <= lr) {
                *reinterpret_cast<float4*>(ap) = make_float4(lp[0], lp[1], lp[2], lp[3]);
            } else {  // the 4-wide group straddles or lies above the diagonal: keep the caller's upper entries
                for (int k = 0; k < 4; ++k)
                    if (lc + k <= lr) ap[k] = lp[k];
            }
        }
        *reinterpret_cast<float4*>(dinv + (ib * 32 + lr) * 128 + jb * 32 + lc) = xo;
    }
    if (lane == 0 && nclamp > 0 && clamped != nullptr) atomicAdd(clamped, nclamp);
    LEAF_STAMP(11);
}

}  // namespace

int launch_potrf_leaf(float* a, int64_t ld, float* dinv_block, int32_t* clamped, float pivot_floor, hipStream_t s) {
    if (NNGP_KNOB(3) != 1 && NNGP_KNOB(3) != 2)
    {
        #ifdef NNGP_TIMING_KNOBS
        if (NNGP_KNOB(3) == 3)  // A/B: round 4's column phases (column pairs through an LDS ring, per-lane FMAs)
            hipLaunchKernelGGL(k_potrf_leaf_panel<0>, dim3(1), dim3(256), 0, s, a, ld, dinv_block, clamped, pivot_floor);
        else
#endif
            hipLaunchKernelGGL(k_potrf_leaf_panel<1>, dim3(1), dim3(256), 0, s, a, ld, dinv_block, clamped, pivot_floor);
#ifdef NNGP_TIMING_KNOBS
        if (NNGP_KNOB(7) == 8) {  // timing study: per wave, cycles from kernel start to the end of each phase
            unsigned long long h[64];
            (void)hipDeviceSynchronize();
            if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_leaf_stamps), sizeof(h)) == hipSuccess)
                for (int w = 0; w < 4; ++w) {
                    fprintf(stderr, "leaf wave %d: load %llu |", w, h[w * 16]);
                    for (int jb = 0; jb < 4; ++jb) fprintf(stderr, " F%d %llu U%d %llu |", jb, h[w * 16 + 1 + 2 * jb], jb, h[w * 16 + 2 + 2 * jb]);
                    fprintf(stderr, " inv %llu asm %llu wb %llu\n", h[w * 16 + 9], h[w * 16 + 10], h[w * 16 + 11]);
                }
        }
#endif
    }
    else if (NNGP_KNOB(3) != 1)  // variant 1 (scalarised broadcasts) measured 57 us vs 84 us for variant 0
        hipLaunchKernelGGL(k_potrf_leaf<1>, dim3(1), dim3(256), 0, s, a, ld, dinv_block, clamped, pivot_floor, NNGP_KNOB(0));
    else
        hipLaunchKernelGGL(k_potrf_leaf<0>, dim3(1), dim3(256), 0, s, a, ld, dinv_block, clamped, pivot_floor, NNGP_KNOB(0));
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

// B[m, n] <- B * L^-T.  L is the n x n lower factor at `l`; dinv holds its inverted diagonal blocks.
int trsm_rlt_f32(float* b, int64_t ldb, int64_t m, const float* l, int64_t ldl, const float* dinv, int64_t n,
                 hipStream_t s) {
    if (m <= 0 || n <= 0) return 0;
    if (n == TB) {
        // in place: C aliases A, one column tile (see gemm_f32.hip header)
        return launch_gemm_nt_f32(b, ldb, b, ldb, dinv, TB, m, TB, TB, 1.0f, 0.0f, false, s);
    }
    // up to 1024 columns: one fused launch, 32 rows per workgroup resident in LDS (trsm_panel.hip) instead of a recursion of
    // 2 n / 128 - 1 small GEMMs (debug key 2 = 4: the recursion, for A/B timing)
    if (n <= 1024 && m % 32 == 0 && NNGP_KNOB(2) != 4)
        return launch_trsm_panel_f32(b, ldb, m, l, ldl, dinv, n, nullptr, 0, 1.0f, s);
    const int64_t n1 = (n / TB / 2) * TB, n2 = n - n1;
    NNGP_TRY(trsm_rlt_f32(b, ldb, m, l, ldl, dinv, n1, s));
    // B2 -= B1 * L21^T,  L21 = L[n1:, :n1]
    NNGP_TRY(launch_gemm_nt_f32(b + n1, ldb, b, ldb, l + n1 * ldl, ldl, m, n2, n1, -1.0f, 1.0f, false, s));
    return trsm_rlt_f32(b + n1, ldb, m, l + n1 * ldl + n1, ldl, dinv + (n1 / TB) * TB * TB, n2, s);
}

// B[m, n] <- B * U^-T with U = L^T stored explicitly (`lt`, upper triangular, row-major); dinvt holds the
// TRANSPOSED inverted diagonal blocks.  Together with trsm_rlt_f32 this applies (L L^T)^-1 to the rows of B:
// Z = (B L^-T) L^-1.  Columns are resolved last-to-first; the update B1 -= X2 U12^T is again an NT GEMM.
int trsm_rut_f32(float* b, int64_t ldb, int64_t m, const float* lt, int64_t ldl, const float* dinvt, int64_t n,
                 hipStream_t s) {
    if (m <= 0 || n <= 0) return 0;
    if (n == TB) return launch_gemm_nt_f32(b, ldb, b, ldb, dinvt, TB, m, TB, TB, 1.0f, 0.0f, false, s);
    const int64_t n1 = (n / TB / 2) * TB, n2 = n - n1;
    NNGP_TRY(trsm_rut_f32(b + n1, ldb, m, lt + n1 * ldl + n1, ldl, dinvt + (n1 / TB) * TB * TB, n2, s));
    // B1 -= X2 * U12^T,  U12 = lt[0:n1, n1:n]
    NNGP_TRY(launch_gemm_nt_f32(b, ldb, b + n1, ldb, lt + n1, ldl, m, n1, n2, -1.0f, 1.0f, false, s));
    return trsm_rut_f32(b, ldb, m, lt, ldl, dinvt, n1, s);
}

int potrf_rec(float* a, int64_t n, int64_t ld, float* dinv, int32_t* clamped, float pivot_floor, hipStream_t s) {
    if (n == TB) return launch_potrf_leaf(a, ld, dinv, clamped, pivot_floor, s);
    const int64_t n1 = (n / TB / 2) * TB, n2 = n - n1;
    NNGP_TRY(potrf_rec(a, n1, ld, dinv, clamped, pivot_floor, s));
    float* a21 = a + n1 * ld;
    float* a22 = a21 + n1;
    NNGP_TRY(trsm_rlt_f32(a21, ld, n2, a, ld, dinv, n1, s));
    NNGP_TRY(launch_gemm_nt_f32(a22, ld, a21, ld, a21, ld, n2, n2, n1, -1.0f, 1.0f, true, s));
    return potrf_rec(a22, n2, ld, dinv + (n1 / TB) * TB * TB, clamped, pivot_floor, s);
}

int potrf_f32(float* a, int64_t n, int64_t ld, float* dinv, int32_t* clamped, float pivot_floor, hipStream_t s) {
    NNGP_REQUIRE(n > 0 && n % TB == 0, "potrf_f32: n must be a positive multiple of %d (got %lld)", TB, (long long)n);
    NNGP_REQUIRE(ld >= n && ld % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)dinv & 15) == 0,
                 "potrf_f32: matrix must be 16-byte aligned with ld >= n");
    return potrf_rec(a, n, ld, dinv, clamped, pivot_floor, s);
}

}  // namespace nngp
