// The rectangular adjoint pass of the sparse evidence (sparse_evidence.hip) as device code shared with the relevance gradient
// (sparse_ard.hip): one workgroup per 64 x 64 tile of (rows of X_c) x (rows of U), mirroring adjoint_tile of nngp_adjoint.h but
// with every entry counted once and no exact-diagonal rule.  With ARD set the pass also leaves behind what its reverse sweep
// holds once it has passed Dense layer 0 -- the seeded adjoints of K0_ij, q_i and q_j -- for the contraction with the raw rows.
#pragma once
#include "nngp_adjoint.h"

namespace nngp {

struct RectArgs {
    const double* x;      // [c, d]
    const double* xq;     // [c]: |x_i|^2 / d
    int64_t c;
    const double* u;      // [m, d]
    const double* uq;     // [m]
    int64_t m;
    int d;
    const double* seed;   // [c, ld]: D
    int64_t ld;
    const double* beta;   // [c]
    const double* gamma;  // [m]
    double* part;         // [2 ncomp][nparts]: the beta gamma^T half of every component, then the D half
    int64_t nparts;       // tiles: ceil(c / 64) * tu
    int64_t tu;           // tiles along the inducing rows
    // input relevances (sparse_ard.hip) only: the seeded adjoints at the input of Dense layer 0
    double* kb_i;         // [c, ld]: kbar of the dense seed, in place over `seed` (D_c is dead once its entry is read)
    double* kb_a;         // [c, ld]: kbar of the rank-one seed
    double* qrow;         // [2][tu][cp]: per seed the tile's sums of qbar1 over its columns, slot = the tile's column index
    int64_t cp;
    double* qcol;         // [2][row tiles][mpc]: per seed the tile's sums of qbar2 over its rows, slot = the tile's row index
    int64_t tr;           // row tiles: ceil(c / 64)
    int64_t mpc;
};

// ARD: also keep kbar = S_ij dK_ij/dK0_ij (both seeds) and the sums of qbar1 = S_ij dK_ij/dq_i over the tile's columns and of
// qbar2 = S_ij dK_ij/dq_j over its rows, laid out as adjoint_tile's rsum / csum: every thread sums into slots of its own in the
// order of its entries, and every global slot has one writer.  The ARD = false instantiation is the pass as it was.
// Static LDS with ARD at NLC = 16: 33 792 (panels) + 32 768 (qs, rq) + 2 080 + 2 048 + 34 816 (rsum, csum) = 105 504 bytes, as
// adjoint_tile<16, ., true>; within gfx950's 160 KiB per workgroup, above the 64 KiB of older parts.
template <int NLC, bool ARD = false>
__device__ __forceinline__ void rect_tile(const RectArgs& a, const ArchDev& arch) {
    __shared__ __attribute__((aligned(16))) double sm[2 * MT * MLD];  // the two row panels, then the Gram tile [MT][MT + 1]
    __shared__ double qs[NLC][2 * MT];  // rows | columns: q at the input of Dense layer l
    __shared__ double rq[NLC][2 * MT];  // 1 / (4 pi q') with q' after Dense layer l; 0 where q' = 0 (the q = 0 rule)
    __shared__ __attribute__((aligned(16))) double tab[65 * 4];
    __shared__ double red[256];
    __shared__ double rsum[ARD ? 2 : 1][ARD ? MT : 1][17], csum[ARD ? 2 : 1][ARD ? MT : 1][17];
    static_assert(sizeof(double) * (2 * MT * MLD + 4 * NLC * MT + 65 * 4 + 256 + (ARD ? 4 * MT * 17 : 2 * 17)) <= 160 * 1024,
                  "static LDS beyond a gfx950 workgroup's 160 KiB");
    static_assert(MT * (MT + 1) <= 2 * MT * MLD, "the Gram tile aliases the panels");
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    if constexpr (ARD) {
        for (int e = tid; e < 2 * MT * 17; e += 256) (&rsum[0][0][0])[e] = (&csum[0][0][0])[e] = 0.0;
    }
    const int nd = arch.n_dense;
    const int64_t t = xcd_tile(blockIdx.x, a.nparts);
    const int64_t i0 = (t / a.tu) * MT, j0 = (t % a.tu) * MT;
    for (int e = tid; e < 65 * 4; e += 256) tab[e] = kTrigTab[e >> 2][e & 3];
    if (tid < 2 * MT) {  // the q chain of the tile's rows and columns, in the kernel build's order of operations
        double q;
        if (tid < MT) q = i0 + tid < a.c ? a.xq[i0 + tid] : 0.0;
        else q = j0 + tid - MT < a.m ? a.uq[j0 + tid - MT] : 0.0;
#pragma unroll
        for (int l = 0; l < NLC; ++l) {
            if (l < nd) {
                qs[l][tid] = q;
                const double qp = fma(arch.w2[l], q, arch.b2[l]);
                rq[l][tid] = qp > 0.0 ? 1.0 / (4.0 * kPi * qp) : 0.0;
                if (l < nd - 1) q = arch.act[l] == NNGP_ACT_ABRELU ? arch.ap[l][2] * qp : 0.5 * qp;
            }
        }
    }

    // ---- Gram tile: rows i0 + tr + 16 p of X_c, columns j0 + tc + 16 q of U, features summed in order ----
    double (*s1)[MLD] = reinterpret_cast<double (*)[MLD]>(sm);
    double (*s2)[MLD] = reinterpret_cast<double (*)[MLD]>(sm + MT * MLD);
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    for (int k0 = 0; k0 < a.d; k0 += MKC) {
        const int kc = a.d - k0 < MKC ? a.d - k0 : MKC;
        for (int e = tid; e < MT * MKC; e += 256) {
            const int r = e / MKC, k = e % MKC;
            const int64_t i = i0 + r, j = j0 + r;
            s1[r][k] = (k < kc && i < a.c) ? a.x[i * a.d + k0 + k] : 0.0;
            s2[r][k] = (k < kc && j < a.m) ? a.u[j * a.d + k0 + k] : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            double uu[4], vv[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) uu[p] = s1[tr + 16 * p][k];
#pragma unroll
            for (int q = 0; q < 4; ++q) vv[q] = s2[tc + 16 * q][k];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(uu[p], vv[q], acc[p][q]);
        }
        __syncthreads();
    }
    double (*gt)[MT + 1] = reinterpret_cast<double (*)[MT + 1]>(sm);
    const double inv_d = 1.0 / (double)a.d;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) gt[tr + 16 * p][tc + 16 * q] = acc[p][q] * inv_d;
    __syncthreads();

    // ---- per entry: forward recursion, then the adjoint sweep from both seeds ----
    double ga[2 * NLC], gi[2 * NLC];
#pragma unroll
    for (int c = 0; c < 2 * NLC; ++c) ga[c] = gi[c] = 0.0;
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const int ri = tr + 16 * (e >> 2), cj = tc + 16 * (e & 3);
        const int64_t i = i0 + ri, j = j0 + cj;
        if (i >= a.c || j >= a.m) continue;  // the tile's tails
        double kb_a = a.beta[i] * a.gamma[j];
        double kb_i = a.seed[i * a.ld + j];
        double k = gt[ri][cj];
        double kin[NLC], ck[NLC], cs[NLC];  // per layer: k into Dense l; dK'/dk and (b - a)^2 s of the activation after it
#pragma unroll
        for (int l = 0; l < NLC; ++l) {
            kin[l] = k;
            ck[l] = 0.0;
            cs[l] = 0.0;
            if (l < nd - 1) {
                const double v = arch.w2[l], c = arch.b2[l];
                const bool ab = arch.act[l] == NNGP_ACT_ABRELU;
                k = fma(v, k, c);
                const double q1 = fma(v, qs[l][ri], c), q2 = fma(v, qs[l][MT + cj], c);
                const double rr = fma(q1, q2, -k * k);
                const double s = rr > 0.0 ? fast_sqrt_pos(rr > 0.0 ? rr : 1.0) : 0.0;
                const double kr = pi_minus_atan2(s, k, tab) * (0.5 / kPi);  // kdot
                const double kk = fma(kr, k, s * (0.5 / kPi));
                if (ab) {
                    k = fma(arch.ap[l][0], k, arch.ap[l][1] * kk);
                    ck[l] = fma(arch.ap[l][1], kr, arch.ap[l][0]);
                    cs[l] = arch.ap[l][1] * s;
                } else {
                    k = kk;
                    ck[l] = kr;
                    cs[l] = s;
                }
            }
        }
        double q1a = 0.0, q2a = 0.0, q1i = 0.0, q2i = 0.0;
#pragma unroll
        for (int l = NLC - 1; l >= 0; --l) {
            if (l < nd) {
                if (l < nd - 1) {  // the activation after Dense layer l: dK'/dq1 = (b - a)^2 s / (4 pi q1'), q' = h q
                    const double h = arch.act[l] == NNGP_ACT_ABRELU ? arch.ap[l][2] : 0.5;
                    const double t1 = cs[l] * rq[l][ri], t2 = cs[l] * rq[l][MT + cj];
                    q1a = fma(kb_a, t1, h * q1a);
                    q2a = fma(kb_a, t2, h * q2a);
                    kb_a *= ck[l];
                    q1i = fma(kb_i, t1, h * q1i);
                    q2i = fma(kb_i, t2, h * q2i);
                    kb_i *= ck[l];
                }
                // Dense layer l: k' = v k + c (likewise q1, q2)
                const double v = arch.w2[l], x1 = qs[l][ri], x2 = qs[l][MT + cj];
                ga[2 * l] += fma(kb_a, kin[l], fma(q1a, x1, q2a * x2));
                ga[2 * l + 1] += kb_a + q1a + q2a;
                gi[2 * l] += fma(kb_i, kin[l], fma(q1i, x1, q2i * x2));
                gi[2 * l + 1] += kb_i + q1i + q2i;
                kb_a *= v;
                q1a *= v;
                q2a *= v;
                kb_i *= v;
                q1i *= v;
                q2i *= v;
            }
        }
        if constexpr (ARD) {
            a.kb_a[i * a.ld + j] = kb_a;
            a.kb_i[i * a.ld + j] = kb_i;
            rsum[0][ri][tc] += q1a;
            rsum[1][ri][tc] += q1i;
            csum[0][cj][tr] += q2a;
            csum[1][cj][tr] += q2i;
        }
    }
    if constexpr (ARD) {
        __syncthreads();
        const int arr = tid >> 6, r = tid & (MT - 1);  // 0, 1: row sums of seed 0, 1; 2, 3: column sums
        const double* src = arr < 2 ? rsum[arr][r] : csum[arr - 2][r];
        double sum = 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e) sum += src[e];
        if (arr < 2) a.qrow[((int64_t)arr * a.tu + t % a.tu) * a.cp + i0 + r] = sum;
        else a.qcol[((int64_t)(arr - 2) * a.tr + t / a.tu) * a.mpc + j0 + r] = sum;
    }
    const int ncomp = 2 * nd;
#pragma unroll
    for (int c = 0; c < 2 * NLC; ++c) {
        if (c < ncomp) {  // uniform over the workgroup
            const double ra = block_sum(ga[c], red);
            const double rb = block_sum(gi[c], red);
            if (tid == 0) {
                a.part[(int64_t)c * a.nparts + blockIdx.x] = ra;
                a.part[(int64_t)(ncomp + c) * a.nparts + blockIdx.x] = rb;
            }
        }
    }
}

}  // namespace nngp
