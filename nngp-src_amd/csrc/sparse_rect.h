// The rectangular adjoint pass of the sparse evidence (sparse_evidence.hip) as device code shared with the relevance gradient
// (sparse_ard.hip): one workgroup per 64 x 64 tile of (rows of X_c) x (rows of U).  Every stage -- q chain, Gram tile, forward
// recursion, reverse sweep, the reductions -- is the piece of nngp_adjoint.h that adjoint_tile runs; what is this tile's own is
// the tile index, the two row sources, the tails, the seeds, that every entry counts once with no exact-diagonal rule, and where
// the ARD left-overs go.  With ARD set the pass also leaves behind what its reverse sweep holds once it has passed Dense layer
// 0 -- the seeded adjoints of K0_ij, q_i and q_j -- for the contraction with the raw rows.
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
// qbar2 = S_ij dK_ij/dq_j over its rows (ard_sums); every global slot has one writer.
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
    if constexpr (ARD) ard_sums_clear(rsum, csum);
    const int64_t t = xcd_tile(blockIdx.x, a.nparts);
    const int64_t i0 = (t / a.tu) * MT, j0 = (t % a.tu) * MT;
    for (int e = tid; e < 65 * 4; e += 256) tab[e] = kTrigTab[e >> 2][e & 3];
    if (tid < 2 * MT) {
        double q;
        if (tid < MT) q = i0 + tid < a.c ? a.xq[i0 + tid] : 0.0;
        else q = j0 + tid - MT < a.m ? a.uq[j0 + tid - MT] : 0.0;
        tile_q_chain<NLC>(q, arch, qs, rq);
    }
    // rows i0 + tr + 16 p of X_c against columns j0 + tc + 16 q of U
    gram_tile(TileRows{a.x, a.c, i0}, TileRows{a.u, a.m, j0}, a.d, 0, a.d, sm);
    double (*gt)[MT + 1] = reinterpret_cast<double (*)[MT + 1]>(sm);
    __syncthreads();

    double ga[2 * NLC], gi[2 * NLC];
#pragma unroll
    for (int c = 0; c < 2 * NLC; ++c) ga[c] = gi[c] = 0.0;
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const int ri = tr + 16 * (e >> 2), cj = tc + 16 * (e & 3);
        const int64_t i = i0 + ri, j = j0 + cj;
        if (i >= a.c || j >= a.m) continue;  // the tile's tails
        // a training row that is also an inducing row takes the general formula, as in the cross build
        InputAdjoint r{a.beta[i] * a.gamma[j], a.seed[i * a.ld + j], 0.0, 0.0, 0.0, 0.0};  // the seeds
        double kin[NLC], ck[NLC], cs[NLC], none;
        entry_forward<NLC, false, false>(gt[ri][cj], false, ri, cj, arch, qs, tab, kin, ck, cs, none);
        entry_reverse<NLC>(r, ri, cj, arch, qs, rq, kin, ck, cs, ga, gi);
        if constexpr (ARD) {
            a.kb_a[i * a.ld + j] = r.kb_a;
            a.kb_i[i * a.ld + j] = r.kb_i;
            rsum[0][ri][tc] += r.q1a;
            rsum[1][ri][tc] += r.q1i;
            csum[0][cj][tr] += r.q2a;
            csum[1][cj][tr] += r.q2i;
        }
    }
    if constexpr (ARD) {
        const double sum = ard_sums(rsum, csum);
        const int arr = tid >> 6, r = tid & (MT - 1);  // 0, 1: row sums of seed 0, 1; 2, 3: column sums
        if (arr < 2) a.qrow[((int64_t)arr * a.tu + t % a.tu) * a.cp + i0 + r] = sum;
        else a.qcol[((int64_t)(arr - 2) * a.tr + t / a.tu) * a.mpc + j0 + r] = sum;
    }
    reduce_components<NLC>(ga, gi, arch.n_dense, red, a.part, a.nparts);
}

}  // namespace nngp
