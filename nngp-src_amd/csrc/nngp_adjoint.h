// Shared between the NNGP marginal likelihood (nngp_mll.hip) and the leave-one-out objectives (nngp_loo.hip): the handle both
// work on, the construction of A = K + r I, and the device code of the fused adjoint pass -- one pass over the lower 64 x 64
// tiles that contracts dK/dtheta with two seed matrices entry by entry, without ever forming dK/dtheta.
//
//   seeds of the marginal likelihood:   alpha_i alpha_j                             and  A^-1_ij
//   seeds of the leave-one-out loss:    1/2 (alpha_i u_j + u_i alpha_j)             and  C_ij = (A^-1 diag(bbar) A^-1)_ij
// Everything else -- tiling, Gram staging, forward recursion, reverse sweep, the q = 0 and exact-diagonal rules, the fixed-order
// reduction -- is one piece of code (adjoint_tile), so both objectives differentiate the same kernel.  Its stages are named
// device functions (tile_q_chain, gram_tile, entry_forward, entry_reverse, ard_sums, reduce_components), of which the rectangular
// pass of the sparse evidence (rect_tile, sparse_rect.h) is the second user: the layer recursion and its adjoint exist once.
// With per-feature input relevances (nngp_ard.hip) the same pass also leaves the seeded adjoints at the input of Dense layer 0
// behind (the ARD flag), from which one contraction with X gives the derivative with respect to every relevance.
#pragma once
#include "gp_f64.h"
#include "f64_math.h"
#include "trig_tab.h"

#include <cmath>
#include <type_traits>
#include <vector>

namespace nngp {

constexpr int MT = kGpTile;    // tile edge of the fused gradient pass
constexpr int MKC = 32;        // feature chunk staged in LDS
constexpr int MLD = MKC + 1;   // LDS row stride (odd: the 16 rows a wave reads sit in different banks)
constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxComp = 2 * NNGP_MAX_DENSE;  // gradient components of K
constexpr int kRed = 8;                       // scalar sums of k_mll_diag and the finish kernels (see nngp_mll::red)
constexpr int kRedLen = kRed + 4 + NNGP_MAX_DENSE + 2 * kMaxComp;
constexpr int kLooVec = 6;                    // vectors of nngp_mll::loo

struct MllArgs {
    const double* x;      // [n, d]
    const double* q;      // [n]: |x_i|^2 / d
    int64_t n;
    int d;
    const double* ainv;   // [Np, ld]: the matrix seed (A^-1, or C for the leave-one-out loss), lower triangle read
    int64_t ld;
    const double* alpha;  // [Np]
    const double* u;      // [Np]: A^-1 abar (leave-one-out loss only)
    double* part;         // [2 ncomp][nparts]: the rank-one / rank-two half of every component, then the matrix half
    int64_t nparts;
    // input relevances (nngp_ard.hip) only: the seeded adjoints at the input of Dense layer 0
    double* cmat;         // [Np, ldc]: kbar of the first seed at (i, j), of the matrix seed at (j, i), for j < i
    int64_t ldc;
    double* qbar;         // [2][tiles per side][np]: per seed the row sums of qbar1 / column sums of qbar2, one slot per tile
    int64_t np;
};

// The terms of the additive kernel over feature groups (nngp_mll_additive.hip): term 0 is the whole input, term t >= 1 group t - 1
struct AddTerms {
    int n_terms;
    const int* gbegin;    // [n_terms - 1]: the groups' feature ranges, zero-weight groups included
    const int* gend;
    const double* tw;     // [n_terms]: w0, then w_g
    double* tpart;        // [2 n_terms][nparts]: per term <seed 0, K^(t)> and <seed 1, K^(t)> of the tile
};

// ---- The pieces of a tile pass: the one copy of every stage that adjoint_tile (below, square, lower tiles) and rect_tile
// (sparse_rect.h, rectangular) share.  Each is called by the whole 256-thread workgroup of a 64 x 64 tile; thread tid holds the
// 16 entries (tr + 16 p, tc + 16 q), tc = tid & 15, tr = tid >> 4.  The LDS arrays belong to the tile function and come in by
// reference, the per-entry state by reference to register arrays; the order of every floating-point operation is fixed here.
// NLC: room for n_dense <= NLC layers (the per-entry state lives in registers, so its size must be known at compile time).

struct TileRows {
    const double* p;  // [n, d]
    int64_t n;        // rows from n on read as zero
    int64_t r0;       // the tile's first row
};

// what the reverse sweep of one entry holds once it has passed Dense layer 0: the adjoints of K0_ij, q_i and q_j, of the first
// seed (a) and of the matrix seed (i)
struct InputAdjoint {
    double kb_a, kb_i, q1a, q2a, q1i, q2i;
};

// The q chain of one of the tile's rows (tid < MT) or columns (tid < 2 MT), in the kernel build's order of operations:
// qs[l][tid] = q at the input of Dense layer l, rq[l][tid] = 1 / (4 pi q') with q' after it, 0 where q' = 0 (the q = 0 rule)
template <int NLC>
__device__ __forceinline__ void tile_q_chain(double q, const ArchDev& arch, double (&qs)[NLC][2 * MT], double (&rq)[NLC][2 * MT]) {
    const int tid = threadIdx.x, nd = arch.n_dense;
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

// The Gram tile gt[MT][MT + 1] (over sm) of rows `ra` against rows `rb` on the features [kb, ke): 32-feature chunks of both row
// panels staged in sm, 4 x 4 register accumulation with the features summed in order, gt = acc / (ke - kb).  SIDE: also both
// sides' sums of squares from the SAME staged values in the SAME order (qa: rows tr + 16 p, qb: columns tc + 16 p), unscaled.
// Returns 1 / (ke - kb); the caller's barrier comes before gt is read.
template <bool SIDE>
__device__ __forceinline__ double gram_tile(const TileRows& ra, const TileRows& rb, int d, int kb, int ke, double* sm,
                                            double (&qa)[SIDE ? 4 : 1], double (&qb)[SIDE ? 4 : 1]) {
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    double (*s1)[MLD] = reinterpret_cast<double (*)[MLD]>(sm);
    double (*s2)[MLD] = reinterpret_cast<double (*)[MLD]>(sm + MT * MLD);
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    if constexpr (SIDE) {
#pragma unroll
        for (int p = 0; p < 4; ++p) qa[p] = qb[p] = 0.0;
    }
    for (int k0 = kb; k0 < ke; k0 += MKC) {
        const int kc = ke - k0 < MKC ? ke - k0 : MKC;
        for (int e = tid; e < MT * MKC; e += 256) {
            const int r = e / MKC, k = e % MKC;
            const int64_t i = ra.r0 + r, j = rb.r0 + r;
            s1[r][k] = (k < kc && i < ra.n) ? ra.p[i * d + k0 + k] : 0.0;
            s2[r][k] = (k < kc && j < rb.n) ? rb.p[j * d + k0 + k] : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            double u[4], v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) u[p] = s1[tr + 16 * p][k];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = s2[tc + 16 * q][k];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(u[p], v[q], acc[p][q]);
            if constexpr (SIDE) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    qa[p] = fma(u[p], u[p], qa[p]);
                    qb[p] = fma(v[p], v[p], qb[p]);
                }
            }
        }
        __syncthreads();
    }
    double (*gt)[MT + 1] = reinterpret_cast<double (*)[MT + 1]>(sm);
    const double inv_d = 1.0 / (double)(ke - kb);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) gt[tr + 16 * p][tc + 16 * q] = acc[p][q] * inv_d;
    return inv_d;
}

__device__ __forceinline__ double gram_tile(const TileRows& ra, const TileRows& rb, int d, int kb, int ke, double* sm) {
    double none[1];
    return gram_tile<false>(ra, rb, d, kb, ke, sm, none, none);
}

// The forward layer recursion of entry (ri, cj) from k = K0_ij.  Per layer: kin = k into Dense l, ck = dK'/dk and cs = (b - a)^2 s
// of the activation after it.  DIAG && dg: the diagonal form (theta = 0 exactly; q q' - k^2 == 0 holds exactly, so K' has no q
// dependence); with DIAG = false no such branch exists.  VALUE: value = K_ij, k out of the last Dense layer (else untouched).
template <int NLC, bool DIAG, bool VALUE>
__device__ __forceinline__ void entry_forward(double k, bool dg, int ri, int cj, const ArchDev& arch, const double (&qs)[NLC][2 * MT],
                                              const double* tab, double (&kin)[NLC], double (&ck)[NLC], double (&cs)[NLC],
                                              double& value) {
    const int nd = arch.n_dense;
#pragma unroll
    for (int l = 0; l < NLC; ++l) {
        kin[l] = k;
        ck[l] = 0.0;
        cs[l] = 0.0;
        if constexpr (VALUE) {
            if (l == nd - 1) value = fma(arch.w2[l], k, arch.b2[l]);
        }
        if (l < nd - 1) {
            const double v = arch.w2[l], c = arch.b2[l];
            const bool ab = arch.act[l] == NNGP_ACT_ABRELU;
            k = fma(v, k, c);
            if (DIAG && dg) {  // theta = 0: K' = (a^2 + b^2) / 2 k  (1/2 for ReLU), no q dependence
                const double kd = ab ? arch.ap[l][2] : 0.5;
                k *= kd;
                ck[l] = kd;
            } else {
                const double q1 = fma(v, qs[l][ri], c), q2 = fma(v, qs[l][MT + cj], c);
                const double rr = fma(q1, q2, -k * k);
                const double s = rr > 0.0 ? fast_sqrt_pos(rr > 0.0 ? rr : 1.0) : 0.0;
                const double kr = pi_minus_atan2(s, k, tab) * (0.5 / kPi);  // kdot
                const double kk = fma(kr, k, s * (0.5 / kPi));
                // ABRelu's form is computed beside ReLU's and one of them chosen: a branch on ab would copy the per-layer arrays
                const double a0 = arch.ap[l][0], a1 = arch.ap[l][1];
                const double ka = fma(a0, k, a1 * kk), cka = fma(a1, kr, a0), csa = a1 * s;
                k = ab ? ka : kk;
                ck[l] = ab ? cka : kr;
                cs[l] = ab ? csa : s;
            }
        }
    }
}

// The reverse sweep of entry (ri, cj).  r comes in as the seeds (kb_a, kb_i; the four q adjoints zero) and leaves as what is left
// at the input of Dense layer 0; every Dense layer's two components are added into ga / gi on the way.
template <int NLC>
__device__ __forceinline__ void entry_reverse(InputAdjoint& r, int ri, int cj, const ArchDev& arch,
                                              const double (&qs)[NLC][2 * MT], const double (&rq)[NLC][2 * MT],
                                              const double (&kin)[NLC], const double (&ck)[NLC], const double (&cs)[NLC],
                                              double (&ga)[2 * NLC], double (&gi)[2 * NLC]) {
    const int nd = arch.n_dense;
    double &kb_a = r.kb_a, &kb_i = r.kb_i, &q1a = r.q1a, &q2a = r.q2a, &q1i = r.q1i, &q2i = r.q2i;
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
}

// ARD: the tile's sums of qbar1 over its columns and of qbar2 over its rows.  Every thread adds into slots of its own of
// rsum [seed][row][tc] / csum [seed][column][tr] in the order of its entries; ard_sums then gives thread tid the sum of the 16
// slots of array tid >> 6 (0, 1: row sums of seed 0, 1; 2, 3: column sums), row / column tid & 63.
using ArdSums = double[2][MT][17];

__device__ __forceinline__ void ard_sums_clear(ArdSums& rsum, ArdSums& csum) {
    for (int e = threadIdx.x; e < 2 * MT * 17; e += 256) (&rsum[0][0][0])[e] = (&csum[0][0][0])[e] = 0.0;
}

__device__ __forceinline__ double ard_sums(const ArdSums& rsum, const ArdSums& csum) {
    __syncthreads();
    const int arr = threadIdx.x >> 6, r = threadIdx.x & (MT - 1);
    const double* src = arr < 2 ? rsum[arr][r] : csum[arr - 2][r];
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) t += src[e];
    return t;
}

// The tile's 2 n_dense components of either seed, summed over the workgroup in a fixed order into the tile's slot of part
template <int NLC>
__device__ __forceinline__ void reduce_components(const double (&ga)[2 * NLC], const double (&gi)[2 * NLC], int nd, double* red,
                                                  double* part, int64_t nparts) {
    const int ncomp = 2 * nd;
#pragma unroll
    for (int c = 0; c < 2 * NLC; ++c) {
        if (c < ncomp) {  // uniform over the workgroup
            const double ra = block_sum(ga[c], red);
            const double rb = block_sum(gi[c], red);
            if (threadIdx.x == 0) {
                part[(int64_t)c * nparts + blockIdx.x] = ra;
                part[(int64_t)(ncomp + c) * nparts + blockIdx.x] = rb;
            }
        }
    }
}

// ---- The symmetric pass over the lower tiles ----
// LOO: the rank-two seed 1/2 (alpha_i u_j + u_i alpha_j) instead of alpha_i alpha_j.
// ARD: also keep what the reverse sweep holds once it has passed Dense layer 0 -- kbar = S_ij dK_ij/dK0_ij into cmat, and
// qbar1 = S_ij dK_ij/dq_i, qbar2 = S_ij dK_ij/dq_j summed over the tile's columns / rows into qbar.  Tile (ti, tj) writes its row
// part to slot tj and its column part to slot ti (a diagonal tile the sum of both), so every slot has one writer.  A diagonal
// entry depends on q_i alone (exact diagonal), so its kbar belongs to qbar.
// ADD: K = sum_t w_t K^(t) (include/nngp_additive_mll.h).  The tile is walked once per term, in the table's order: the term's Gram
// tile over its feature range with its own 1 / d_t, for a group also both slices' |x_t|^2 / d_t from the SAME staged values in the
// SAME order as the Gram entry (k_build_add's rule: identical slices give k == q == q' bit for bit and take the diagonal form,
// whose derivative goes through the k chain alone), the q chain, then per entry the forward recursion, the term's value times both
// seeds into the term's two halves, and -- unless w_t == 0 -- the reverse sweep from the seeds times w_t into the shared
// accumulators.  With one term of weight 1 every operation of the plain pass is repeated in its order.
template <int NLC, bool LOO, bool ARD = false, bool ADD = false>
__device__ __forceinline__ void adjoint_tile(const MllArgs& a, const ArchDev& arch, const AddTerms& add = AddTerms{}) {
    __shared__ __attribute__((aligned(16))) double sm[2 * MT * MLD];  // the two row panels, then the Gram tile [MT][MT + 1]
    __shared__ double qs[NLC][2 * MT];  // rows | columns: q at the input of Dense layer l
    __shared__ double rq[NLC][2 * MT];  // 1 / (4 pi q') with q' after Dense layer l; 0 where q' = 0 (the q = 0 rule)
    __shared__ __attribute__((aligned(16))) double tab[65 * 4];
    __shared__ double red[256];
    // ARD: [seed][row][tc] and [seed][column][tr] -- every thread sums into slots of its own, in the order of its entries
    __shared__ double rsum[ARD ? 2 : 1][ARD ? MT : 1][17], csum[ARD ? 2 : 1][ARD ? MT : 1][17];
    __shared__ double qg[ADD ? 2 * MT : 1];  // ADD: rows | columns, a group's |x_t|^2 / d_t
    static_assert(MT * (MT + 1) <= 2 * MT * MLD, "the Gram tile aliases the panels");
    static_assert(!(ARD && ADD), "relevances together with groups are not covered");
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    if constexpr (ARD) ard_sums_clear(rsum, csum);
    const int nd = arch.n_dense;
    const int64_t tn = (a.n + MT - 1) / MT;
    int64_t ti, tj;
    lower_tile(xcd_tile(blockIdx.x, tn * (tn + 1) / 2), &ti, &tj);
    const int64_t i0 = ti * MT, j0 = tj * MT;
    for (int e = tid; e < 65 * 4; e += 256) tab[e] = kTrigTab[e >> 2][e & 3];
    double (*gt)[MT + 1] = reinterpret_cast<double (*)[MT + 1]>(sm);
    double ga[2 * NLC], gi[2 * NLC];
    const int n_terms = ADD ? add.n_terms : 1;
    int t = 0;
    do {  // the terms; a do loop, with which the plain instantiations compile to the registers they had without it
        const bool grp = ADD && t > 0;  // a group's term: the slice's own q, the identical-slice rule
        int kb = 0, ke = a.d;
        [[maybe_unused]] double wt = 1.0;
        if constexpr (ADD) {
            wt = add.tw[t];
            if (grp) {
                kb = add.gbegin[t - 1];
                ke = add.gend[t - 1];
            }
        }
        if (!grp && tid < 2 * MT) {
            const int64_t g = tid < MT ? i0 + tid : j0 + tid - MT;
            tile_q_chain<NLC>(g < a.n ? a.q[g] : 0.0, arch, qs, rq);
        }

        // ---- Gram tile: rows i0 + tr + 16 p, columns j0 + tc + 16 q, features summed in order ----
        [[maybe_unused]] double qa[ADD ? 4 : 1], qb[ADD ? 4 : 1];
        [[maybe_unused]] const double inv_d = gram_tile<ADD>(TileRows{a.x, a.n, i0}, TileRows{a.x, a.n, j0}, a.d, kb, ke, sm, qa, qb);
        if constexpr (ADD) {
            if (grp) {  // every row / column of the tile has 16 threads with the same sums: one of them writes
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (tc == 0) qg[tr + 16 * p] = qa[p] * inv_d;
                    if (tr == 0) qg[MT + tc + 16 * p] = qb[p] * inv_d;
                }
            }
        }
        __syncthreads();
        if constexpr (ADD) {
            if (grp) {
                if (tid < 2 * MT) tile_q_chain<NLC>(qg[tid], arch, qs, rq);
                __syncthreads();
            }
        }

        // ---- per entry: forward recursion, then the adjoint sweep from both seeds ----
        if (t == 0) {  // the accumulators are shared by all terms
#pragma unroll
            for (int c = 0; c < 2 * NLC; ++c) ga[c] = gi[c] = 0.0;
        }
        [[maybe_unused]] double ha = 0.0, hi = 0.0;  // ADD: the term's value against either seed
#pragma unroll 1
        for (int e = 0; e < 16; ++e) {
            const int ri = tr + 16 * (e >> 2), cj = tc + 16 * (e & 3);
            const int64_t i = i0 + ri, j = j0 + cj;
            if (i >= a.n || j > i) continue;  // padding, and the upper half of a diagonal tile (j <= i < n for every other entry)
            // a group's term takes the diagonal form wherever both slices give k == q == q' bit for bit (the diagonal does)
            const bool dg = grp ? (qs[0][ri] == gt[ri][cj] && qs[0][MT + cj] == gt[ri][cj]) : i == j;
            const double w = i == j ? 1.0 : 2.0;  // the lower triangle stands for the whole square
            InputAdjoint r{0.0, w * a.ainv[i * a.ld + j], 0.0, 0.0, 0.0, 0.0};  // the seeds
            if constexpr (LOO) r.kb_a = w * (0.5 * (a.alpha[i] * a.u[j] + a.u[i] * a.alpha[j]));
            else r.kb_a = w * (a.alpha[i] * a.alpha[j]);
            const double k = dg ? qs[0][ri] : gt[ri][cj];  // exact diagonal: q q' - k^2 == 0 holds exactly
            double kin[NLC], ck[NLC], cs[NLC];
            [[maybe_unused]] double val = 0.0;  // ADD: K^(t)_ij
            entry_forward<NLC, true, ADD>(k, dg, ri, cj, arch, qs, tab, kin, ck, cs, val);
            if constexpr (ADD) {
                ha = fma(r.kb_a, val, ha);
                hi = fma(r.kb_i, val, hi);
                if (wt == 0.0) continue;  // the term is not in K: its own d/dw_t only
                r.kb_a *= wt;
                r.kb_i *= wt;
            }
            entry_reverse<NLC>(r, ri, cj, arch, qs, rq, kin, ck, cs, ga, gi);
            if constexpr (ARD) {
                if (dg) {
                    rsum[0][ri][tc] += r.kb_a;
                    rsum[1][ri][tc] += r.kb_i;
                } else {
                    a.cmat[i * a.ldc + j] = r.kb_a;
                    a.cmat[j * a.ldc + i] = r.kb_i;
                    rsum[0][ri][tc] += r.q1a;
                    rsum[1][ri][tc] += r.q1i;
                    csum[0][cj][tr] += r.q2a;
                    csum[1][cj][tr] += r.q2i;
                }
            }
        }
        if constexpr (ARD) {
            const double t = ard_sums(rsum, csum);
            const int arr = tid >> 6, r = tid & (MT - 1);  // 0, 1: row sums of seed 0, 1; 2, 3: column sums
            red[tid] = t;
            __syncthreads();
            if (ti == tj) {
                if (tid < 2 * MT) a.qbar[((int64_t)arr * tn + ti) * a.np + i0 + r] = red[tid] + red[tid + 2 * MT];
            } else {
                a.qbar[((int64_t)(arr & 1) * tn + (arr < 2 ? tj : ti)) * a.np + (arr < 2 ? i0 : j0) + r] = t;
            }
            __syncthreads();
        }
        if constexpr (ADD) {  // the term's halves, one slot per (term, tile); the barriers also free the panels for the next term
            const double ra = block_sum(ha, red);
            const double rb = block_sum(hi, red);
            if (tid == 0) {
                add.tpart[(int64_t)(2 * t) * a.nparts + blockIdx.x] = ra;
                add.tpart[(int64_t)(2 * t + 1) * a.nparts + blockIdx.x] = rb;
            }
        }
    } while (ADD && ++t < n_terms);
    reduce_components<NLC>(ga, gi, nd, red, a.part, a.nparts);
}

// out[e] = sum_i q_i^(e), the diagonal's q at the input of Dense layer e (one workgroup, fixed order): tr dK/dtheta follows from
// these in closed form (trace_dk)
// q_of(i): the diagonal's q at the input of Dense layer 0
template <class Q>
__device__ __forceinline__ void finish_qsums_of(Q q_of, int64_t n, const ArchDev& arch, double* red, double* out) {
    const int nd = arch.n_dense;
    double sq[NNGP_MAX_DENSE];
#pragma unroll
    for (int e = 0; e < NNGP_MAX_DENSE; ++e) sq[e] = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        double z = q_of(i);
#pragma unroll
        for (int e = 0; e < NNGP_MAX_DENSE; ++e) {
            if (e < nd) {
                sq[e] += z;
                const double zp = fma(arch.w2[e], z, arch.b2[e]);
                if (e < nd - 1) z = arch.act[e] == NNGP_ACT_ABRELU ? arch.ap[e][2] * zp : 0.5 * zp;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NNGP_MAX_DENSE; ++e) {
        if (e < nd) {
            const double r = block_sum(sq[e], red);
            if (threadIdx.x == 0) out[e] = r;
        }
    }
}

__device__ __forceinline__ void finish_qsums(const double* q, int64_t n, const ArchDev& arch, double* red, double* out) {
    finish_qsums_of([q](int64_t i) { return q[i]; }, n, arch, red, out);
}

// tr dK / dtheta from the diagonal's closed form: K_ii = u_{nd-1}, u_l = v_l z_l + c_l, z_{l+1} = h_l u_l, so
// dK_ii / du_l = prod_{m >= l, hidden} h_m prod_{m > l} v_m =: D_l and tr dK/dv_l = D_l sum_i z_l,i, tr dK/dc_l = D_l N
inline void trace_dk(const ArchDev& arch, const double* sq, double dn, double* trdk) {
    const int nd = arch.n_dense;
    double dl = 1.0;
    for (int l = nd - 1; l >= 0; --l) {
        if (l < nd - 1) dl *= arch.act[l] == NNGP_ACT_ABRELU ? arch.ap[l][2] : 0.5;
        trdk[2 * l] = dl * sq[l];
        trdk[2 * l + 1] = dl * dn;
        dl *= arch.w2[l];
    }
}

// dK_ii / dq_i, q_i the diagonal's q at the input of Dense layer 0: D_0 v_0 of trace_dk
inline double diag_q_slope(const ArchDev& arch) {
    const int nd = arch.n_dense;
    double d0v0 = 1.0;
    for (int l = nd - 1; l >= 0; --l) {
        if (l < nd - 1) d0v0 *= arch.act[l] == NNGP_ACT_ABRELU ? arch.ap[l][2] : 0.5;
        d0v0 *= arch.w2[l];
    }
    return d0v0;
}

// the d relevances of a caller (host): every one finite and non-negative, or rc -2 naming `who`
inline int check_relevances(const char* who, const double* s, int d) {
    for (int k = 0; k < d; ++k)
        NNGP_REQUIRE(std::isfinite(s[k]) && s[k] >= 0.0, "%s: relevance %d must be finite and non-negative (%g)", who, k, s[k]);
    return 0;
}

}  // namespace nngp

namespace nngp {
// What nngp_mll_reserve_ard adds to the handle (include/nngp_ard.h); all NULL / empty on a handle without relevances
struct ArdBuffers {
    bool reserved = false;
    double* xs = nullptr;     // n_cap x d: x scaled by sqrt(s), what the kernel build and the adjoint pass read
    double* q = nullptr;      // n_cap: |xs_i|^2 / d
    double* s = nullptr;      // d: the relevances
    double* qbar = nullptr;   // [2][tiles per side][np_cap]: MllArgs::qbar
    double* part = nullptr;   // [3][tiles per side][d]: per row block the contraction of either seed, and sum x_ik^2
    double* out = nullptr;    // [3][d]: these summed over the row blocks
    std::vector<double> host;   // out on the host
    std::vector<double> terms;  // nngp_mll_ard_terms: both halves per feature, then tr dK/ds_k
    bool have_terms = false;
};
// What nngp_mll_reserve_additive adds to the handle (include/nngp_additive_mll.h); empty on a handle without a group table
struct AddBuffers {
    bool reserved = false;
    int n_terms = 0;              // T = 1 + n_groups, zero-weight groups included
    int* range = nullptr;         // device [4 G]: begin, end of every group; then begin, end of the groups with w_g > 0 (the build's)
    double* weight = nullptr;     // device [T + G]: w0, w_g; then the w_g > 0 (the build's table)
    double* red = nullptr;        // device [T (2 + NNGP_MAX_DENSE)]: the term halves summed over the tiles, then per term sum_i z_l,i
    GroupsDev dev{};              // the build's table of the current evaluation (points into range / weight)
    std::vector<int> range_host;
    std::vector<double> weight_host, red_host;
    std::vector<double> terms;    // nngp_mll_additive_terms
    bool have_terms = false;
};
}  // namespace nngp

// The handle of include/nngp_mll.h, include/nngp_loo.h and include/nngp_ard.h
struct nngp_mll {
    nngp::GpWorkspace w;      // part: 2 kMaxComp per tile; red: [0, 2) tr K, r; [kRed, ...) the finish kernels' sums
    double* q = nullptr;      // n_cap: |x_i|^2 / d
    double* loo = nullptr;    // kLooVec x np_cap: -b, abar, bbar, u, the leave-one-out means and variances
    int n_dense = 0;
    bool have_terms = false;
    double terms[2 * (nngp::kMaxComp + 1) + 5 + nngp::kMaxComp] = {};
    int n_terms = 0;
    int loo_get = 0;          // NNGP_GET_* of the last leave-one-out evaluation (0: none, or the data changed since)
    bool have_loo_terms = false;
    double loo_terms[2 * (nngp::kMaxComp + 1) + 3 + nngp::kMaxComp] = {};
    int n_loo_terms = 0;
    nngp::ArdBuffers ard;
    nngp::AddBuffers add;
};

namespace nngp {
// The one ladder from n_dense to the NLC a tile pass is instantiated for.  launch(std::integral_constant<int, NLC>{}, grid)
// launches the pass's kernel on `grid`, one workgroup per tile; who prefixes the error.
template <class Launch>
int launch_by_nlc(const ArchDev& arch, int64_t nparts, const char* who, Launch launch) {
    NNGP_REQUIRE(nparts < 2147483647LL, "%s: gradient grid too large", who);
    const dim3 grid((unsigned)nparts);
    if (arch.n_dense <= 2) launch(std::integral_constant<int, 2>{}, grid);
    else if (arch.n_dense <= 4) launch(std::integral_constant<int, 4>{}, grid);
    else if (arch.n_dense <= 8) launch(std::integral_constant<int, 8>{}, grid);
    else launch(std::integral_constant<int, NNGP_MAX_DENSE>{}, grid);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}
// The two symmetric passes that the sparse evidence runs over K_uu as well, both handle-free: the plain pass (nngp_mll.hip,
// k_nngp_mll_partial) and the pass with ARD set (nngp_ard.hip, k_nngp_ard_partial; a.cmat / a.qbar filled in by the caller)
int launch_mll_partial(const MllArgs& a, const ArchDev& arch, hipStream_t s);
int launch_ard_partial(const MllArgs& a, const ArchDev& arch, bool loo, hipStream_t s);
// What follows the pass with ARD set, handle-free as well (nngp_ard.hip, k_ard_contract and k_ard_finish): cmat [., ldc] and
// qbar [2][tiles per side][np] as that pass left them, x [n, d] the raw rows, part [3][tiles per side][d] scratch; out [3][d]
int launch_ard_contract(const double* cmat, int64_t ldc, const double* x, int64_t n, int d, const double* qbar, int64_t np, double* part,
                        double* out, hipStream_t s);
// nngp_mll.hip: the architecture checked for the float64 gradient paths (rc -2 naming `who`), and A = K + r I (get: NNGP_GET_NNGP,
// or NNGP_GET_NTK for Theta + r I) in w.a with the identity on the padding; red[0] = tr K, red[1] = r
// x, q: the inputs and their row norms (the handle's own, or the scaled copy of ArdBuffers)
int mll_make_arch(const nngp_arch_act* arch_in, double diag_reg, const char* who, ArchDev* arch);
int mll_build_a(nngp_mll* h, const ArchDev& arch, int get, double diag_reg, int absolute, const double* x, const double* q,
                hipStream_t s);
// The evaluations behind nngp_mll_evaluate / nngp_mll_loo_evaluate and their _ard forms.  rel: host, d relevances, or NULL for
// the handle's own x (then grad_s is NULL too); grad_s: host, d values, or NULL.
// weights: host, the 1 + n_groups term weights of the additive kernel (then rel is NULL), or NULL for the plain kernel; grad_w: host,
// as many values, or NULL.
int mll_evaluate_core(nngp_mll* h, const nngp_arch_act* arch_in, double diag_reg, int absolute, double* nlml, double* grad,
                      const double* rel, double* grad_s, const char* who, hipStream_t s, const double* weights = nullptr,
                      double* grad_w = nullptr);
int loo_evaluate_core(nngp_mll* h, const nngp_arch_act* arch_in, int get, double diag_reg, int absolute, int objective, double* value,
                      double* grad, const double* rel, double* grad_s, const char* who, hipStream_t s);
// nngp_ard.hip.  ard_begin: checks rel, uploads it, fills ard.xs and ard.q.  launch_ard_partial(h, ...): the adjoint pass with ARD set
// (a.cmat / a.qbar filled in from the handle, then the handle-free launcher above).  ard_contract: the contraction and its finish into ard.out, queued for the host
// copy ard.host.  ard_finish_host (after the stream is synchronised): grad_s and the terms from ard.host; s1, s2 multiply
// lambda tr dK / N in the two halves (alpha^T alpha, tr A^-1; or alpha^T u, tr C), loo picks -(h1 + h2) over -h1/2 + h2/2.
int ard_begin(nngp_mll* h, const double* rel, const char* who, hipStream_t s);
int launch_ard_partial(nngp_mll* h, MllArgs a, const ArchDev& arch, bool loo, hipStream_t s);
int ard_contract(nngp_mll* h, hipStream_t s);
void ard_finish_host(nngp_mll* h, const ArchDev& arch, double diag_reg, int absolute, double s1, double s2, bool loo, double* grad_s);
void ard_free(nngp_mll* h);
// nngp_mll_additive.hip.  add_begin: checks the weights, uploads them and the build's table; *groups is that table, or NULL when
// it is the plain kernel (no group, w0 = 1).  launch_add_partial: the adjoint pass with ADD set, its term partials over L^-T.
// launch_add_finish: the fixed-order sums of the plain finish kernel (their bits) and of the term partials, over several
// workgroups, and the per-term sums of the diagonal's q chain; queues the host copy.  add_trace_dk (after the stream is
// synchronised): tr dK/dtheta_p = sum_t w_t tr dK^(t)/dtheta_p.  add_finish_host: grad_w and the terms; aa = alpha^T alpha.
int add_begin(nngp_mll* h, const double* weights, const char* who, const GroupsDev** groups, hipStream_t s);
int launch_add_partial(nngp_mll* h, const MllArgs& a, const ArchDev& arch, hipStream_t s);
int launch_add_finish(nngp_mll* h, const ArchDev& arch, int64_t nparts, hipStream_t s);
void add_trace_dk(const nngp_mll* h, const ArchDev& arch, double dn, double* trdk);
void add_finish_host(nngp_mll* h, const ArchDev& arch, double diag_reg, int absolute, double aa, double tr_ainv, double* grad_w);
void add_free(nngp_mll* h);
}  // namespace nngp
