/* nngp_sparse_ard.h -- per-feature input relevances (ARD) on the sparse (inducing-point) NNGP, on the nngp_sparse handle of
 * nngp_sparse.h in libnngp_hip.so (gfx950): K_s(x, x') = K(x o sqrt(s), x' o sqrt(s)) with one s_k >= 0 per input feature, and
 * the derivative of the sparse evidence (nngp_sparse_evidence.h, DTC and VFE) with respect to every s_k, at O(N m^2).
 *
 * All quantities of nngp_sparse_evidence.h are taken on the scaled rows X o sqrt(s), U o sqrt(s); the inducing rows are held
 * fixed as RAW rows, so U_s moves with s.  For feature k the derivative is  -1/2 quad_k + 1/2 trace_k,
 *
 *   quad_k  = 2 sum_ij beta_i gamma_j dK_fu,ij/ds_k - gamma^T (dK~_uu/ds_k) gamma + beta^T beta dsigma2/ds_k
 *   trace_k = 2 sum_ij (K_fu M')_ij dK_fu,ij/ds_k + sum_ij E_ij dK~_uu,ij/ds_k + ts dsigma2/ds_k  [+ tr dK_ff/ds_k / sigma2 for vfe]
 *
 * with M', E and ts those of nngp_sparse_evidence.h for each bound.  The raw rows enter, so s_k = 0 has a finite derivative:
 *
 *   rectangular:  dK_ij/ds_k = (1/d) [ c_ij x_ik u_jk + e1_ij x_ik^2 + e2_ij u_jk^2 ],   c = dK/dK0, e1 = dK/dq_i, e2 = dK/dq_j;
 *                 every entry counts once, no exact-diagonal rule (as in the cross build)
 *   symmetric (K_uu): as nngp_ard.h, with its exact-diagonal rule
 *   tr dK_ff/ds_k = D0 v0 sum_i x_ik^2 / d,   tr dK_uu/ds_k = D0 v0 sum_{j<m} u_jk^2 / d   (D0 v0 = dK_ii/dq_i, closed form)
 *   dK~_uu = dK_uu + (jitter / m) tr(dK_uu) I,   dsigma2 = lambda tr(dK_ff/ds_k) / n  (0 with the absolute flag)
 *
 * No dK/ds matrix exists: the rectangular adjoint pass leaves the seeded adjoints at the input of Dense layer 0 behind, and one
 * contraction with the raw rows on the float64 MFMA turns them into d sums (csrc/sparse_ard.hip).  Everything is float64, no
 * atomics, no device-side waits: two evaluations give the same bits.  Hidden layers ReLU and ABRelu; no feature groups; ny = 1.
 * Conventions as in nngp_sparse.h: 0 on success, -2 for argument errors before any GPU work, device pointers unless marked host.
 */
#ifndef NNGP_SPARSE_ARD_H
#define NNGP_SPARSE_ARD_H

#include "nngp_sparse_evidence.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The only call that allocates for the relevances; needs nngp_sparse_reserve_evidence first (-2 otherwise).  Allocates the
 * relevances and their square roots, the raw inducing rows [m_cap, d], a scaled-row scratch for a chunk or a test block, a second
 * chunk_rows x mp_cap buffer for the rank-one half of the seeded adjoint, the per-tile row and column sums, the per-row-block
 * feature partials and the accumulators.  Repeatable (the second call does nothing).  A handle that never calls it allocates and
 * computes what it did without this header.  The one exception, as in nngp_sparse.h: a NNGP_COV_FULL predict under relevances
 * keeps its scaled test rows in a buffer allocated on first use and grown with the number of rows. */
int nngp_sparse_reserve_ard(nngp_sparse* h);
/* s: host, d values, each finite and >= 0 (-2 otherwise, or before nngp_sparse_reserve_ard); NULL: no relevances again.  Like
 * nngp_sparse_set_kernel it drops the inducing set and the accumulated rows.  From then on nngp_sparse_set_inducing, add_rows,
 * predict, evidence_grad and evidence_grad_ard take RAW rows and the handle scales them on the device: sqrt(s_k) is taken on
 * the host in double and each element is multiplied once, so s_k = 1 leaves the bits of x and x * sqrt(s) computed by the
 * caller gives the same rows.  Waits for the handle's work. */
int nngp_sparse_set_relevance(nngp_sparse* h, const double* s);
/* nngp_sparse_evidence_grad plus the derivative with respect to every relevance.  x: [n, d] raw rows, y: [n]: the rows that were
 * added, handed again.  nlml: host, the bits of nngp_sparse_evidence; grad: host, 2 n_dense + 1 values with the bits of
 * nngp_sparse_evidence_grad at the same relevances, or NULL; grad_s: host, d values.  -2 under the conditions of
 * nngp_sparse_evidence_grad and before nngp_sparse_set_relevance.  Synchronises. */
int nngp_sparse_evidence_grad_ard(nngp_sparse* h, const double* x, const double* y, int64_t n, int32_t bound, double* nlml,
                                  double* grad, double* grad_s, void* stream);
/* out: host, count >= 4 d.  Of the last nngp_sparse_evidence_grad_ard: quad_k, trace_k interleaved (2 d), then tr dK_ff/ds_k (d),
 * then tr dK_uu/ds_k (d). */
int nngp_sparse_ard_terms(const nngp_sparse* h, double* out, int32_t count);
/* The rectangular pass with its contraction alone (tests and integration): for the c x m block K = K(x o sqrt(s), u o sqrt(s)) of
 * the network `arch`,
 *   out[k] = sum_ij beta_i gamma_j dK_ij/ds_k,   out[d + k] = sum_ij seed[i * ld + j] dK_ij/ds_k,   k < d.
 * x: [c, d], u: [m, d] raw rows; s: host, d values; seed: [c, ld >= m] (columns m .. ld - 1 are never read; not written);
 * beta: [c], gamma: [m]; out: host, 2 d values.  Allocates and frees its buffers on the stream; synchronises. */
int nngp_sparse_ard_rect(const double* x, int64_t c, const double* u, int64_t m, int32_t d, const nngp_arch_act* arch,
                         const double* s, const double* seed, int64_t ld, const double* beta, const double* gamma, double* out,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_SPARSE_ARD_H */
