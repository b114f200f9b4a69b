/* nngp_sparse_evidence.h -- the evidence of the sparse (inducing-point) NNGP and its gradient, on the nngp_sparse handle of
 * nngp_sparse.h in libnngp_hip.so (gfx950): what tunes W_std / b_std / diag_reg at the N the sparse model is for.
 *
 * With the quantities of nngp_sparse.h (L_u, G, R, sigma2, B = L_B L_B^T, C = L_B^-1 R), ny = 1, all sums over the true m:
 *
 *   NLML_dtc = 1/2 (y^T y - |C|^2) / sigma2 + 1/2 [(n - m) log sigma2 + 2 sum_i log (L_B)_ii] + (n / 2) log 2 pi
 *   NLML_vfe = NLML_dtc + (tr K_ff - tr G) / (2 sigma2)                       (Titsias' collapsed bound: an upper bound of the exact NLML)
 *
 * With U = X and jitter 0 both are the exact NLML of nngp_mll.h.  The gradient is taken with respect to v_l = W_std_l^2,
 * c_l = b_std_l^2 of every Dense layer and lambda = diag_reg, with the inducing rows held fixed and the jitter's dependence on
 * tr K_uu included.  With gamma = L_u^-T L_B^-T C, beta = (y - K_fu gamma) / sigma2, M = L_u^-T B^-1 L_u^-1 and
 * P = K~_uu^-1 - sigma2 M it is  -1/2 quad_p + 1/2 trace_p,
 *
 *   quad_p  = 2 sum_ij beta_i gamma_j dK_fu,ij - gamma^T dK~_uu gamma + beta^T beta dsigma2
 *   trace_p = 2 sum_ij (K_fu M')_ij dK_fu,ij + sum_ij E_ij dK~_uu,ij + ts dsigma2 [+ tr dK_ff / sigma2 for vfe]
 *   dtc:  M' = M,                       E = -P,                                       ts = (n - m + sigma2 tr B^-1) / sigma2
 *   vfe:  M' = M - K~_uu^-1 / sigma2,   E = -P + L_u^-T G L_u^-1 / sigma2,            ts -= (tr K_ff - tr G) / sigma2^2
 *   dK~_uu = dK_uu + jitter / m tr(dK_uu) I,   dsigma2 = lambda tr(dK_ff) / n  (0 with the absolute flag; d/dlambda: tr K_ff / n, or 1)
 *
 * No dK / dtheta matrix exists: two adjoint passes of the layer recursion contract it entry by entry -- the symmetric one of
 * nngp_mll.h over K_uu, and a rectangular one over each chunk's K(X_c, U) (csrc/sparse_evidence.hip).  Hidden layers ReLU and
 * ABRelu (LeakyRelu, Abs); no feature groups.  Everything is float64; no atomics: two evaluations give the same bits.
 * Conventions as in nngp_sparse.h: 0 on success, -2 for argument errors before any GPU work, device pointers unless marked host.
 */
#ifndef NNGP_SPARSE_EVIDENCE_H
#define NNGP_SPARSE_EVIDENCE_H

#include "nngp_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNGP_BOUND_DTC 0
#define NNGP_BOUND_VFE 1

/* The only call that allocates for the evidence: three mp_cap^2 matrices, a chunk_rows x mp_cap seed buffer, gamma, beta and the
 * per-tile partials.  The evidence calls after it add nothing to nngp_alloc_count(); a handle that never calls it allocates what
 * nngp_sparse_create allocates.  Repeatable (the second call does nothing). */
int nngp_sparse_reserve_evidence(nngp_sparse* h);
/* New hyperparameters on the same handle, without reallocation: arch must have the handle's number of Dense layers and pass the
 * checks of nngp_mll_evaluate (finite non-negative w_std / b_std, no Erf layer).  Drops the inducing set and the accumulated
 * rows: set_inducing, add_rows and finish follow. */
int nngp_sparse_set_kernel(nngp_sparse* h, const nngp_arch_act* arch, double diag_reg, int32_t diag_reg_absolute_scale);
/* nlml: host.  Valid after nngp_sparse_finish, with ny = 1; no pass over the data.  Synchronises the stream. */
int nngp_sparse_evidence(nngp_sparse* h, int32_t bound, double* nlml, void* stream);
/* x: [n, d], y: [n] -- the rows that were added, handed again, walked in the same chunks.  nlml: host, the bits of
 * nngp_sparse_evidence.  grad: host, 2 n_dense + 1 values: d/dv_l, d/dc_l per Dense layer, then d/dlambda.  -2 when n differs from
 * the rows added, ny != 1, the handle has feature groups or an Erf layer, or the evidence was not reserved.  Synchronises. */
int nngp_sparse_evidence_grad(nngp_sparse* h, const double* x, const double* y, int64_t n, int32_t bound, double* nlml, double* grad,
                              void* stream);
/* out: host, count >= 2 (2 n_dense + 1) + 7.  Of the last gradient: quad_p, trace_p interleaved for the 2 n_dense + 1 components,
 * then sum_i log (L_B)_ii, y^T y - |C|^2, tr K_ff, tr G, sigma2, tr B^-1, beta^T beta. */
int nngp_sparse_evidence_terms(const nngp_sparse* h, double* out, int32_t count);
/* The rectangular adjoint pass alone (tests and integration): for the c x m block K(x, u) of the network `arch`,
 *   out[p] = sum_ij beta_i gamma_j dK_ij / dtheta_p,   out[2 n_dense + p] = sum_ij seed[i * ld + j] dK_ij / dtheta_p,   p < 2 n_dense.
 * x: [c, d], u: [m, d], seed: [c, ld >= m] (columns m .. ld - 1 are never read), beta: [c], gamma: [m]; out: host, 4 n_dense values.
 * Allocates and frees its partials on the stream; synchronises. */
int nngp_sparse_adjoint_rect(const double* x, int64_t c, const double* u, int64_t m, int32_t d, const nngp_arch_act* arch,
                             const double* seed, int64_t ld, const double* beta, const double* gamma, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_SPARSE_EVIDENCE_H */
