/* nngp_ard.h -- C ABI of per-feature input relevances (automatic relevance determination, ARD) for the NNGP evidence and the
 * leave-one-out objectives in libnngp_hip.so (gfx950), on the handle of nngp_mll.h.  GPU only, like nngp_mll.h / nngp_loo.h.
 *
 * With relevances s in R^d, s_k >= 0:  K_s(x, x') = K(x o sqrt(s), x' o sqrt(s)), that is
 *   K0_ij = (1/d) sum_k s_k x_ik x_jk,   q_i = (1/d) sum_k s_k x_ik^2,
 * and everything after the input stage as in nngp_mll.h (recursion, exact diagonal, the q = 0 rule, r = lambda tr K / N).
 * For a loss whose gradient is sum_ij S_ij dA_ij/dtheta (S = the two seeds of nngp_mll.h or nngp_loo.h):
 *   dK_ij/ds_k = (1/d) [c_ij x_ik x_jk + e1_ij x_ik^2 + e2_ij x_jk^2],   c = dK/dK0, e1 = dK/dq_i, e2 = dK/dq_j,
 *   dK_ii/ds_k = D0 v0 x_ik^2 / d  (the diagonal depends on q_i alone),   tr dK/ds_k = D0 v0 sum_i x_ik^2 / d,
 *   dA/ds_k = dK/ds_k + lambda (tr dK/ds_k / N) I  (relative; no I term when absolute).
 * The raw x enters, so s_k = 0 has a finite gradient.  dK/ds_k is never formed: the adjoint pass leaves S o c (lower
 * triangle, over the dead L^-T) and the row sums of S o e, and one float64 MFMA contraction with X finishes all d features.
 * No atomics, every sum in a fixed order: repeated evaluations are bit-identical, and with every s_k = 1 the value and the
 * 2 n_dense + 1 gradient components have the bits of nngp_mll_evaluate / nngp_mll_loo_evaluate.
 */
#ifndef NNGP_ARD_H
#define NNGP_ARD_H

#include "nngp_mll.h"
#include "nngp_loo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Allocates, once, what the relevances need: a second n_cap x d copy of x (scaled), its row norms, the relevances, the
 * per-tile row sums (2 (n_cap / 64) Np doubles) and the d-length partial and result vectors.  No device allocation after it.
 * A handle that never gets this call allocates and computes exactly what it did before this header existed. */
int nngp_mll_reserve_ard(nngp_mll* h);
/* nngp_mll_evaluate at relevances s (host, d values).  grad (2 n_dense + 1, as nngp_mll_evaluate) and grad_s (host, d values:
 * dNLML/ds_k) may each be NULL.  A negative or non-finite s_k, a call before nngp_mll_reserve_ard, an Erf layer: -2. */
int nngp_mll_evaluate_ard(nngp_mll* h, const nngp_arch_act* arch, const double* s, double diag_reg,
                          int32_t diag_reg_absolute_scale, double* nlml, double* grad, double* grad_s, void* stream);
/* nngp_mll_loo_evaluate at relevances s, with its restrictions; the NTK gets the value only (grad_s must be NULL). */
int nngp_mll_loo_evaluate_ard(nngp_mll* h, const nngp_arch_act* arch, int32_t get, const double* s, double diag_reg,
                              int32_t diag_reg_absolute_scale, int32_t objective, double* value, double* grad, double* grad_s,
                              void* stream);
/* Of the last evaluation with grad_s (host): out[2k], out[2k+1] = the two cancelling halves of feature k, as nngp_mll_terms
 * (grad_s[k] = -1/2 out[2k] + 1/2 out[2k+1]) or nngp_mll_loo_terms (grad_s[k] = -(out[2k] + out[2k+1])) report them; then
 * out[2d + k] = tr dK/ds_k.  count: room in out (at least 3 d). */
int nngp_mll_ard_terms(const nngp_mll* h, double* out, int32_t count);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_ARD_H */
