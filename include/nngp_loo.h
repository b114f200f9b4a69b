/* nngp_loo.h -- C ABI of leave-one-out cross-validation in libnngp_hip.so (gfx950): the leave-one-out (LOO) predictions of
 * the NNGP posterior (or of kernel ridge regression with the NTK) at every training point, the two objectives built on them
 * and their gradient with respect to every Dense layer's sigma_w^2, sigma_b^2 and the regulariser.
 *
 * GPU only, like nngp_mll.h, and on the SAME handle (nngp_mll_create / nngp_mll_set_train): one handle serves the marginal
 * likelihood and the LOO objectives of a tuning run.  No device allocation after nngp_mll_create; no atomics, every sum in a
 * fixed order: repeated evaluations are bit-identical.
 *
 * With A = K + r I (get = NNGP_GET_NNGP) or A = Theta + r I (NNGP_GET_NTK), r = lambda tr / N (relative) or lambda (absolute),
 * B = A^-1, alpha = B y, b_i = B_ii  (Rasmussen & Williams, section 5.4.2):
 *   residual  r_i = alpha_i / b_i,   mean  mu_i = y_i - r_i,   variance  s_i = 1 / b_i  (of y_i, the regulariser as noise)
 *   mse  = 1/N sum r_i^2,            nlpd = 1/N sum [ 1/2 log(2 pi s_i) + r_i^2 / (2 s_i) ]
 * Convention: r keeps its FULL-DATA value when a point is left out (tr K is not recomputed without row i); with it the closed
 * form equals the refit without point i exactly.  y is one column, uncentred, as in the marginal likelihood.
 *
 * Gradient (NNGP only): with abar_i = dL/dalpha_i, bbar_i = dL/db_i
 *   mse:  abar_i = 2 r_i / (N b_i),   bbar_i = -2 r_i^2 / (N b_i)
 *   nlpd: abar_i = alpha_i / (N b_i), bbar_i = -(1 / b_i + alpha_i^2 / b_i^2) / (2 N)
 * u = B abar, C = B diag(bbar) B, and dL/dtheta_p = sum_ij W_ij dA_ij/dtheta_p with W = -1/2 (alpha u^T + u alpha^T) - C.
 * dA/dtheta_p and dA/dlambda are those of nngp_mll.h (the relative regulariser's trace terms multiply tr W); dK/dtheta is never
 * formed: the fused adjoint pass of the marginal likelihood runs from the seeds 1/2 (alpha_i u_j + u_i alpha_j) and C_ij, with
 * the same q = 0 and exact-diagonal rules.
 */
#ifndef NNGP_LOO_H
#define NNGP_LOO_H

#include "nngp_mll.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNGP_LOO_NLPD 0
#define NNGP_LOO_MSE 1

/* Builds A for arch / get / diag_reg, factors it in float64 and evaluates the objective (NNGP_LOO_*).  value: host.  grad:
 * host, 2*n_dense + 1 values in the layout of nngp_mll_evaluate, or NULL for the value alone (which then costs no A^-1
 * product: alpha and b come from the rows of L^-T).  The value is the same number, bit for bit, with and without the gradient.
 * Synchronises the stream.  Returns -2 (nngp_last_error says why) for an Erf layer, a non-finite or negative parameter, an
 * unknown get / objective, get = NNGP_GET_NTK with a gradient (the NTK mean is kernel ridge regression, its ensemble posterior
 * is not a GP with prior Theta) and get = NNGP_GET_NTK with NNGP_LOO_NLPD (no predictive variance); a pivot that is not
 * positive returns rc < 0 naming its column and leaves the handle usable.
 * An evaluation WITH a gradient writes C over the factor: nngp_mll_factor_buffer then returns an error until the next
 * evaluation that keeps its factor (nngp_mll_evaluate, or this one without a gradient). */
int nngp_mll_loo_evaluate(nngp_mll* h, const nngp_arch_act* arch, int32_t get, double diag_reg, int32_t diag_reg_absolute_scale,
                          int32_t objective, double* value, double* grad, void* stream);
/* LOO means and variances of the last nngp_mll_loo_evaluate: device outputs of n values each.  var may be NULL, and must be
 * NULL after an NTK evaluation (-2 otherwise). */
int nngp_mll_loo_predictions(const nngp_mll* h, double* mean, double* var, void* stream);
/* The cancelling halves of each gradient component of the last LOO evaluation with a gradient (host): for p = 0 .. 2*n_dense,
 * out[2p] = sum_ij 1/2 (alpha_i u_j + u_i alpha_j) dA_ij/dtheta_p, out[2p+1] = sum_ij C_ij dA_ij/dtheta_p
 * (grad[p] = -(out[2p] + out[2p+1])); then alpha^T u, tr C, tr K, and tr dK_p for p = 0 .. 2*n_dense-1.  count: room in out
 * (at least 2 (2 n_dense + 1) + 3 + 2 n_dense). */
int nngp_mll_loo_terms(const nngp_mll* h, double* out, int32_t count);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_LOO_H */
