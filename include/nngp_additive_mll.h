/* nngp_additive_mll.h -- C ABI of the marginal likelihood of the additive NNGP kernel over feature groups in libnngp_hip.so
 * (gfx950): the evidence of the kernel of nngp_additive.h and its derivative with respect to every Dense layer's sigma_w^2 and
 * sigma_b^2, the regulariser and EVERY TERM WEIGHT.  On the handle of nngp_mll.h; GPU library only.
 *
 * With K = sum_t w_t K^(t) (t = 0: the whole input, t = 1 .. G: group t - 1, each term with its own 1 / d_t normalisation),
 * T = 1 + G, A = K + r I and NLML, alpha, r, lambda as in nngp_mll.h:
 *   dA/dw_t     = K^(t) + lambda (tr K^(t) / N) I            (relative; no I term when absolute)
 *   dK/dtheta_p = sum_t w_t dK^(t)/dtheta_p                  (the shared layer parameters), tr dK/dtheta_p likewise
 *   dNLML/dw_t  = -1/2 <alpha alpha^T, dA/dw_t> + 1/2 <A^-1, dA/dw_t>
 * A weight's derivative contracts the two seeds with the term's VALUE; the layer parameters take the reverse sweep of nngp_mll.h
 * once per term from seeds scaled by w_t.  Nothing of size N^2 exists per term.
 * Rules, so that the pass differentiates exactly the matrix nngp_kernel_build_additive produces: the whole-input term takes the
 * diagonal form (theta = 0) at i == j only; a group term takes it wherever the two slices give k == q == q' bit for bit (identical
 * slices), and its derivative there goes through the k chain alone; the q = 0 rule of nngp_mll.h holds per term.  A term with
 * weight 0 adds nothing to K, to dK/dtheta or to the traces, and still gets its own d/dw_t (forward recursion only): the answer
 * to "would adding this group help?".
 * Identity: sum_t w_t dNLML/dw_t = v_last dNLML/dv_last + c_last dNLML/dc_last -- a common factor on all weights is the last Dense
 * layer's sigma_w^2 and sigma_b^2.
 */
#ifndef NNGP_ADDITIVE_MLL_H
#define NNGP_ADDITIVE_MLL_H

#include "nngp_additive.h"
#include "nngp_mll.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fixes the table's ranges on the handle (weights in `groups` are ignored) and allocates, once, what the terms need: the table,
 * the weights and (1 + n_groups) (2 + NNGP_MAX_DENSE) reduced sums on the device, their host copies.  The per-tile partials of
 * the term halves go over the L^-T storage of the handle, which is dead once A^-1 and alpha exist.  A second call replaces the
 * table.  A bad table (the range checks of nngp_additive.h) returns -2, and so does a handle that has nngp_mll_reserve_ard
 * (nngp_mll_reserve_ard on a handle that has this call does too): relevances together with groups are not covered. */
int nngp_mll_reserve_additive(nngp_mll* h, const nngp_groups* groups);
/* As nngp_mll_evaluate, for the additive kernel.  weights: host, 1 + n_groups values (w0, then w_g in the table's order), finite,
 * >= 0, not all zero.  grad: host, 2 n_dense + 1 values as nngp_mll_evaluate, or NULL.  grad_w: host, 1 + n_groups values, or
 * NULL.  No device allocation; repeated evaluations are bit-identical (no atomics).  With n_groups = 0 and weights = {1.0},
 * nlml and grad have the bits of nngp_mll_evaluate.  Before nngp_mll_reserve_additive, with a negative or non-finite weight,
 * all weights zero or an Erf layer: -2.  nngp_mll_terms reports the layer and lambda halves as for nngp_mll_evaluate. */
int nngp_mll_evaluate_additive(nngp_mll* h, const nngp_arch_act* arch, const double* weights, double diag_reg,
                               int32_t diag_reg_absolute_scale, double* nlml, double* grad, double* grad_w, void* stream);
/* Of the last evaluation with grad_w: out[2t], out[2t+1] = the two halves of weight t (alpha^T dA/dw_t alpha and
 * tr(A^-1 dA/dw_t); grad_w[t] = -1/2 out[2t] + 1/2 out[2t+1]); then out[2T + t] = tr K^(t).  T = 1 + n_groups; count: room in
 * out (at least 3 T). */
int nngp_mll_additive_terms(const nngp_mll* h, double* out, int32_t count);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_ADDITIVE_MLL_H */
