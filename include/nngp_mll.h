/* nngp_mll.h -- C ABI of the NNGP marginal likelihood and its gradient in libnngp_hip.so (gfx950): the evidence of the
 * NNGP posterior (get = 'nngp') of stax.serial(Dense, (act, Dense)*) with act ReLU or ABRelu (LeakyRelu, Abs), and its
 * derivative with respect to every Dense layer's sigma_w^2, sigma_b^2 and the regulariser.
 *
 * Same conventions as nngp_hip.h.  Kept apart from nngp_hip.h because these entry points have no host build: they run on the
 * GPU only.  All-ReLU networks come in as an nngp_arch_act with NNGP_ACT_RELU codes.
 *
 * With v_l = w_std[l]^2, c_l = b_std[l]^2 (l = 0 .. n_dense-1) and lambda = diag_reg:
 *   A = K + r I,   r = lambda tr(K) / N  (relative, the default)   or   r = lambda  (diag_reg_absolute_scale)
 *   NLML = 1/2 y^T A^-1 y + 1/2 log det A + (N/2) log(2 pi)        (y uncentred: the zero-mean prior of the posterior)
 *   dNLML/dtheta = -1/2 alpha^T (dA/dtheta) alpha + 1/2 tr(A^-1 dA/dtheta),   alpha = A^-1 y
 *   dA/dtheta_p = dK/dtheta_p + lambda (tr dK/dtheta_p / N) I  (relative; no I term when absolute),
 *   dA/dlambda = (tr K / N) I  (relative)  or  I  (absolute)
 * dK/dtheta is never formed: one pass contracts it with W = alpha alpha^T - A^-1 entry by entry, by the adjoint of the layer
 * recursion (Dense: k <- v k + c; ReLU: s = sqrt(max(q1 q2 - k^2, 0)), theta = atan2(s, k), kdot = (pi - theta) / 2 pi,
 * k <- kdot k + s / 2 pi, q <- q / 2; ABRelu(a, b): k <- a b k + (b - a)^2 relu(k), q <- (a^2 + b^2) / 2 q):
 *   dK'/dk = kdot,  dK'/dq1 = s / (4 pi q1)  (ReLU; ABRelu: a b + (b - a)^2 kdot and (b - a)^2 s / (4 pi q1))
 * Rules: a ReLU input with q1 = 0 contributes 0 to the adjoint of q1 (exact for every sigma_w^2 component and for every
 * sigma_b^2 component from the first positive bias on; where a zero row meets sigma_b^2 = 0 in the layers before the first
 * positive bias, the true one-sided derivative of those sigma_b^2 is unbounded and the value reported is the rule's).
 * Diagonal entries take theta = 0 exactly (s = 0, kdot = 1/2), as the kernel build does.
 */
#ifndef NNGP_MLL_H
#define NNGP_MLL_H

#include "nngp_activations.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Everything is float64 and has its own factorisation (the float64 Cholesky behind nngp_potrf_f64); the NNGP model is not
 * involved.  The handle holds A / L, L^-T and A^-1 (3 Np^2 doubles, Np = n_cap rounded up to 128), the row norms, y,
 * alpha, w = L^-1 y and the gradient partials.  No device allocation after create.  One handle is driven from one stream
 * at a time.  The same handle serves the leave-one-out objectives of nngp_loo.h. */
typedef struct nngp_mll nngp_mll;
int nngp_mll_create(nngp_mll** out, int64_t n_cap, int32_t d);
int nngp_mll_destroy(nngp_mll* h);
/* x: [n, d], y: [n, ny]; ny != 1 returns -2. */
int nngp_mll_set_train(nngp_mll* h, const double* x, const double* y, int64_t n, int32_t ny, void* stream);
/* Builds A for arch / diag_reg, factors it in float64, keeps the factor.  nlml: host.  grad: host, 2*n_dense + 1 values
 * (d/dsigma_w,l^2, d/dsigma_b,l^2 for l = 0 .. n_dense-1, then d/dlambda) or NULL for the NLML alone.  Synchronises the
 * stream.  A pivot that is not positive returns rc < 0 naming its column; an Erf layer or a non-finite / negative
 * parameter returns -2.  (Only the NNGP posterior has this evidence: the NTK ensemble is not a GP with prior Theta.) */
int nngp_mll_evaluate(nngp_mll* h, const nngp_arch_act* arch, double diag_reg, int32_t diag_reg_absolute_scale,
                      double* nlml, double* grad, void* stream);
/* The cancelling halves of each gradient component of the last evaluation with a gradient (host): for p = 0 .. 2*n_dense,
 * out[2p] = alpha^T dA_p alpha, out[2p+1] = tr(A^-1 dA_p) (grad[p] = -1/2 out[2p] + 1/2 out[2p+1]); then sum log L_ii,
 * y^T A^-1 y, tr K, alpha^T alpha, tr A^-1, and tr dK_p for p = 0 .. 2*n_dense-1.  count: room in out (at least
 * 2 (2 n_dense + 1) + 5 + 2 n_dense). */
int nngp_mll_terms(const nngp_mll* h, double* out, int32_t count);
/* Device factor of the last evaluation: L in the lower triangle of [n_padded, ld] (identity on the padding; the part above
 * the diagonal blocks is workspace, read the lower triangle only).  An error after a leave-one-out evaluation with a
 * gradient (nngp_loo.h), which reuses the factor's storage. */
int nngp_mll_factor_buffer(const nngp_mll* h, double** l, int64_t* ld, int64_t* n_padded);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_MLL_H */
