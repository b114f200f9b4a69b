/* nngp_activations.h -- C ABI of the closed-form NNGP / NTK kernels of networks with other activations than ReLU in
 * libnngp_hip.so (gfx950): stax.serial(Dense, (act, Dense)*) with act one of Relu, ABRelu (LeakyRelu, Abs) and Erf, chosen
 * per hidden layer.
 *
 * Same conventions as nngp_hip.h.  Kept apart from nngp_hip.h because these entry points have no host build: they run on the
 * GPU only, and a host build that read an nngp_arch_act as an nngp_arch would compute ReLU kernels for it.
 *
 * Per hidden layer, after its Dense layer (k: the cross entry, q1, q2: the two diagonal entries; NTK: Theta <- kdot Theta,
 * then the next Dense layer adds K):
 *   ABRelu(a, b), phi(x) = a x (x < 0), b x (x >= 0):  s = sqrt(max(q1 q2 - k^2, 0)), theta = atan2(s, k),
 *     K' = a b k + (b - a)^2 (s + (pi - theta) k) / (2 pi),  kdot = a b + (b - a)^2 (pi - theta) / (2 pi),  q' = (a^2 + b^2) / 2 q
 *     (LeakyRelu(alpha) = ABRelu(alpha, 1), Abs = ABRelu(-1, 1); ABRelu(0, 1) is ReLU and computed by the ReLU kernels)
 *   Erf(a, b, c), phi(x) = a erf(b x) + c:  u = 2 b^2 k,  r = 1 + 2 b^2 (q1 + q2) + 4 b^4 (q1 q2 - k^2),  w = sqrt(r),
 *     K' = a^2 (2 / pi) asin(u / sqrt(u^2 + r)) + c^2,  kdot = a^2 (4 / pi) b^2 / w,
 *     q' = a^2 (2 / pi) asin(2 b^2 q / (1 + 2 b^2 q)) + c^2
 */
#ifndef NNGP_ACTIVATIONS_H
#define NNGP_ACTIVATIONS_H

#include "nngp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNGP_ACT_RELU 0   /* p unused                     */
#define NNGP_ACT_ABRELU 1 /* p = {a, b, unused}           */
#define NNGP_ACT_ERF 2    /* p = {a, b, c}                */

/* The architecture of nngp_hip.h plus one activation per hidden layer: act[l] / p[l] follow Dense layer l,
 * l = 0 .. base.n_dense - 2.  An all-ReLU nngp_arch_act computes exactly what nngp_arch does. */
typedef struct nngp_arch_act {
    nngp_arch base;
    int32_t act[NNGP_MAX_DENSE - 1];
    double p[NNGP_MAX_DENSE - 1][3];
} nngp_arch_act;

/* As nngp_kernel_build, nngp_kernel_diag and nngp_model_create, for an nngp_arch_act.  An unknown activation code or a
 * non-finite parameter returns -2.  A model created here runs fit, append, predict, serving and pool selection unchanged. */
int nngp_kernel_build_act(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d,
                          const nngp_arch_act* arch, int32_t out_dtype, void* out_nngp, void* out_ntk,
                          int64_t ld, int64_t row_begin, int64_t row_end, void* stream);
int nngp_kernel_diag_act(const double* x, int64_t n, int32_t d, const nngp_arch_act* arch,
                         double* diag_nngp, double* diag_ntk, void* stream);
int nngp_model_create_act(nngp_model** out, int64_t n_cap, int64_t m_cap, int32_t d, int32_t ny,
                          const nngp_arch_act* arch, int32_t get, double diag_reg,
                          int32_t diag_reg_absolute_scale);

#ifdef __cplusplus
}
#endif

#endif /* NNGP_ACTIVATIONS_H */
