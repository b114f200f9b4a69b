/* nngp_additive.h -- C ABI of the additive NNGP / NTK kernels over feature groups in libnngp_hip.so (gfx950).
 *
 * The prior is a sum of independent networks of one architecture, one on the whole input and one per group of features:
 *   f(x) = sqrt(w0) f0(x) + sum_g sqrt(w_g) f_g(x_g),   x_g = x[begin_g:end_g]
 * so that, in both the NNGP and the NTK form,
 *   K(x, x') = w0 K_arch(x, x') + sum_g w_g K_arch(x_g, x'_g).
 * Every term is the closed form of nngp_activations.h with its own input normalisation: the Gram entry x_g . x'_g / d_g and the
 * two diagonal entries |x_g|^2 / d_g, |x'_g|^2 / d_g are taken over the d_g = end_g - begin_g features of the group.
 *
 * Same conventions as nngp_hip.h, with one difference: the two stand-alone calls copy the group table to the device and free it,
 * so they wait for their work on `stream` before they return (the _act calls only enqueue).  A caller that builds the same
 * kernel many times should hold a model.  GPU library only (no host build), like nngp_activations.h.
 */
#ifndef NNGP_ADDITIVE_H
#define NNGP_ADDITIVE_H

#include "nngp_activations.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNGP_MAX_GROUPS 1024

typedef struct nngp_groups {
    int32_t n_groups;     /* 0 .. NNGP_MAX_GROUPS */
    int32_t reserved;
    const int32_t* begin; /* host arrays [n_groups]: 0 <= begin < end <= d; groups may overlap, may leave features uncovered */
    const int32_t* end;
    const double* weight; /* [n_groups], finite, >= 0 */
    double full_weight;   /* w0 >= 0: weight of the whole-input term; 0 leaves it out */
} nngp_groups;

/* As nngp_kernel_build_act, nngp_kernel_diag_act and nngp_model_create_act, for the summed kernel.  A bad range, a negative or
 * non-finite weight, all weights zero (w0 included) or n_groups above NNGP_MAX_GROUPS return -2.  The library copies the group
 * table: the caller's arrays need not outlive the call.  With n_groups = 0 and full_weight = 1 the three calls compute the bits
 * of their _act counterparts.  A model created here runs fit, append, predict (every covariance mode and refine level),
 * prepare_serving, pool selection, build_rows, matvec_rows and kernel_buffer on the summed kernel. */
int nngp_kernel_build_additive(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d,
                               const nngp_arch_act* arch, const nngp_groups* groups, int32_t out_dtype, void* out_nngp,
                               void* out_ntk, int64_t ld, int64_t row_begin, int64_t row_end, void* stream);
int nngp_kernel_diag_additive(const double* x, int64_t n, int32_t d, const nngp_arch_act* arch, const nngp_groups* groups,
                              double* diag_nngp, double* diag_ntk, void* stream);
int nngp_model_create_additive(nngp_model** out, int64_t n_cap, int64_t m_cap, int32_t d, int32_t ny,
                               const nngp_arch_act* arch, const nngp_groups* groups, int32_t get, double diag_reg,
                               int32_t diag_reg_absolute_scale);

#ifdef __cplusplus
}
#endif

#endif /* NNGP_ADDITIVE_H */
