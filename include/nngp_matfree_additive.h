/* nngp_matfree_additive.h -- C ABI of the matrix-free exact NNGP posterior on the additive kernel over feature groups
 * (nngp_additive.h) in libnngp_hip.so (gfx950).
 *
 *   K(x, x') = w0 K_arch(x, x') + sum_g w_g K_arch(x_g, x'_g),   x_g = x[begin_g:end_g]
 *
 * The model of nngp_matfree.h with this kernel in all four places where the kernel enters: the fused operator runs its additive
 * tile body (per 64 x 64 tile the group terms are summed in the table's order and the whole-input term is added last -- the
 * value and the order of operations of nngp_kernel_build_additive), the preconditioner is the sparse model of the summed kernel
 * (nngp_sparse_create with the table), the m = 0 noise and the predictive K(x, x) come from the grouped diagonal, and the cross
 * block of predict from the additive build.  The predictive variance is taken in its second-order form
 *     var = K(x, x) - (B . Z + Z . (B - A Z))
 * with the true residual the solver has formed anyway: B . Z alone keeps a term that is first order in Z's error, and on this
 * kernel (variances of 1e-4 .. 1e-3 of K(x, x), solves of two dozen iterations) that term is what limits the variance.
 * NNGP only.  The cost is one layer map per live group and entry on top of the plain operator's one, in every CG iteration.
 *
 * The handle is an nngp_matfree: fit, solve, predict, alpha, info and destroy of nngp_matfree.h work on it unchanged, and fit,
 * solve and predict still add nothing to nngp_alloc_count().  The handle owns its copy of the group table.
 * `groups` is required; its errors are the -2s of nngp_additive.h (a bad range, a negative or non-finite weight, all weights
 * zero, n_groups above NNGP_MAX_GROUPS).  With the plain table (n_groups = 0, full_weight = 1) both calls compute the bytes of
 * nngp_matfree_create / nngp_kmv_f64.  GPU library only (no host build).
 */
#ifndef NNGP_MATFREE_ADDITIVE_H
#define NNGP_MATFREE_ADDITIVE_H

#include "nngp_matfree.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nngp_matfree_create for the summed kernel: the same sizes, limits and footprint (plus the group table). */
int nngp_matfree_create_additive(nngp_matfree** out, int64_t n_cap, int64_t m_cap, int64_t chunk_rows, int64_t rhs_cap, int32_t d,
                                 int32_t ny, const nngp_arch_act* arch, const nngp_groups* groups, double diag_reg,
                                 int32_t diag_reg_absolute_scale, double jitter);

/* nngp_kmv_f64 for the summed kernel: out [r, ldo] = (K(x, x) + diag_add I) v.  The call copies the group table to the device
 * and frees it, so it waits for its work on `stream` before it returns (as the stand-alone calls of nngp_additive.h do). */
int nngp_kmv_additive_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int32_t r, const double* x, int64_t n, int32_t d,
                          const nngp_arch_act* arch, const nngp_groups* groups, double diag_add, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_MATFREE_ADDITIVE_H */
