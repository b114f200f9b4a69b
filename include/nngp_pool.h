/* nngp_pool.h -- C ABI of the batch-aware pool selection in libnngp_hip.so (gfx950).
 *
 * nngp_pool_select (nngp_hip.h) scores every pool query by its own posterior standard deviation.  The call below picks a batch
 * that accounts for the correlation between the queries: greedy selection by conditional variance, which is a partial pivoted
 * Cholesky factorisation of the pool's posterior covariance (plus the observation noise on the picked entries).
 *
 * Same conventions as nngp_hip.h: 0 on success, non-zero with text in nngp_last_error(); device pointers; asynchronous on
 * `stream`.  GPU library only (no host build), like nngp_activations.h.
 */
#ifndef NNGP_POOL_H
#define NNGP_POOL_H

#include "nngp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Greedy selection by conditional variance = partial pivoted Cholesky of cov + noise*I restricted to the picks.
 * cov: [m, m] f64 on the device, leading dimension ld >= m, symmetric PSD; only rows/cols < m are read.
 * noise >= 0 (the model's reg: an observed label is y + N(0, noise)).  1 <= count <= m (count 0: returns 0, touches nothing).
 * indices: [count] int64, in the order picked.  gains: [count] f64 or NULL: the conditional variance of pick j when it was picked.
 * factor: [count, ldf] f64 with ldf >= m, or NULL (the library then uses its own workspace): row j is the j-th column of the factor,
 *   c_j = (cov[:, p_j] - sum_{t<j} c_t[:] c_t[p_j]) / sqrt(d[p_j] + noise),  d <- d - c_j^2,  d starts as diag(cov).
 * Asynchronous on `stream`; no read-back.
 *
 * Pick rule: p_j is the index with the largest d among those not picked yet; equal d goes to the lowest index.  A NaN d never
 *   wins over one that is not NaN (a diagonal entry of -inf counts as NaN), so such indices go last, lowest index first.
 * Degenerate pivot: where d[p_j] + noise > 0 does not hold (<= 0, or NaN), c_j is zero and d stays as it is.
 * A picked index is marked in d itself (-inf) and never compared again: the exclusion does not depend on its residual, which
 *   rounding can leave negative and a NaN entry of cov can make NaN; the mark stays whatever the later columns hold.  An index
 *   that is not picked never carries the mark: a d that overflows to -inf counts as NaN.  So every index is picked at most once,
 *   whatever cov holds.  gains[j] is d[p_j] as it stood, without the noise.
 * cov is taken as symmetric: the column cov[:, p_j] is read as the row cov[p_j, :].  Columns >= m of a factor row (the padding
 *   up to ldf) are not written.  Two calls on the same input give the same bits, whatever the device does in between.
 * Errors (-2, before any GPU work): NULL cov or indices, m < 1, count < 0 or > m, ld < m, factor given with ldf < m, noise
 *   negative or not finite. */
int nngp_pool_select_greedy(const double* cov, int64_t m, int64_t ld, double noise, int64_t count,
                            int64_t* indices, double* gains, double* factor, int64_t ldf, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NNGP_POOL_H */
