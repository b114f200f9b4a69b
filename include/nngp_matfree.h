/* nngp_matfree.h -- C ABI of the matrix-free exact NNGP posterior in libnngp_hip.so (gfx950).
 *
 * The exact models hold the N x N kernel and pay N^3 / 3; the sparse model (nngp_sparse.h) leaves the exact posterior.  This
 * model gives the EXACT posterior -- mean and variances -- without ever storing K: a preconditioned conjugate-gradient solver
 * applies A = K(X, X) + sigma2 I through a fused kernel that builds K tile by tile and multiplies it into a block of vectors
 * (nngp_kmv_f64), and the sparse model of m inducing rows is the preconditioner.  Everything is float64.
 *
 *   sigma2 = diag_reg * (sum_i K(x_i, x_i)) / n                       (diag_reg itself with the absolute flag)
 *   sparse fit (nngp_sparse.h):  L_u,  Vt = K(X, U) L_u^-T  [n, mp]  (kept),  L_B = chol(sigma2 I + Vt^T Vt)
 *   P = sigma2 I + Vt Vt^T,    P^-1 r = (r - Vt L_B^-T L_B^-1 Vt^T r) / sigma2      (Woodbury; m = 0: P = I)
 *   alpha = A^-1 Y by PCG on all ny columns at once
 *   predict, per block of at most rhs_cap test rows:  B = K(X, X_b),  mean = B^T alpha,  Z = A^-1 B by PCG,
 *       var = K(x, x) - sum_i B_i Z_i       (the covariance of the latent function, as in the other models)
 *
 * The solver: per-column scalars from fixed-order reductions; a column that has converged (|r| <= tol |b|), or whose p^T A p is
 * not positive and finite, is frozen; a column's result does not depend on which other columns share its block.  After the loop
 * one more pass forms the true residual B - A X; a column above tol restarts once from it; the reported residual is the recomputed
 * one.  Return codes of fit / solve / predict: 0 = every column's true relative residual <= tol; 1 = not reached within max_iter
 * (the results are written, nngp_matfree_info says so); < 0 errors; -2 argument errors before any GPU work.
 *
 * Vectors are RHS-major: [r, ld], each vector contiguous.  Same conventions as nngp_sparse.h: device pointers, work enqueued on
 * `stream`, one handle driven from one stream at a time; fit, solve and predict wait for the stream (the stop rule reads the
 * residual norms back every iteration).  Only the NNGP kernel of the whole input: get = NNGP_GET_NTK, NNGP_COV_FULL and a
 * group table other than the plain one return -2.  GPU library only (no host build), like nngp_sparse.h.
 */
#ifndef NNGP_MATFREE_H
#define NNGP_MATFREE_H

#include "nngp_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nngp_matfree nngp_matfree;

typedef struct nngp_matfree_info_t {
    int64_t n;             /* training rows of the last fit */
    int64_t m;             /* inducing rows of the preconditioner (0: none) */
    double sigma2;         /* the noise of the last fit */
    int32_t iterations;    /* CG iterations of the last fit / solve / predict (predict: the most of any block) */
    int32_t k_passes;      /* applications of the fused operator in that call */
    double rel_residual;   /* worst true relative residual |b - A x| / |b| over the columns of that call */
    int32_t converged;     /* 1: rel_residual <= tol */
    int32_t restarts;      /* restarts from the true residual in that call */
} nngp_matfree_info_t;

/* All device memory is allocated here; fit, solve and predict add nothing to nngp_alloc_count().  With np = n_cap rounded up to
 * 128, mp = m_cap rounded up to 128 and rp = rhs_cap rounded up to 128 the footprint in doubles is
 *     n_cap (d + 1)  +  2 np mp  +  7 rp np  +  mp^2 + 2 rp mp + 128 max(rp, mp)  +  partials  +  the sparse handle
 * (the inputs and their norms; Vt and its transposed copy; the solver's R, Z, P, Q, the cross block B, its solution and the
 * right-hand sides of alpha; L_B^-T, two [rp, mp] blocks and the solve scratch; the operator's split partials, at most
 * 64 (n_cap + 131072) doubles; nngp_sparse.h for the handle, with test_cap = 128).  Nothing is N x N.
 * n_cap >= 1; m_cap 0 .. 16384 (0: never a preconditioner); chunk_rows a positive multiple of 128; 1 <= rhs_cap <= 4096;
 * 1 <= ny <= 16; diag_reg and jitter finite and >= 0; get must be NNGP_GET_NNGP; groups NULL or the plain table. */
int nngp_matfree_create(nngp_matfree** out, int64_t n_cap, int64_t m_cap, int64_t chunk_rows, int64_t rhs_cap, int32_t d, int32_t ny,
                        const nngp_arch_act* arch, const nngp_groups* groups, int32_t get, double diag_reg,
                        int32_t diag_reg_absolute_scale, double jitter);
int nngp_matfree_destroy(nngp_matfree* h);
/* x: [n, d], y: [n, ny], 1 <= n <= n_cap; u: [m, d], 0 <= m <= m_cap (u = NULL, m = 0: no preconditioner).  tol finite in (0, 1),
 * max_iter >= 1.  A pivot error of the sparse handle is passed through (rc < 0); the handle then accepts another fit. */
int nngp_matfree_fit(nngp_matfree* h, const double* x, const double* y, int64_t n, const double* u, int64_t m, double tol,
                     int32_t max_iter, void* stream);
/* out [r, ldo] = (K + sigma2 I)^-1 b for the caller's b [r, ldb], RHS-major, 1 <= r <= rhs_cap, ldb, ldo >= n. */
int nngp_matfree_solve(nngp_matfree* h, const double* b, int64_t ldb, int32_t r, double* out, int64_t ldo, double tol, int32_t max_iter,
                       void* stream);
/* x_test: [mt, d], walked in blocks of rhs_cap; cov_mode NNGP_COV_NONE / NNGP_COV_DIAG; mean: [mt, ny]; var: [mt] (NULL with
 * NNGP_COV_NONE).  rc 1: some block's solve did not reach tol (every block is still computed and written). */
int nngp_matfree_predict(nngp_matfree* h, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var, double tol,
                         int32_t max_iter, void* stream);
/* alpha_out: [n, ny] like y (device). */
int nngp_matfree_alpha(nngp_matfree* h, double* alpha_out, void* stream);
/* info: host. */
int nngp_matfree_info(nngp_matfree* h, nngp_matfree_info_t* info);

/* The fused operator on its own (csrc/kmv_f64.hip): out [r, ldo] = (K(x, x) + diag_add I) v for x [n, d] and v [r, ldv], RHS-major,
 * ldo, ldv >= n, out and v distinct.  K is never written to memory.  Entries of out beyond column n and vectors beyond r are not
 * touched, those of v never read.  Two calls on the same input give the same bytes, and a vector's result does not depend on r.
 * Stand-alone form for tests and integration: it allocates and frees the rows' norms and its split partials on the stream. */
int nngp_kmv_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int32_t r, const double* x, int64_t n, int32_t d,
                 const nngp_arch_act* arch, double diag_add, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_MATFREE_H */
