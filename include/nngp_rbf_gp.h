/* nngp_rbf_gp.h -- C ABI of the float64 RBF Gaussian process in libnngp_hip.so (gfx950): the reference's
 * --kernel_type gp (train.py:60-150, GP_train_and_test, dispatched at train.py:243-244).
 *
 * Same conventions as nngp_hip.h (device pointers unless marked host, row-major float64, stream = hipStream_t as
 * void*, 0 = success and < 0 = error with nngp_last_error()).  Kept apart from nngp_hip.h because these entry points
 * have no host build: they run on the GPU only.
 */
#ifndef NNGP_RBF_GP_H
#define NNGP_RBF_GP_H

#include "nngp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- RBF Gaussian process, float64 --------------------------------------------------------------------------------------
 * The reference's second model: an RBF GP whose hyperparameters (amplitude, noise, length scale) are trained by adaptive
 * gradient steps on the negative log marginal likelihood, then used to predict.  With raw = (p_amp, p_noise, p_ls) and
 * (amp, noise, ls) = softplus(raw):
 *   K_ij = exp(-|x_i / ls - x_j / ls|^2),  A = amp K + (noise + 1e-6) I,  A = L L^T,  alpha = A^-1 (y - mean(y)),
 *   NLML = 1/2 y^T alpha + sum log L_ii + (N/2) c - c/2 - (log amp)^2,  c = log(2 * 3.1415)   (train.py:96-102)
 * and grad_raw = dNLML/draw analytically (W = alpha alpha^T - A^-1; dNLML/dtheta = -1/2 sum W o dA/dtheta + prior term).
 * Everything is float64 and has its own factorisation; the NNGP model is not involved.  One handle is driven from one
 * stream at a time.  No device allocation after create except in predict when mt > m_cap.                             */
typedef struct nngp_rbf_gp nngp_rbf_gp;
int nngp_rbf_gp_create(nngp_rbf_gp** out, int64_t n_cap, int64_t m_cap, int32_t d);
int nngp_rbf_gp_destroy(nngp_rbf_gp* gp);
/* x: [n, d], y: [n, ny] (ny must be 1).  Keeps a copy of x and y - mean(y); mean(y) is added back by predict. */
int nngp_rbf_gp_set_train(nngp_rbf_gp* gp, const double* x, const double* y, int64_t n, int32_t ny, void* stream);
/* Builds A for raw (host, 3 values), factors it and keeps the factor.  nlml: host.  grad_raw: host, 3 values, or NULL for
 * the NLML alone (no A^-1).  Synchronises the stream.  A pivot that is not positive returns rc < 0 naming its column. */
int nngp_rbf_gp_evaluate(nngp_rbf_gp* gp, const double* raw, double* nlml, double* grad_raw, void* stream);
/* The reduced sums of the last evaluation with a gradient (host, 8 values): sum log L_ii, y^T A^-1 y, alpha^T K alpha,
 * tr(A^-1 K), alpha^T (K o D2) alpha, tr(A^-1 (K o D2)), alpha^T alpha, tr(A^-1)   (D2: squared distances of x / ls). */
int nngp_rbf_gp_terms(const nngp_rbf_gp* gp, double* out);
/* Posterior at the last evaluated parameters (train.py:118-124): mean [mt] = amp K(X_t, X) alpha + mean(y); cov_mode
 * NNGP_COV_DIAG: var_or_cov [mt] = diag(amp K(X_t, X_t) - V^T V), V = L^-1 amp K(X, X_t); NNGP_COV_FULL: [mt, mt]. */
int nngp_rbf_gp_predict(nngp_rbf_gp* gp, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var_or_cov,
                        void* stream);
/* K(x1, x2) alone (x2 NULL: x1 against itself) into out [n1, ld]: exp(-|x1_i / ls - x2_j / ls|^2). */
int nngp_rbf_gp_kernel(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d, double ls, double* out, int64_t ld,
                       void* stream);
/* Device factor of the last evaluation: L in the lower triangle of [n_padded, ld] (identity on the padding; the part
 * above the diagonal blocks is workspace, read the lower triangle only). */
int nngp_rbf_gp_factor_buffer(const nngp_rbf_gp* gp, double** l, int64_t* ld, int64_t* n_padded);
/* Blocked lower Cholesky of a float64 matrix in place (n multiple of 128, ld >= n even); the lower triangle receives L.
 * A pivot that is not positive returns rc < 0 with a message naming the column; nothing is clamped.  Synchronises.
 * The strict upper triangle of the input is never read.  On return the part above the 128 x 128 diagonal blocks is
 * workspace (inside the diagonal blocks the upper triangle is zero): read the lower triangle only. */
int nngp_potrf_f64(double* a, int64_t n, int64_t ld, void* stream);

/* ---- the float64 core on its own: what every float64 model above and in nngp_mll.h / nngp_sparse.h factors and solves with ----
 * The same factorisation, keeping the inverted diagonal blocks: dinv [n, 128], block kb at dinv + kb * 128 * 128 holds
 * L_kk^-1 (lower, zero above the diagonal), which every panel and every solve multiplies by. */
int nngp_potrf_dinv_f64(double* a, int64_t n, int64_t ld, double* dinv, void* stream);
/* bt [rows, ldb] <- bt L^-T in place (each row b becomes L^-1 b), with l [n, ldl] and dinv as nngp_potrf_dinv_f64 left them.
 * rows and n are multiples of 128, ldb and ldl even and >= n, the pointers 16-byte aligned.  tri != 0: bt holds the identity
 * (rows == n), the result L^-T is upper triangular and only the rows down to the end of each column's diagonal block are
 * written; the rest of bt is not touched.  The rows x 128 scratch is allocated and freed in stream order. */
int nngp_trsm_fwd_f64(double* bt, int64_t ldb, int64_t rows, const double* l, int64_t ldl, const double* dinv, int64_t n, int32_t tri,
                      void* stream);
/* The evaluation sequence of the models on a caller's matrix: a [n, lda] (lower triangle read), y [n], any n >= 1, padded
 * inside to Np = n rounded up to 128 with the identity.  mode 0: L and w = L^-1 y; mode 1: also L^-T, A^-1 = L^-T L^-1,
 * alpha = A^-1 y and neg_rowsq = -diag(A^-1); mode 2: as mode 1 without the A^-1 product.  alpha has the same bits in modes 1
 * and 2, with or without neg_rowsq.  Outputs (each may be NULL): l, zt, ainv [Np, Np]; w, alpha, neg_rowsq [Np].  An output
 * the mode does not produce must be NULL (rc < 0).  Allocates and frees its workspace; synchronises. */
int nngp_factor_solve_f64(const double* a, int64_t lda, const double* y, int64_t n, int32_t mode, double* l, double* w, double* zt,
                          double* ainv, double* alpha, double* neg_rowsq, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_RBF_GP_H */
