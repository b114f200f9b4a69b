/* nngp_sparse.h -- C ABI of the sparse (inducing-point, DTC) NNGP posterior in libnngp_hip.so (gfx950).
 *
 * The exact models hold the N x N kernel and pay N^3 / 3.  The sparse model keeps every label, summarises the inputs by
 * m << N inducing rows U and pays O(N m^2) once and O(m^2) per served query.  Everything is float64.  With mp = m rounded
 * up to 128 (the padding rows and columns are the identity):
 *
 *   sigma2 = diag_reg * (sum_i K(x_i, x_i)) / n   over all rows added so far (diag_reg itself with the absolute flag)
 *   K_uu  <- K(U, U) + jitter * trace(K(U, U)) / m * I,      L_u = chol(K_uu)         (nothing is clamped)
 *   for each chunk X_c, Y_c of at most chunk_rows rows:
 *       Vt = K(X_c, U) L_u^-T  [c, mp];   G += Vt^T Vt (lower triangle);   R += Vt^T Y_c  [mp, ny];   tr += sum K_ii;   n += c
 *   finish:   B = sigma2 I + G  (a second buffer: G survives for later rows),   L_B = chol(B),   C = L_B^-1 R
 *   predict:  p = L_u^-1 K(U, x),  q = L_B^-1 p,  mean = q . C,  var = K(x, x) - |p|^2 + sigma2 |q|^2,
 *             cov = K_tt - P P^T + sigma2 Q Q^T   (the covariance of the latent function, as in the exact model)
 *
 * With U = X and jitter = 0 this is the exact GP posterior.  Only the NNGP kernel: the NTK posterior covariance has no DTC
 * analogue.  Same conventions as nngp_hip.h: 0 on success, non-zero with text in nngp_last_error(), -2 for argument errors
 * before any GPU work; device pointers; work is enqueued on `stream`.  One handle is driven from one stream at a time.
 * GPU library only (no host build), like nngp_activations.h.
 */
#ifndef NNGP_SPARSE_H
#define NNGP_SPARSE_H

#include "nngp_additive.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nngp_sparse nngp_sparse;

typedef struct nngp_sparse_info_t {
    int64_t n;            /* training rows added since the last set_inducing */
    int64_t m;            /* inducing rows */
    int64_t m_padded;     /* m rounded up to 128 */
    int64_t chunks;       /* chunks accumulated since the last set_inducing */
    double sigma2;        /* the noise of the last finish (0 before it) */
    double trace_mean;    /* (sum K_ii) / n of the rows added so far (0 while n = 0) */
    double jitter_added;  /* jitter * trace(K(U, U)) / m, what set_inducing added to the diagonal of K_uu */
} nngp_sparse_info_t;

/* All device memory is allocated here: three mp^2 matrices (L_u, G, B / L_B), their two sets of inverted diagonal blocks,
 * the chunk_rows x mp chunk buffer, two test_cap x mp buffers, the split partials of the Gram kernel (sized for whichever
 * m <= m_cap needs most of them) and small vectors;
 * add_rows, finish and predict add nothing to nngp_alloc_count().  The one exception: NNGP_COV_FULL keeps all mt rows of
 * P and Q and an mt x mt scratch, allocated on first use and grown when a later call has more rows.
 * m_cap (1 .. 16384) is rounded up to a multiple of 128; chunk_rows is a positive multiple of 128; test_cap >= 1 is rounded up
 * likewise; 1 <= ny <= 16; diag_reg and jitter finite and >= 0.  groups: NULL for the plain kernel, else as in nngp_additive.h. */
int nngp_sparse_create(nngp_sparse** out, int64_t m_cap, int64_t chunk_rows, int64_t test_cap, int32_t d, int32_t ny,
                       const nngp_arch_act* arch, const nngp_groups* groups, double diag_reg, int32_t diag_reg_absolute_scale,
                       double jitter);
int nngp_sparse_destroy(nngp_sparse* h);
/* u: [m, d], 1 <= m <= m_cap.  Builds K_uu, adds the jitter, factors it, zeroes G, R, tr and n, and synchronises the stream
 * for the pivot status: a pivot that is not positive returns rc < 0 and names its column (the handle then has no inducing set
 * and accepts another one). */
int nngp_sparse_set_inducing(nngp_sparse* h, const double* u, int64_t m, void* stream);
/* x: [n, d], y: [n, ny], n >= 1: walked in chunks of chunk_rows.  Legal before and after nngp_sparse_finish; rows added after a
 * finish take part in the next one (predict wants a finish after the last add_rows). */
int nngp_sparse_add_rows(nngp_sparse* h, const double* x, const double* y, int64_t n, void* stream);
/* B = sigma2 I + G, its factor and C.  Repeatable.  Synchronises the stream for the pivot status. */
int nngp_sparse_finish(nngp_sparse* h, void* stream);
/* x_test: [mt, d], walked in blocks of test_cap.  cov_mode NNGP_COV_NONE / NNGP_COV_DIAG / NNGP_COV_FULL; mean: [mt, ny];
 * var_or_cov: [mt] or [mt, mt] (NULL with NNGP_COV_NONE). */
int nngp_sparse_predict(nngp_sparse* h, const double* x_test, int64_t mt, int32_t cov_mode, double* mean, double* var_or_cov,
                        void* stream);
/* info: host.  Waits for the handle's work. */
int nngp_sparse_info(nngp_sparse* h, nngp_sparse_info_t* info);

/* The Gram product of a tall row-major block, contracting over its rows (csrc/sparse_gp.hip: k_syrk_tn_f64):
 *   C_lower [mp, mp] = beta * C_lower + A^T A   and, when r is given,   R [mp, ny] = beta * R + A^T Y.
 * a: [rows, mp] with leading dimension lda >= mp (even, the pointer 16-byte aligned); y: [rows, ny], 1 <= ny <= 16 (read only
 * with r); rows >= 1; mp a positive multiple of 128; c: leading dimension ldc >= mp.  Only the 128 x 128 tiles on or below the
 * diagonal are written (the diagonal tiles in full).  Two calls on the same input give the same bits.  Stand-alone form for
 * tests and integration: it allocates and frees its split partials on the stream. */
int nngp_syrk_tn_f64(double* c, int64_t ldc, double* r, const double* a, int64_t lda, const double* y, int64_t rows, int64_t mp,
                     int32_t ny, double beta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_SPARSE_H */
