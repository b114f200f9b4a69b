/* nngp_i8s.h -- C ABI of the stand-alone operators of the sliced int8 product (csrc/gemm_i8s.hip) in libnngp_hip.so (gfx950).
 *
 * The posterior's residual product R = K_td - Z (K + reg I) runs on the int8 matrix pipe: every float64 row is scaled by its own
 * power of two and cut into `ns` balanced base-256 digits (one int8 plane per digit), the plane pairs are multiplied exactly in
 * int32 and a float64 pass combines them.  nngp_gemm_nt_i8s (nngp_hip.h) is the general product with both operands cut by their
 * own row maxima.  The calls below run the other launches of that pipeline -- the kernel-matrix cut with scales from the
 * diagonal, the symmetric cut, the write-back of the rounded rows, the fused row statistics and the floor estimate -- in the
 * order nngp_model_predict issues them, without a model object, for tests/test_gpu_i8s.py.
 *
 * Same conventions as nngp_hip.h: 0 on success, non-zero with text in nngp_last_error(); device pointers; asynchronous on
 * `stream`; every argument is checked before the first launch.  GPU library only (no host build), like nngp_activations.h.
 *
 * The digits of a row with scale s (a power of two) and ns planes: X = rint(x 2^(8 ns) / s) (ties to even; the scaling is exact),
 * X = sum_i dig_i 256^(ns-1-i), dig_i in [-128, 127] for i >= 1, plane 0 (the most significant) holding what is left as int8.
 * Own-row scales: the smallest power of two s with max|row| / s <= 126/256, so that plane 0 holds at most 126 + 1 (carry).
 *
 * Rows the planes cannot hold:
 *   - a row whose maximum is below 2^-960 counts as zero: scale 1, planes zero, write-back zero.  The error is the row itself
 *     (< 2^-960 per entry); a scale that small would overflow 2^(8 ns) / s.
 *   - a row with a NaN, an Inf or an entry >= 1e300 in magnitude gets the scale NaN: its write-back is NaN in every column and every
 *     entry of the product's row (for a row of the B operand: of its column) is NaN.  Its planes hold no meaning.  Write-back
 *     never turns a non-finite entry finite.
 *   - the kernel-matrix cut takes its scales from the diagonal and makes no pass over the matrix.  A DIAGONAL entry that is NaN,
 *     Inf or >= 1e300 in magnitude becomes the largest diagonal and gives EVERY row the scale NaN, as above.  A row whose product
 *     |K_ii| max_j |K_jj| overflows float64 (both from about 1e154 on) or whose bound reaches 1e300 gets the scale NaN too,
 *     although its entries are finite: the bound is formed as sqrt(|K_ii| max_j |K_jj|).  A non-finite entry OFF the diagonal
 *     is out of contract there (its digits are whatever the conversion leaves).
 *   - the estimate of k_i8s_floor_ratio reads a row in pairs; its launcher refuses an odd column count.  No entry point of this
 *     header can pass one (n is a multiple of 128), and nngp_model_predict does not use that launcher.
 */
#ifndef NNGP_I8S_H
#define NNGP_I8S_H

#include "nngp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src [rows, ld] f64 -> planes [ns][rows][ldp] int8, 2 <= ns <= 7.  Columns [cols, round_up(cols, 128)) of every plane row are
 * written as zero, bytes beyond that and the padding of src (columns >= cols) are not touched / not read beyond the pair that
 * holds the last column.  scale_in [rows] (powers of two, >= max|row| 256/126) or NULL: own-row scales, written to scale_out [rows].
 * writeback [rows, ld] or NULL, may be src: receives every row rounded to its digits, X s 2^(-8 ns), exactly what the planes hold.
 * ld even and >= cols, ldp a multiple of 16 and >= round_up(cols, 128), src / planes / writeback 16-byte aligned. */
int nngp_i8s_cut_rows(const double* src, int64_t ld, int64_t rows, int64_t cols, int32_t ns, const double* scale_in, double* scale_out,
                      int8_t* planes, int64_t ldp, double* writeback, void* stream);

/* The cut of a bitwise symmetric positive semi-definite src [n, n] (n a multiple of 128; padding rows and columns hold zeros):
 * scale_out [n] = own-row-scale rule applied to the bound sqrt(|K_ii| max_j |K_jj|) (1 + 1e-9) of row i, planes [ns][n][ldp] cut
 * with those scales -- by the symmetric kernel that reads every entry once (ns = 5 or 7), or with by_rows != 0 by the row kernel
 * (2 <= ns <= 7); both give the same bytes.  sqsum (or NULL): one f64, sum_i scale_out[i]^2. */
int nngp_i8s_cut_sym(const double* src, int64_t ld, int64_t n, int32_t ns, double* scale_out, int8_t* planes, int64_t ldp,
                     int32_t by_rows, double* sqsum, void* stream);

/* out [mp, n] = beta cin + alpha z kmat^T + gamma z  with z [mp, n] and the symmetric kmat [n, n] (mp, n multiples of 128):
 * the kernel-matrix cut of kmat into ns_k planes (sym != 0: the symmetric kernel, ns_k = 5 or 7), z cut into ns_z planes with
 * own-row scales (round_z != 0: z is overwritten by its rounded rows, and the product is that of the rounded z), the plane
 * pairs with ia + ib <= cut (cut beyond ns_z + ns_k - 2 is clamped), the float64 combination.  cin may be NULL when beta = 0 and
 * may be out.  Leading dimensions even and >= n.
 * Fused outputs, all of out32 / base / var / delta / zstat or none (they need cin): out32 [mp, n] f32 = (float)out;
 * var[r] = base[r] - sum_c z (cin + out), delta[r] = sum_c z out, zstat[2 r] = sum_c z^2, zstat[2 r + 1] = max_c |z|.
 * floor_rows (or NULL; needs the fused outputs): one f64, max_r of the floor estimate / var[r] from zstat (k_i8s_floor_ratio_rows);
 * floor_z (or NULL; likewise): the same from a pass over z itself (k_i8s_floor_ratio). */
int nngp_i8s_residual(double* out, int64_t ldo, const double* cin, int64_t ldcin, double* z, int64_t ldz, const double* kmat,
                      int64_t ldk, int64_t mp, int64_t n, double alpha, double beta, double gamma, int32_t ns_z, int32_t ns_k,
                      int32_t cut, int32_t round_z, int32_t sym, float* out32, const double* base, double* var, double* delta,
                      double* zstat, double* floor_rows, double* floor_z, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NNGP_I8S_H */
