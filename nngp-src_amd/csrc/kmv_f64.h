// kmv_f64.hip: the fused operator OUT = (K(X, X) + diag_add I) V of the matrix-free model (include/nngp_matfree.h).
#pragma once
#include "common.h"
#include "../../include/nngp_matfree.h"
#include "../../include/nngp_matfree_additive.h"

namespace nngp {
// doubles of split partials a product of r vectors over n rows needs (a function of n, and of whether r exceeds one 16-wide pass)
int64_t kmv_ws_doubles(int64_t n, int r);
// the argument checks alone (-2), before any GPU work
int kmv_check(const double* out, int64_t ldo, const double* v, int64_t ldv, int r, const double* x, int64_t n, int d, const ArchDev& arch,
              double diag_add);
// v, out: RHS-major [r, ld]; q: |x_i|^2 / d (launch_row_sqnorm); ws: kmv_ws_doubles(n, r) doubles at least.
// arch.groups set: the operator of the summed kernel (the additive form of the tile body)
int launch_kmv_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int r, const double* x, const double* q, int64_t n, int d,
                   const ArchDev& arch, double diag_add, double* ws, int64_t ws_doubles, hipStream_t s);
// kmv_additive_f64.hip: the additive forms' tile launch of one pass (the arguments of kmv_kernel.h)
struct KmvAddArgs;
void launch_kmv_tiles_additive(int w, bool general, unsigned grid, const KmvAddArgs& a, const ArchDev& arch, hipStream_t s);
}  // namespace nngp
