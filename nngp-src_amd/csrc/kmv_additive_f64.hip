// The additive forms of the matrix-free operator (include/nngp_matfree_additive.h): the instantiations of k_kmv_f64 with the group
// walk of k_build_add in front of each tile (kmv_kernel.h), in a translation unit of their own, and the stand-alone call.
#include "kmv_kernel.h"

namespace nngp {

// one pass of w = 16 or 64 vectors.  general picks the whole-input term's map, as in the plain form; the group terms take group_map
// for every architecture
void launch_kmv_tiles_additive(int w, bool general, unsigned grid, const KmvAddArgs& a, const ArchDev& arch, hipStream_t s) {
    if (w == 64) {
        if (general) hipLaunchKernelGGL((k_kmv_f64<4, true, true>), dim3(grid), dim3(256), 0, s, a, arch);
        else hipLaunchKernelGGL((k_kmv_f64<4, false, true>), dim3(grid), dim3(256), 0, s, a, arch);
    } else {
        if (general) hipLaunchKernelGGL((k_kmv_f64<1, true, true>), dim3(grid), dim3(256), 0, s, a, arch);
        else hipLaunchKernelGGL((k_kmv_f64<1, false, true>), dim3(grid), dim3(256), 0, s, a, arch);
    }
}

}  // namespace nngp

using namespace nngp;

// include/nngp_matfree_additive.h: the operator of the summed kernel.  The call makes its own copy of the group table and waits
// for its work, as the stand-alone additive build does; the plain table takes nngp_kmv_f64 itself.
extern "C" int nngp_kmv_additive_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int32_t r, const double* x, int64_t n,
                                     int32_t d, const nngp_arch_act* arch, const nngp_groups* groups, double diag_add, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    NNGP_TRY(kmv_check(out, ldo, v, ldv, r, x, n, d, ad, diag_add));
    GroupsDev gd{};
    bool plain = false;
    NNGP_TRY(groups_create(groups, d, &gd, &plain));
    if (plain) return nngp_kmv_f64(out, ldo, v, ldv, r, x, n, d, arch, diag_add, stream);
    ad.groups = &gd;
    const int64_t wsd = kmv_ws_doubles(n, r);
    double* q = nullptr;
    double* ws = nullptr;
    int rc = 0;
    if (hipMallocAsync(reinterpret_cast<void**>(&q), sizeof(double) * (size_t)n, s) != hipSuccess ||
        hipMallocAsync(reinterpret_cast<void**>(&ws), sizeof(double) * (size_t)wsd, s) != hipSuccess) {
        set_error("kmv_additive_f64: no room for the norms and %lld doubles of partials", (long long)wsd);
        rc = -1;
    }
    if (rc == 0) rc = launch_row_sqnorm(x, n, d, q, s);
    if (rc == 0) rc = launch_kmv_f64(out, ldo, v, ldv, r, x, q, n, d, ad, diag_add, ws, wsd, s);
    if (ws) (void)hipFreeAsync(ws, s);
    if (q) (void)hipFreeAsync(q, s);
    if (hipStreamSynchronize(s) != hipSuccess && rc == 0) {
        set_error("kmv_additive_f64: the stream reported an error");
        rc = -1;
    }
    groups_destroy(&gd);
    return rc;
}
