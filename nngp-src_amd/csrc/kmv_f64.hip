// The matrix-free NNGP operator: OUT = (K(X, X) + diag_add I) V for a block of r vectors, K never written to memory.
//
//   k_kmv_f64      (kmv_kernel.h; the plain forms are instantiated here, the additive ones in kmv_additive_f64.hip)
//                  one workgroup owns a 64-column block of K and a contiguous range of 64-row tiles.  Per tile it calls the pieces
//                  of the kernel build (kernel_tile.h, the ones k_build_mfma of kernel_build.hip is made of: gram_mfma_64 stages
//                  the X panels through LDS in k-chunks of 16 and forms the Gram block on v_mfma_f64_16x16x4_f64; relu_block_map /
//                  gen_block_map run the layer recursion in the accumulator layout, without the NTK chain; stage_layer_q) and then
//                  multiplies the finished block into the vectors without moving it: the C/D layout of the float64 MFMA is
//                  col = lane & 15, row = (lane >> 4) + 4 reg, and its B operand is one value per lane at (k = lane >> 4,
//                  col = lane & 15), so register `reg` of a finished 16 x 16 block IS the operand B[k][j] = K[4 reg + k][j].  With
//                  A[c][k] = V[c][i0 + 4 reg + k] (the V tile staged through LDS: the lanes of that operand read 16 different
//                  vectors) the second MFMA accumulates OUT^T[c, j] += sum_i V[c, i] K[i, j] -- row block i's contribution to the
//                  output rows of COLUMN block j, the whole product because K is symmetric.
//                  The two waves that share a column half are summed through LDS (upper rows + lower rows, fixed), and the
//                  workgroup writes one partial [16 RB vectors][64 columns].
//   k_kmv_reduce   OUT[c, j] = sum over the row splits in ascending order + diag_add V[c, j].
// No atomics, no counters, no cooperative launch: the launch boundary is the only synchronisation (as in k_syrk_tn_f64).  The
// split is a function of n alone, each vector's sums never see another vector (one MFMA output column each), so a vector's result
// does not depend on r, on its position in the block or on the pass width, and two calls give the same bytes.
#include "kmv_kernel.h"

#include <cmath>

namespace nngp {

namespace {

constexpr int kKmvTargetGroups = 2048;  // workgroups wanted when the column blocks alone are fewer

// one workgroup per column block: OUT[c, j] = sum over the splits, ascending, + diag_add V[c, j]
__global__ __launch_bounds__(256) void k_kmv_reduce(double* __restrict__ out, int64_t ldo, const double* __restrict__ v, int64_t ldv,
                                                    int rc, int w, int64_t n, int64_t nb, int nsplit, const double* __restrict__ part,
                                                    double diag_add) {
    const int64_t cb = blockIdx.x;
    for (int e = threadIdx.x; e < rc * KT; e += 256) {
        const int c = e >> 6, col = e & 63;
        const int64_t gj = cb * KT + col;
        if (gj >= n) continue;
        double s = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) s += part[(((int64_t)sp * nb + cb) * w + c) * KT + col];
        out[(int64_t)c * ldo + gj] = s + diag_add * v[(int64_t)c * ldv + gj];
    }
}

// the row tiles are cut into nsplit runs of `per`; a function of n alone
int kmv_splits(int64_t n, int64_t* per) {
    const int64_t nb = (n + KT - 1) / KT;
    int64_t want = (kKmvTargetGroups + nb - 1) / nb;
    if (want > nb) want = nb;
    *per = (nb + want - 1) / want;
    return (int)((nb + *per - 1) / *per);
}

}  // namespace

int64_t kmv_ws_doubles(int64_t n, int r) {
    int64_t per;
    const int64_t nb = (n + KT - 1) / KT, ns = kmv_splits(n, &per);
    return ns * nb * KT * (r > 16 ? 64 : 16);
}

// the checks that both forms share
static int kmv_check_args(const double* out, int64_t ldo, const double* v, int64_t ldv, int r, const double* x, int64_t n, int d,
                          double diag_add) {
    NNGP_REQUIRE(out != nullptr && v != nullptr && x != nullptr && out != v, "kmv_f64: NULL argument, or out aliases v");
    NNGP_REQUIRE(n >= 1 && n <= ((int64_t)1 << 26) && d >= 1 && r >= 1 && r <= 65536,
                 "kmv_f64: need 1 <= n <= 2^26, d >= 1 and 1 <= r <= 65536 (n=%lld, d=%d, r=%d)", (long long)n, d, r);
    NNGP_REQUIRE(ldo >= n && ldv >= n, "kmv_f64: leading dimensions must be >= n (ldo=%lld, ldv=%lld, n=%lld)", (long long)ldo,
                 (long long)ldv, (long long)n);
    NNGP_REQUIRE(std::isfinite(diag_add), "kmv_f64: diag_add must be finite");
    return 0;
}

int kmv_check(const double* out, int64_t ldo, const double* v, int64_t ldv, int r, const double* x, int64_t n, int d, const ArchDev& arch,
              double diag_add) {
    NNGP_TRY(kmv_check_args(out, ldo, v, ldv, r, x, n, d, diag_add));
    NNGP_REQUIRE(arch.groups == nullptr, "kmv_f64: additive kernels are not supported by the fused operator");
    return 0;
}

int launch_kmv_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int r, const double* x, const double* q, int64_t n, int d,
                   const ArchDev& arch, double diag_add, double* ws, int64_t ws_doubles, hipStream_t s) {
    NNGP_TRY(kmv_check_args(out, ldo, v, ldv, r, x, n, d, diag_add));
    NNGP_REQUIRE(q != nullptr && ws != nullptr && ws_doubles >= kmv_ws_doubles(n, r), "kmv_f64: workspace missing or too small");
    const bool add = arch.groups != nullptr;  // the additive form; the kernels take the table by value
    ArchDev plain = arch;
    plain.groups = nullptr;
    KmvAddArgs a{};
    if (add) a.g = *arch.groups;
    a.x = x;
    a.q = q;
    a.n = n;
    a.d = d;
    a.ldv = ldv;
    a.part = ws;
    a.nb = (n + KT - 1) / KT;
    a.nsplit = kmv_splits(n, &a.per);
    const unsigned grid = (unsigned)(a.nb * a.nsplit);
    // passes of 64 vectors while more than 16 remain, one of 16 for a short tail: each pass builds K once
    for (int c0 = 0; c0 < r;) {
        const int rem = r - c0, w = rem > 16 ? 64 : 16;
        a.v = v + (int64_t)c0 * ldv;
        a.rc = rem < w ? rem : w;
        const KmvArgs& pa = a;
        if (add) {
            launch_kmv_tiles_additive(w, arch.general != 0, grid, a, plain, s);
        } else if (w == 64) {
            if (arch.general) hipLaunchKernelGGL((k_kmv_f64<4, true, false>), dim3(grid), dim3(256), 0, s, pa, arch);
            else hipLaunchKernelGGL((k_kmv_f64<4, false, false>), dim3(grid), dim3(256), 0, s, pa, arch);
        } else {
            if (arch.general) hipLaunchKernelGGL((k_kmv_f64<1, true, false>), dim3(grid), dim3(256), 0, s, pa, arch);
            else hipLaunchKernelGGL((k_kmv_f64<1, false, false>), dim3(grid), dim3(256), 0, s, pa, arch);
        }
        hipLaunchKernelGGL(k_kmv_reduce, dim3((unsigned)a.nb), dim3(256), 0, s, out + (int64_t)c0 * ldo, ldo, a.v, ldv, a.rc, w, n, a.nb,
                           a.nsplit, a.part, diag_add);
        NNGP_HIP_CHECK(hipGetLastError());
        c0 += a.rc;
    }
    return 0;
}

}  // namespace nngp

using namespace nngp;

extern "C" int nngp_kmv_f64(double* out, int64_t ldo, const double* v, int64_t ldv, int32_t r, const double* x, int64_t n, int32_t d,
                            const nngp_arch_act* arch, double diag_add, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    NNGP_TRY(kmv_check(out, ldo, v, ldv, r, x, n, d, ad, diag_add));
    const int64_t wsd = kmv_ws_doubles(n, r);
    double* q = nullptr;
    double* ws = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&q), sizeof(double) * (size_t)n, s));
    if (hipMallocAsync(reinterpret_cast<void**>(&ws), sizeof(double) * (size_t)wsd, s) != hipSuccess) {
        (void)hipFreeAsync(q, s);
        set_error("kmv_f64: no room for %lld doubles of partials", (long long)wsd);
        return -1;
    }
    int rc = launch_row_sqnorm(x, n, d, q, s);
    if (rc == 0) rc = launch_kmv_f64(out, ldo, v, ldv, r, x, q, n, d, ad, diag_add, ws, wsd, s);
    (void)hipFreeAsync(ws, s);
    (void)hipFreeAsync(q, s);
    return rc;
}
