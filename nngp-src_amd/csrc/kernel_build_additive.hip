// Additive NNGP / NTK kernel over feature groups (include/nngp_additive.h) for gfx950:
//   K(x, x') = w0 K_arch(x, x') + sum_g w_g K_arch(x_g, x'_g),   x_g = x[begin_g:end_g].
//
// The whole-input term is the kernel build of kernel_build.hip, written in float64 to the output itself (or to scratch when only
// float32 outputs are asked for).  k_build_add then computes, one 64 x 64 tile per 256-thread workgroup and 4 x 4 entries per
// thread, the group sum on the float64 VALU and adds it to that result in float64:
//   * a group's Gram entries x_g . x'_g are as short as one or two products, so they are accumulated from row slices staged in
//     LDS (k-chunks of 8, the next chunk's global loads in flight while the current one is consumed) -- no padded MFMA
//     (group_walk of kernel_tile.h, shared with the matrix-free operator's additive form);
//   * the two diagonal entries |x_g|^2, |x'_g|^2 of every entry come from the SAME staged values in the SAME order of
//     operations as the Gram entry.  Two rows whose slice is bit-identical (untouched default predicates: the common case) then
//     give k == q == q' bit for bit and are taken through the diagonal form of the map (theta = 0 exactly), instead of a square
//     root of the rounding noise of q q' - k^2.  The diagonal of a symmetric build is such a pair, so it needs no flag of its own;
//   * the layer recursion per group is the one of kernel_build.hip (act_cross / act_diag of act_map.h: ReLU, ABRelu, Erf,
//     biases, NNGP and NTK); the sum over groups is carried in float64 registers, in the table's order, without atomics;
//   * every output is written from the float64 sum: float64, float32 (+ the regulariser on its diagonal), the mirror image of an
//     off-diagonal tile of a symmetric build (transposed through LDS), the float32 copy's lower triangle only when asked.
// Cost: one map evaluation per group and entry, against one for the plain kernel, plus one read-modify-write of K.
#include "kernel_tile.h"
#include <math.h>
#include <vector>

namespace nngp {

namespace {

struct AddArgs {
    BuildArgs a;           // the caller's build: operands, range, outputs
    const double* full_n;  // the whole-input term, float64, indexed like the outputs (NULL: full_weight == 0 or not wanted)
    const double* full_t;
    int64_t ldf;
    GroupsDev g;
};

// NTK: the Theta outputs are wanted too (otherwise the NTK chain is dead code and its sums take no registers).
template <bool NTK>
__global__ __launch_bounds__(256) void k_build_add(AddArgs p, ArchDev arch, int64_t tiles_c, int vec_ok) {
    __shared__ __attribute__((aligned(16))) double smem[KT * LDP];  // As | Bs while the groups are walked, T for the mirror
    __shared__ __attribute__((aligned(16))) double tab[65 * 4];
    const BuildArgs& a = p.a;

    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    int64_t bi, bj;
    if (a.sym) {
        lower_tile(blockIdx.x, &bi, &bj);
    } else {
        bi = blockIdx.x / tiles_c;
        bj = blockIdx.x % tiles_c;
    }
    const int64_t i0 = a.row_begin + bi * KT, j0 = bj * KT;
    const int64_t i_end = a.row_end, j_end = a.n2;
    for (int i = tid; i < 65 * 4; i += 256) tab[i] = kTrigTab[i >> 2][i & 3];  // read after the first barrier below

    // the group sum, in the table's order, in float64 registers (group_walk of kernel_tile.h; tab is read after its first barrier)
    double sn[4][4], st[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) sn[r][c] = st[r][c] = 0.0;
    group_walk<NTK>(GroupLay4x4{}, PanelRows{a.x1, i0, i_end}, PanelRows{a.x2, j0, j_end}, a.d, p.g, arch, tab, smem,
                    [&](double wg, const double (&k)[4][4], const double (&t)[4][4]) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                sn[r][c] = fma(wg, k[r][c], sn[r][c]);
                                if (NTK) st[r][c] = fma(wg, t[r][c], st[r][c]);
                            }
                    });

    // ---- the whole-input term, then every output from the float64 sum ----
    const double w0 = p.g.full_weight;
    const bool vec = vec_ok != 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t gi = i0 + ty + 16 * r, gj = j0 + tx * 4;
        if (gi < i_end) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (gj + c >= j_end) continue;
                if (p.full_n != nullptr) sn[r][c] = fma(w0, p.full_n[gi * p.ldf + gj + c], sn[r][c]);
                if (NTK && p.full_t != nullptr) st[r][c] = fma(w0, p.full_t[gi * p.ldf + gj + c], st[r][c]);
            }
        }
        tile_store_4x4<NTK>(a, i0, j0, r, sn, st, vec);
    }
    if (a.sym && bi != bj) tile_mirror_4x4<NTK>(a, i0, j0, smem, sn, st, vec);
}

// K's diagonal of the summed kernel, one row per thread: sum_g w_g diag(q_g) in the table's order, then the whole-input term from
// q = |x|^2 / d -- the operations of k_build_add on an entry (i, i), in their order.
__global__ __launch_bounds__(256) void k_diag_add(const double* __restrict__ x, const double* __restrict__ q, int64_t n, int d,
                                                  ArchDev arch, GroupsDev gr, double* __restrict__ dn, double* __restrict__ dt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* tab = &kTrigTab[0][0];
    const double* xr = x + i * (int64_t)d;
    double sn = 0.0, st = 0.0;
    for (int g = 0; g <= gr.n_groups; ++g) {  // the last pass is the whole-input term
        const bool full = g == gr.n_groups;
        if (full && gr.full_weight == 0.0) break;
        double k;
        if (full) {
            k = q[i];
        } else {
            const int kb = gr.begin[g], ke = gr.end[g];
            double s = 0.0;
            for (int f = kb; f < ke; ++f) s = fma(xr[f], xr[f], s);
            k = s * (1.0 / (double)(ke - kb));
        }
        double t = 0.0;
        diag_chain_act(arch, tab, k, t);
        const double w = full ? gr.full_weight : gr.weight[g];
        sn = fma(w, k, sn);
        st = fma(w, t, st);
    }
    if (dn) dn[i] = sn;
    if (dt) dt[i] = st;
}

}  // namespace

int groups_create(const nngp_groups* g, int d, GroupsDev* out, bool* plain) {
    *out = GroupsDev{};
    *plain = false;
    NNGP_REQUIRE(g != nullptr, "groups: the group table is NULL");
    NNGP_REQUIRE(g->n_groups >= 0 && g->n_groups <= NNGP_MAX_GROUPS, "groups: n_groups must be in [0, %d] (got %d)",
                 NNGP_MAX_GROUPS, g->n_groups);
    NNGP_REQUIRE(g->n_groups == 0 || (g->begin != nullptr && g->end != nullptr && g->weight != nullptr),
                 "groups: begin / end / weight is NULL");
    NNGP_REQUIRE(std::isfinite(g->full_weight) && g->full_weight >= 0.0, "groups: full_weight must be finite and >= 0");
    std::vector<double> w;
    std::vector<int> be;  // begins, then ends
    for (int i = 0; i < g->n_groups; ++i) {
        NNGP_REQUIRE(0 <= g->begin[i] && g->begin[i] < g->end[i] && g->end[i] <= d,
                     "groups: group %d has the range [%d, %d), outside 0 <= begin < end <= d = %d", i, g->begin[i], g->end[i], d);
        NNGP_REQUIRE(std::isfinite(g->weight[i]) && g->weight[i] >= 0.0, "groups: weight %d must be finite and >= 0", i);
    }
    for (int i = 0; i < g->n_groups; ++i)
        if (g->weight[i] > 0.0) {
            w.push_back(g->weight[i]);
            be.push_back(g->begin[i]);
        }
    for (int i = 0; i < g->n_groups; ++i)
        if (g->weight[i] > 0.0) be.push_back(g->end[i]);
    const int n = (int)w.size();
    NNGP_REQUIRE(n > 0 || g->full_weight > 0.0, "groups: all weights are zero");
    out->n_groups = n;
    out->full_weight = g->full_weight;
    if (n == 0) {
        *plain = g->full_weight == 1.0;
        return 0;
    }
    char* buf = nullptr;
    NNGP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&buf), (sizeof(double) + 2 * sizeof(int)) * (size_t)n));
    note_alloc();
    if (hipMemcpy(buf, w.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(buf + sizeof(double) * n, be.data(), 2 * sizeof(int) * n, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(buf);
        set_error("groups: could not copy the group table to the device");
        *out = GroupsDev{};
        return -1;
    }
    out->weight = reinterpret_cast<const double*>(buf);
    out->begin = reinterpret_cast<const int*>(buf + sizeof(double) * n);
    out->end = out->begin + n;
    return 0;
}

void groups_destroy(GroupsDev* g) {
    if (g->weight != nullptr) (void)hipFree(const_cast<double*>(g->weight));
    *g = GroupsDev{};
}

int launch_diag_additive(const double* x, const double* q, int64_t n, int d, const ArchDev& arch, double* dn, double* dt,
                         hipStream_t s) {
    if (n <= 0) return 0;
    NNGP_REQUIRE(arch.groups != nullptr, "diag_additive: no group table");
    ArchDev plain = arch;
    plain.groups = nullptr;
    hipLaunchKernelGGL(k_diag_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, q, n, d, plain, *arch.groups, dn, dt);
    NNGP_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_kernel_build_additive(const BuildArgs& a, const ArchDev& arch, hipStream_t s) {
    NNGP_REQUIRE(arch.groups != nullptr, "kernel_build_additive: no group table");
    const GroupsDev& g = *arch.groups;
    ArchDev plain = arch;
    plain.groups = nullptr;
    const bool want_n = a.nngp64 != nullptr || a.nngp32 != nullptr, want_t = a.ntk64 != nullptr || a.ntk32 != nullptr;
    int64_t tiles_r, tiles_c, nblocks;
    int vec_ok;
    NNGP_TRY(plan_build_tiles(a, false, &tiles_r, &tiles_c, &nblocks, &vec_ok));
    if (nblocks == 0) return 0;

    // 1. the whole-input term in float64: into the float64 outputs themselves, or into scratch when a wanted kernel has none
    AddArgs p{};
    p.a = a;
    p.g = g;
    double* scratch = nullptr;
    if (g.full_weight != 0.0) {
        BuildArgs f = a;
        f.nngp32 = nullptr; f.ntk32 = nullptr;
        f.diag_add_nngp32 = f.diag_add_ntk32 = 0.0;
        f.lower32 = 0;
        if ((want_n && a.nngp64 == nullptr) || (want_t && a.ntk64 == nullptr)) {
            const int64_t ldf = round_up(a.n2, 2);
            const int64_t each = a.row_end * ldf;  // indexed by the absolute row, like the outputs (rows below row_begin unused)
            NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&scratch), sizeof(double) * each * ((want_n ? 1 : 0) + (want_t ? 1 : 0)), s));
            f.ld64 = ldf;
            f.nngp64 = want_n ? scratch : nullptr;
            f.ntk64 = want_t ? scratch + (want_n ? each : 0) : nullptr;
        }
        const int rc = launch_kernel_build_plain(f, plain, s);
        if (rc != 0) {
            if (scratch) (void)hipFreeAsync(scratch, s);
            return rc;
        }
        p.full_n = f.nngp64;
        p.full_t = f.ntk64;
        p.ldf = f.ld64;
    }

    // 2. the group sum, added in float64; every output from the sum
    if (want_t)
        hipLaunchKernelGGL(k_build_add<true>, dim3((unsigned)nblocks), dim3(256), 0, s, p, plain, tiles_c, vec_ok);
    else
        hipLaunchKernelGGL(k_build_add<false>, dim3((unsigned)nblocks), dim3(256), 0, s, p, plain, tiles_c, vec_ok);
    const hipError_t e = hipGetLastError();
    if (scratch) (void)hipFreeAsync(scratch, s);
    NNGP_HIP_CHECK(e);
    return 0;
}

}  // namespace nngp
