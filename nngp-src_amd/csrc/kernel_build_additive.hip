// Additive NNGP / NTK kernel over feature groups (include/nngp_additive.h) for gfx950:
//   K(x, x') = w0 K_arch(x, x') + sum_g w_g K_arch(x_g, x'_g),   x_g = x[begin_g:end_g].
//
// The whole-input term is the kernel build of kernel_build.hip, written in float64 to the output itself (or to scratch when only
// float32 outputs are asked for).  k_build_add then computes, one 64 x 64 tile per 256-thread workgroup and 4 x 4 entries per
// thread, the group sum on the float64 VALU and adds it to that result in float64:
//   * a group's Gram entries x_g . x'_g are as short as one or two products, so they are accumulated from row slices staged in
//     LDS (k-chunks of 8, the next chunk's global loads in flight while the current one is consumed) -- no padded MFMA;
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

constexpr int GKC = 8;       // features staged per step

struct AddArgs {
    BuildArgs a;           // the caller's build: operands, range, outputs
    const double* full_n;  // the whole-input term, float64, indexed like the outputs (NULL: full_weight == 0 or not wanted)
    const double* full_t;
    int64_t ldf;
    GroupsDev g;
};

// lo with hi + lo = w2 * x + b2 to twice the working precision, for hi = fma(w2, x, b2): the product's and the sum's rounding
// errors, exactly (two-product by fma, two-sum), plus what the fma's single rounding left of them.
__device__ __forceinline__ double affine_lo(double w2, double x, double b2, double hi) {
    const double p = w2 * x, ep = fma(w2, x, -p);
    const double s = p + b2, bb = s - p;
    const double es = (p - (s - bb)) + (b2 - bb);
    return (s - hi) + (ep + es);
}

// act_cross of an Erf layer (act_map.h) with the bracket q1 q2 - k^2 taken from k, q1, q2 as hi + lo pairs.  A group's slices are
// nearly parallel far more often than whole rows are, and then r = 1 + 2 b^2 (q1 + q2) + 4 b^4 (q1 q2 - k^2) is left with
// r ~ 4 b^2 q while one rounding of the Dense layer's affine map is worth 4 b^4 u q^2 of it: at raw forest norms (q ~ 6e5) that is
// 5e-11 of Theta.  The first-order terms of the lo parts remove it (the operations on the hi parts are act_cross's own).
__device__ __forceinline__ void erf_cross_comp(const double* ap, double k, double kl, double q1, double q1l, double q2, double q2l,
                                               const double* __restrict__ tab, double& ko, double& kd) {
    const double kk = k * k;
    const double lo = fma(q1, q2l, fma(q2, q1l, -2.0 * (k * kl)));
    const double br = fmax((fma(q1, q2, -kk) + fma(-k, k, kk)) + lo, 0.0);
    const double w = fast_sqrt_pos(fma(ap[1] * ap[1], br, fma(ap[1], q1 + q2, 1.0)));
    ko = fma(ap[0], pi_minus_atan2(w, ap[1] * k, tab) - 0.5 * kPi, ap[2]);
    kd = ap[3] * fast_rcp(w);
}

// One group's term of a thread's 4 x 4 entries through Dense, (act, Dense)*: k[r][c] the Gram entries, q1[r] / q2[c] the diagonal
// entries of its rows / columns, all already normalised.  The layers are the outer loop, so a layer's map of the 4 + 4 diagonal
// entries runs once per thread and not once per entry.  same: k == q1 == q2 bit for bit (identical slices) -- the diagonal form.
template <bool NTK>
__device__ __forceinline__ void group_map(double (&k)[4][4], double (&q1)[4], double (&q2)[4], const ArchDev& arch,
                                          const double* __restrict__ tab, double (&t)[4][4]) {
    bool same[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            same[r][c] = (q1[r] == k[r][c]) && (q2[c] == k[r][c]);
            t[r][c] = 0.0;
        }
    for (int l = 0; l < arch.n_dense; ++l) {
        const double w2 = arch.w2[l], b2 = arch.b2[l];
        const bool hidden = l < arch.n_dense - 1;
        const int code = hidden ? arch.act[l] : NNGP_ACT_RELU;
        const bool erf = hidden && code == NNGP_ACT_ERF;
        const double* ap = arch.ap[hidden ? l : 0];
        double q1l[4], q2l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double a = q1[e], b = q2[e];
            q1[e] = fma(w2, a, b2);
            q2[e] = fma(w2, b, b2);
            q1l[e] = erf ? affine_lo(w2, a, b2, q1[e]) : 0.0;
            q2l[e] = erf ? affine_lo(w2, b, b2, q2[e]) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double kk = fma(w2, k[r][c], b2);
                double tt = NTK ? fma(w2, t[r][c], kk) : 0.0;
                if (hidden) {
                    double kd;
                    if (same[r][c]) act_diag(code, ap, kk, tab, kk, kd);
                    else if (erf) erf_cross_comp(ap, kk, affine_lo(w2, k[r][c], b2, kk), q1[r], q1l[r], q2[c], q2l[c], tab, kk, kd);
                    else act_cross(code, ap, kk, q1[r], q2[c], tab, kk, kd);
                    tt *= kd;
                }
                k[r][c] = kk;
                t[r][c] = tt;
            }
        if (hidden) {
            double unused;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                act_diag(code, ap, q1[e], tab, q1[e], unused);
                act_diag(code, ap, q2[e], tab, q2[e], unused);
            }
        }
    }
}

// NTK: the Theta outputs are wanted too (otherwise the NTK chain is dead code and its sums take no registers).
template <bool NTK>
__global__ __launch_bounds__(256) void k_build_add(AddArgs p, ArchDev arch, int64_t tiles_c, int vec_ok) {
    __shared__ __attribute__((aligned(16))) double smem[KT * LDP];  // As | Bs while the groups are walked, T for the mirror
    __shared__ __attribute__((aligned(16))) double tab[65 * 4];
    double* As = smem;               // [GKC][LDP]
    double* Bs = smem + GKC * LDP;   // [GKC][LDP]
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

    double sn[4][4], st[4][4], acc[4][4], qa[4], qb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        qa[r] = 0.0;
        qb[r] = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) sn[r][c] = st[r][c] = acc[r][c] = 0.0;
    }

    // The (group, k-chunk) steps form one flat sequence; the global loads of step s + 1 are issued into registers before step s
    // is consumed from LDS, so their latency hides behind the FMAs and the layer map of the group that has just ended.
    const int G = p.g.n_groups;
    double ra[2], rb[2];
    auto load_chunk = [&](int k0, int k_end) {  // 64 rows x GKC features per operand; features past the group's end are zero
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 256 * e;
            const int kk = idx & (GKC - 1), row = idx >> 3;
            const int kg = k0 + kk;
            const int64_t gi = i0 + row, gj = j0 + row;
            ra[e] = (kg < k_end && gi < i_end) ? a.x1[gi * a.d + kg] : 0.0;
            rb[e] = (kg < k_end && gj < j_end) ? a.x2[gj * a.d + kg] : 0.0;
        }
    };
    int g = 0, k0 = 0, k_begin = 0, k_end = 0;
    if (G > 0) {
        k_begin = p.g.begin[0];
        k_end = p.g.end[0];
        k0 = k_begin;
        load_chunk(k0, k_end);
    } else {
        __syncthreads();  // tab
    }
    while (g < G) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 256 * e;
            const int kk = idx & (GKC - 1), row = idx >> 3;
            As[kk * LDP + row] = ra[e];
            Bs[kk * LDP + row] = rb[e];
        }
        __syncthreads();
        // the step after this one
        int ng = g, nk0 = k0 + GKC, nk_begin = k_begin, nk_end = k_end;
        if (nk0 >= k_end) {
            ng = g + 1;
            if (ng < G) {
                nk_begin = p.g.begin[ng];
                nk_end = p.g.end[ng];
                nk0 = nk_begin;
            }
        }
        if (ng < G) load_chunk(nk0, nk_end);
        const int kn = (k_end - k0) < GKC ? (k_end - k0) : GKC;
        for (int kk = 0; kk < kn; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) av[r] = As[kk * LDP + ty + 16 * r];
            const double2 b01 = *reinterpret_cast<const double2*>(&Bs[kk * LDP + tx * 4]);
            const double2 b23 = *reinterpret_cast<const double2*>(&Bs[kk * LDP + tx * 4 + 2]);
            bv[0] = b01.x; bv[1] = b01.y; bv[2] = b23.x; bv[3] = b23.y;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                qa[r] = fma(av[r], av[r], qa[r]);
                qb[r] = fma(bv[r], bv[r], qb[r]);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(av[r], bv[c], acc[r][c]);
            }
        }
        __syncthreads();
        if (ng != g) {  // the group is complete: its term of every entry
            const double inv_dg = 1.0 / (double)(k_end - k_begin);
            const double wg = p.g.weight[g];
            double tv[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                qa[r] *= inv_dg;
                qb[r] *= inv_dg;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] *= inv_dg;
            }
            group_map<NTK>(acc, qa, qb, arch, tab, tv);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                qa[r] = qb[r] = 0.0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sn[r][c] = fma(wg, acc[r][c], sn[r][c]);
                    if (NTK) st[r][c] = fma(wg, tv[r][c], st[r][c]);
                    acc[r][c] = 0.0;
                }
            }
        }
        g = ng; k0 = nk0; k_begin = nk_begin; k_end = nk_end;
    }

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
