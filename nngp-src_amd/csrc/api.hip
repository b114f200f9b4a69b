// C-ABI entry points of libnngp_hip.so (include/nngp_hip.h) and the model object that owns the
// device buffers of one GP fit.  Mirrors the three nested reference interfaces of SURVEY.md 8b:
//   kernel_fn(x1, x2, get)                                  -> nngp_kernel_build
//   gradient_descent_mse_ensemble(kernel_fn, X, Y, diag_reg) -> nngp_model_create / _fit
//   predict_fn(x_test, get, compute_cov)                    -> nngp_model_predict  (api_predict.hip)
// The deferred CG solve for alpha -- nngp_model_solve, _set_alpha, _alpha -- is in alpha_solve.hip.
#include "model.h"

namespace nngp {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int make_arch_dev(const nngp_arch* arch, ArchDev* out) {
    NNGP_REQUIRE(arch != nullptr, "arch is NULL");
    NNGP_REQUIRE(arch->n_dense >= 1 && arch->n_dense <= NNGP_MAX_DENSE, "arch.n_dense must be in [1, %d] (got %d)",
                 NNGP_MAX_DENSE, arch->n_dense);
    out->n_dense = arch->n_dense;
    out->groups = nullptr;
    for (int l = 0; l < NNGP_MAX_DENSE; ++l) {
        out->w2[l] = l < arch->n_dense ? arch->w_std[l] * arch->w_std[l] : 0.0;
        out->b2[l] = l < arch->n_dense ? arch->b_std[l] * arch->b_std[l] : 0.0;
    }
    return 0;
}

// An ABRelu(a, b) with a == 0 and b == 1 is ReLU: it is given to the ReLU kernels, so that it computes the same bits.
int make_arch_dev_act(const nngp_arch_act* arch, ArchDev* out) {
    NNGP_REQUIRE(arch != nullptr, "arch is NULL");
    NNGP_TRY(make_arch_dev(&arch->base, out));
    constexpr double kPi = 3.14159265358979323846;
    out->general = 0;
    for (int l = 0; l < NNGP_MAX_DENSE - 1; ++l) {
        out->act[l] = NNGP_ACT_RELU;
        for (int e = 0; e < 4; ++e) out->ap[l][e] = 0.0;
    }
    for (int l = 0; l < arch->base.n_dense - 1; ++l) {
        const int code = arch->act[l];
        const double* p = arch->p[l];
        NNGP_REQUIRE(code == NNGP_ACT_RELU || code == NNGP_ACT_ABRELU || code == NNGP_ACT_ERF,
                     "arch_act: unknown activation code %d in hidden layer %d", code, l);
        if (code == NNGP_ACT_RELU) continue;
        const int np = code == NNGP_ACT_ERF ? 3 : 2;
        for (int e = 0; e < np; ++e)
            NNGP_REQUIRE(std::isfinite(p[e]), "arch_act: parameter %d of hidden layer %d is not finite", e, l);
        if (code == NNGP_ACT_ABRELU) {
            const double a = p[0], b = p[1];
            if (a == 0.0 && b == 1.0) continue;
            out->act[l] = NNGP_ACT_ABRELU;
            out->ap[l][0] = a * b;
            out->ap[l][1] = (b - a) * (b - a);
            out->ap[l][2] = 0.5 * (a * a + b * b);
        } else {
            const double a = p[0], b = p[1], c = p[2];
            out->act[l] = NNGP_ACT_ERF;
            out->ap[l][0] = a * a * (2.0 / kPi);
            out->ap[l][1] = 2.0 * b * b;
            out->ap[l][2] = c * c;
            out->ap[l][3] = out->ap[l][0] * out->ap[l][1];
        }
        out->general = 1;
    }
    return 0;
}

std::atomic<long long> g_alloc_count{0};
void note_alloc() { g_alloc_count.fetch_add(1, std::memory_order_relaxed); }


}  // namespace nngp

using namespace nngp;


namespace {

// out[0] = max(a), out[1] = sum(a)
__global__ __launch_bounds__(1024) void k_sum(const double* __restrict__ a, int64_t n, double* out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += a[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        out[1] = t;
    }
    __syncthreads();
    double mx = -1.0e300;
    for (int64_t i = threadIdx.x; i < n; i += 1024) mx = fmax(mx, a[i]);
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
        for (int w = 1; w < 16; ++w) t = fmax(t, red[w]);
        out[0] = t;
    }
}
}  // namespace

extern "C" {

int nngp_version(void) { return NNGP_ABI_VERSION; }

#ifdef NNGP_TIMING_KNOBS
int nngp_debug_set(int32_t key, int32_t value) {
    NNGP_REQUIRE(key >= 0 && key < 16, "debug_set: key out of range");
    g_knobs[key].store(value, std::memory_order_relaxed);
    return 0;
}
#endif

const char* nngp_last_error(void) { return g_err; }

static int kernel_diag(const double* x, int64_t n, int32_t d, const ArchDev& ad, double* diag_nngp, double* diag_ntk,
                       void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(x != nullptr && n >= 0 && d > 0, "kernel_diag: bad arguments");
    if (n == 0) return 0;
    double* q = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&q), sizeof(double) * n, s));
    int rc = launch_row_sqnorm(x, n, d, q, s);
    if (rc == 0) rc = launch_kernel_diag(x, q, n, d, ad, diag_nngp, diag_ntk, s);
    (void)hipFreeAsync(q, s);
    return rc;
}

int nngp_kernel_diag(const double* x, int64_t n, int32_t d, const nngp_arch* arch, double* diag_nngp,
                     double* diag_ntk, void* stream) {
    ArchDev ad{};
    NNGP_TRY(make_arch_dev(arch, &ad));
    return kernel_diag(x, n, d, ad, diag_nngp, diag_ntk, stream);
}

int nngp_kernel_diag_act(const double* x, int64_t n, int32_t d, const nngp_arch_act* arch, double* diag_nngp,
                         double* diag_ntk, void* stream) {
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    return kernel_diag(x, n, d, ad, diag_nngp, diag_ntk, stream);
}

static int kernel_build(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d, const ArchDev& ad,
                        int32_t out_dtype, void* out_nngp, void* out_ntk, int64_t ld, int64_t row_begin,
                        int64_t row_end, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const bool sym = (x2 == nullptr);
    if (sym) n2 = n1;
    NNGP_REQUIRE(n1 >= 0 && n2 >= 0 && d > 0, "kernel_build: bad n1/n2/d");
    if (n1 == 0 || n2 == 0) return 0;  // empty inputs: nothing to write
    NNGP_REQUIRE(x1 != nullptr, "kernel_build: x1 is NULL");
    NNGP_REQUIRE(n2 >= 0 && ld >= n2, "kernel_build: ld (%lld) < n2 (%lld)", (long long)ld, (long long)n2);
    NNGP_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= n1, "kernel_build: bad row range");
    NNGP_REQUIRE(out_dtype == NNGP_DTYPE_F32 || out_dtype == NNGP_DTYPE_F64, "kernel_build: bad out_dtype");
    NNGP_REQUIRE(out_nngp != nullptr || out_ntk != nullptr, "kernel_build: no output requested");
    if (n1 == 0 || n2 == 0 || row_begin == row_end) return 0;

    double *q1 = nullptr, *q2 = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&q1), sizeof(double) * n1, s));
    int rc = launch_row_sqnorm(x1, n1, d, q1, s);
    if (!sym && rc == 0) {
        if (hipMallocAsync(reinterpret_cast<void**>(&q2), sizeof(double) * n2, s) != hipSuccess) {
            set_error("kernel_build: hipMallocAsync failed");
            rc = -1;
        } else {
            rc = launch_row_sqnorm(x2, n2, d, q2, s);
        }
    }
    if (rc == 0) {
        BuildArgs a{};
        a.x1 = x1; a.x2 = sym ? x1 : x2; a.q1 = q1; a.q2 = sym ? q1 : q2;
        a.n1 = n1; a.n2 = n2; a.d = d;
        a.row_begin = row_begin; a.row_end = row_end;
        a.sym = (sym && row_begin == 0 && row_end == n1) ? 1 : 0;
        a.ld64 = a.ld32 = ld;
        if (out_dtype == NNGP_DTYPE_F64) {
            a.nngp64 = (double*)out_nngp; a.ntk64 = (double*)out_ntk;
        } else {
            a.nngp32 = (float*)out_nngp; a.ntk32 = (float*)out_ntk;
        }
        rc = launch_kernel_build(a, ad, s);
    }
    if (q1) (void)hipFreeAsync(q1, s);
    if (q2) (void)hipFreeAsync(q2, s);
    return rc;
}

int nngp_kernel_build(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d, const nngp_arch* arch,
                      int32_t out_dtype, void* out_nngp, void* out_ntk, int64_t ld, int64_t row_begin,
                      int64_t row_end, void* stream) {
    ArchDev ad{};
    NNGP_TRY(make_arch_dev(arch, &ad));
    return kernel_build(x1, n1, x2, n2, d, ad, out_dtype, out_nngp, out_ntk, ld, row_begin, row_end, stream);
}

int nngp_kernel_build_act(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d, const nngp_arch_act* arch,
                          int32_t out_dtype, void* out_nngp, void* out_ntk, int64_t ld, int64_t row_begin,
                          int64_t row_end, void* stream) {
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    return kernel_build(x1, n1, x2, n2, d, ad, out_dtype, out_nngp, out_ntk, ld, row_begin, row_end, stream);
}

static int model_create(nngp_model** out, int64_t n_cap, int64_t m_cap, int32_t d, int32_t ny, const ArchDev* arch,
                        int32_t get, double diag_reg, int32_t diag_reg_absolute_scale, const nngp_groups* groups = nullptr);

// ---- include/nngp_additive.h: the stand-alone calls make their own copy of the group table and wait for their work ----
int nngp_kernel_build_additive(const double* x1, int64_t n1, const double* x2, int64_t n2, int32_t d, const nngp_arch_act* arch,
                               const nngp_groups* groups, int32_t out_dtype, void* out_nngp, void* out_ntk, int64_t ld,
                               int64_t row_begin, int64_t row_end, void* stream) {
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    NNGP_REQUIRE(d > 0, "kernel_build: bad n1/n2/d");
    GroupsDev gd{};
    bool plain = false;
    NNGP_TRY(groups_create(groups, d, &gd, &plain));
    if (!plain) ad.groups = &gd;
    int rc = kernel_build(x1, n1, x2, n2, d, ad, out_dtype, out_nngp, out_ntk, ld, row_begin, row_end, stream);
    if (!plain) {
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == 0) {
            set_error("kernel_build_additive: the stream reported an error");
            rc = -1;
        }
        groups_destroy(&gd);
    }
    return rc;
}

int nngp_kernel_diag_additive(const double* x, int64_t n, int32_t d, const nngp_arch_act* arch, const nngp_groups* groups,
                              double* diag_nngp, double* diag_ntk, void* stream) {
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    NNGP_REQUIRE(d > 0, "kernel_diag: bad arguments");
    GroupsDev gd{};
    bool plain = false;
    NNGP_TRY(groups_create(groups, d, &gd, &plain));
    if (!plain) ad.groups = &gd;
    int rc = kernel_diag(x, n, d, ad, diag_nngp, diag_ntk, stream);
    if (!plain) {
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == 0) {
            set_error("kernel_diag_additive: the stream reported an error");
            rc = -1;
        }
        groups_destroy(&gd);
    }
    return rc;
}

int nngp_model_create_additive(nngp_model** out, int64_t n_cap, int64_t m_cap, int32_t d, int32_t ny, const nngp_arch_act* arch,
                               const nngp_groups* groups, int32_t get, double diag_reg, int32_t diag_reg_absolute_scale) {
    NNGP_REQUIRE(out != nullptr, "model_create: out is NULL");
    *out = nullptr;
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    NNGP_REQUIRE(groups != nullptr, "groups: the group table is NULL");
    return model_create(out, n_cap, m_cap, d, ny, &ad, get, diag_reg, diag_reg_absolute_scale, groups);
}

int nngp_model_create(nngp_model** out, int64_t n_cap, int64_t m_cap, int32_t d, int32_t ny, const nngp_arch* arch,
                      int32_t get, double diag_reg, int32_t diag_reg_absolute_scale) {
    NNGP_REQUIRE(out != nullptr, "model_create: out is NULL");
    *out = nullptr;
    ArchDev ad{};
    NNGP_TRY(make_arch_dev(arch, &ad));
    return model_create(out, n_cap, m_cap, d, ny, &ad, get, diag_reg, diag_reg_absolute_scale);
}

int nngp_model_create_act(nngp_model** out, int64_t n_cap, int64_t m_cap, int32_t d, int32_t ny, const nngp_arch_act* arch,
                          int32_t get, double diag_reg, int32_t diag_reg_absolute_scale) {
    NNGP_REQUIRE(out != nullptr, "model_create: out is NULL");
    *out = nullptr;
    ArchDev ad{};
    NNGP_TRY(make_arch_dev_act(arch, &ad));
    return model_create(out, n_cap, m_cap, d, ny, &ad, get, diag_reg, diag_reg_absolute_scale);
}

static int model_create(nngp_model** out, int64_t n_cap, int64_t m_cap, int32_t d, int32_t ny, const ArchDev* arch,
                        int32_t get, double diag_reg, int32_t diag_reg_absolute_scale, const nngp_groups* groups) {
    NNGP_REQUIRE(n_cap > 0 && d > 0 && ny > 0 && m_cap >= 0, "model_create: bad sizes");
    NNGP_REQUIRE(get == NNGP_GET_NNGP || get == NNGP_GET_NTK, "model_create: get must be NNGP_GET_NNGP or NNGP_GET_NTK");
    NNGP_REQUIRE(diag_reg >= 0.0, "model_create: diag_reg must be >= 0");
    nngp_model* m = new (std::nothrow) nngp_model();
    NNGP_REQUIRE(m != nullptr, "model_create: out of host memory");
    int rc = 0;
    m->arch = *arch;
    if (groups != nullptr) {  // the model's own copy of the group table (include/nngp_additive.h)
        bool plain = false;
        rc = groups_create(groups, d, &m->groups, &plain);
        if (rc != 0) {
            delete m;
            return rc;
        }
        if (!plain) m->arch.groups = &m->groups;
    }
    m->n_cap = n_cap; m->np_cap = round_up(n_cap, TB); m->m_cap = 0;
    m->ld = m->np_cap;
    m->d = d; m->ny = ny; m->get = get; m->diag_reg = diag_reg; m->absolute = diag_reg_absolute_scale;
    const int64_t np = m->np_cap;
    auto A = [&](int r) { if (rc == 0) rc = r; };
    A(dev_alloc(&m->x, n_cap * d)); A(dev_alloc(&m->y, n_cap * ny)); A(dev_alloc(&m->q, n_cap));
    A(dev_alloc(&m->kdiag, n_cap)); A(dev_alloc(&m->k64, np * np)); A(dev_alloc(&m->a32, np * np));
    A(dev_alloc(&m->dinv, (np / TB) * TB * TB)); A(dev_alloc(&m->clamped, 1)); A(dev_alloc(&m->alpha, n_cap * ny));
    A(dev_alloc(&m->pcg.r, np)); A(dev_alloc(&m->pcg.z, np)); A(dev_alloc(&m->pcg.p, np)); A(dev_alloc(&m->pcg.q, np));
    A(dev_alloc(&m->pcg.xcol, np)); A(dev_alloc(&m->pcg.bcol, np));
    A(dev_alloc(&m->pcg.f32a, np)); A(dev_alloc(&m->pcg.f32b, np)); A(dev_alloc(&m->pcg.f32c, np));
    A(dev_alloc(&m->pcg.scal, 32));
    A(dev_alloc(&m->pcg.symv_part, (np / TB) * np));
    A(dev_alloc(&m->pcg.dot_part, 32));
    A(dev_alloc(&m->pcg.dot_ctr, 1));
    if (rc == 0 && hipMemset(m->pcg.dot_ctr, 0, sizeof(unsigned)) != hipSuccess) rc = -1;
    m->pcg.symv_np = np;
    {
        const int64_t bs_cap = triinv_block(np);
        const int64_t nblk = (np + bs_cap - 1) / bs_cap;
        A(dev_alloc(&m->tri.tinv, nblk * bs_cap * bs_cap)); A(dev_alloc(&m->tri.xinv, nblk * bs_cap * bs_cap));
        A(dev_alloc(&m->tri.partial, (bs_cap / TB) * np)); A(dev_alloc(&m->tri.tmp, bs_cap));
    }
    if (rc == 0 && hipHostMalloc(reinterpret_cast<void**>(&m->pcg.host_scal), sizeof(double) * 32) != hipSuccess) {
        set_error("model_create: hipHostMalloc failed");
        rc = -1;
    }
    if (rc == 0) rc = lookahead_create(&m->la);
    int prio_least = 0, prio_greatest = 0;  // the solve's many small kernels must not queue behind the covariance GEMMs
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_least = prio_greatest = 0;
    if (rc == 0 && (hipStreamCreateWithPriority(&m->solve_stream, hipStreamNonBlocking, prio_greatest) != hipSuccess ||
                    hipEventCreateWithFlags(&m->alpha_solve.ev_ready, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&m->ev_lt, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&m->alpha_solve.ev_solved, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&m->alpha_solve.ev_predict, hipEventDisableTiming) != hipSuccess)) {
        set_error("model_create: could not create the solve stream");
        rc = -1;
    }
    if (rc == 0 && np >= 4 * kLookAheadNb) {  // the look-ahead factorisation keeps a float16-split copy of one block column
        // ... and keeps the copies of all block columns: the posterior's blocked triangular solves read them again
        m->split.rows_cap = np + 256;
        m->split.k_cap = kLookAheadNb;
        m->split.col_stride = m->split.rows_cap * m->split.k_cap * 4;
        const int64_t ncols = (np + kLookAheadNb - 1) / kLookAheadNb;
        rc = dev_alloc(&m->split.planes, ncols * m->split.col_stride);
        if (rc == 0) rc = dev_alloc(&m->split.counters, 16);
        if (rc == 0 && hipMemset(m->split.counters, 0, 16 * sizeof(int)) != hipSuccess) rc = -1;
        // the transposed split copy (operand of the posterior's "B L^-1" solves): the factorisation's panel solves write it as they go
        if (rc == 0 && !soft_alloc(&m->split.planes_t, ncols * m->split.col_stride)) m->split.planes_t = nullptr;  // (no room: built lazily, or float32 path)
        if (rc == 0) rc = dev_alloc(&m->split.ldiag, 2 * kLookAheadNb * kLookAheadNb * 4);
        if (rc == 0) rc = dev_alloc(&m->split.dfrag, 2 * kLookAheadNb * 128);
        if (rc == 0) rc = dev_alloc(&m->split.dscale, 2 * kLookAheadNb);
    }
    if (rc == 0 && m_cap > 0) rc = ensure_predict_capacity(m, m_cap, true);
    if (rc != 0) {
        delete m;
        return rc;
    }
    *out = m;
    return 0;
}

int64_t nngp_alloc_count(void) { return (int64_t)g_alloc_count.load(std::memory_order_relaxed); }

// Everything a predict of up to `rows` test rows with this covariance mode allocates lazily otherwise (workspace is
// allocated ahead, never inside the timed launch functions): cross-kernel / right-hand-side buffers, the persistent solves'
// workspace, the refinement rows, the int8 path's digit planes and products, the float32 path's L^T, the full-covariance blocks.
int nngp_model_reserve(nngp_model* m, int64_t rows, int32_t cov_mode) {
    NNGP_REQUIRE(m != nullptr && rows > 0 && cov_mode >= NNGP_COV_NONE && cov_mode <= NNGP_COV_FULL, "reserve: bad arguments");
    NNGP_TRY(ensure_predict_capacity(m, rows, true));
    if (cov_mode == NNGP_COV_NONE) return 0;
    const int64_t mp = round_up(rows, TB);
    if (m->var_refine >= 1 || m->get == NNGP_GET_NTK) NNGP_TRY(ensure_refine_capacity(m, mp));
    const bool split_path = m->split.planes != nullptr && mp <= m->split.mb_cap && mp >= 256 && mp * m->np_cap >= 7000000;
    if (!split_path) NNGP_TRY(ensure_lt_alloc(m));
    NNGP_TRY(i8s_reserve(m, mp, cov_mode));
    if (cov_mode == NNGP_COV_FULL) NNGP_TRY(ensure_full_cov_capacity(m, rows));
    return 0;
}

int nngp_model_destroy(nngp_model* m) {
    if (m) {
        (void)hipDeviceSynchronize();
        delete m;
    }
    return 0;
}

int nngp_model_set_train(nngp_model* m, const double* x, const double* y, int64_t n, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && x != nullptr && y != nullptr, "set_train: NULL argument");
    NNGP_REQUIRE(n > 0 && n <= m->n_cap, "set_train: n=%lld outside (0, n_cap=%lld]", (long long)n, (long long)m->n_cap);
    m->alpha_solve.plan.invalidate();
    m->n = n;
    m->np = round_up(n, TB);
    m->built = m->factored = false;
    m->serving_ready = false;
    NNGP_HIP_CHECK(hipMemcpyAsync(m->x, x, sizeof(double) * n * m->d, hipMemcpyDeviceToDevice, s));
    NNGP_HIP_CHECK(hipMemcpyAsync(m->y, y, sizeof(double) * n * m->ny, hipMemcpyDeviceToDevice, s));
    NNGP_TRY(launch_row_sqnorm(m->x, n, m->d, m->q, s));
    NNGP_TRY(launch_kernel_diag(m->x, m->q, n, m->d, m->arch, m->get == NNGP_GET_NNGP ? m->kdiag : nullptr,
                                m->get == NNGP_GET_NTK ? m->kdiag : nullptr, s));
    hipLaunchKernelGGL(k_sum, dim3(1), dim3(1024), 0, s, m->kdiag, n, m->pcg.scal + 6);  // [6] = max, [7] = sum
    NNGP_HIP_CHECK(hipMemcpyAsync(m->pcg.host_scal + 6, m->pcg.scal + 6, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    m->trace_mean = m->pcg.host_scal[7] / (double)n;
    m->diag_max = m->pcg.host_scal[6];
    m->reg = m->absolute ? m->diag_reg : m->diag_reg * m->trace_mean;
    m->reg_fac = m->reg;
    set_split_scale(m);
    m->have_train = true;
    return 0;
}

int nngp_model_build_rows(nngp_model* m, int64_t row_begin, int64_t row_end, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->have_train, "build_rows: call set_train first");
    NNGP_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= m->n, "build_rows: bad row range");
    m->alpha_solve.plan.invalidate();
    BuildArgs a{};
    a.x1 = m->x; a.x2 = m->x; a.q1 = m->q; a.q2 = m->q;
    a.n1 = m->n; a.n2 = m->n; a.d = m->d;
    a.row_begin = row_begin; a.row_end = row_end;
    a.sym = (row_begin == 0 && row_end == m->n) ? 1 : 0;
    a.ld64 = a.ld32 = m->ld;
    if (m->get == NNGP_GET_NNGP) a.nngp64 = m->k64; else a.ntk64 = m->k64;
    m->a32_built = false;
    m->a32_complete = false;
    m->k64_partial = false;
    m->k64_symmetric = a.sym != 0;
    i8s_kernel_changed(m);
    if (a.sym) {  // whole matrix in one build: the float32 factorisation input falls out of the same epilogue
        if (m->get == NNGP_GET_NNGP) { a.nngp32 = m->a32; a.diag_add_nngp32 = m->reg; }
        else { a.ntk32 = m->a32; a.diag_add_ntk32 = m->reg; }
        a.lower32 = 1;
        m->a32_built = true;
    }
    // An NTK model whose covariance has been asked for before keeps the NNGP kernel of its training rows beside Theta (kaux64, the
    // K_dd of cov = K_tt + Z K_dd Z^T - ...): the layer recursion carries both kernels anyway, so the same launch writes it -- one
    // kernel build per fit instead of two (the second one used to run inside the first covariance predict).  Same leading dimension only.
    m->aux_ready = false;
    const bool aux_too = a.sym && m->get == NNGP_GET_NTK && m->kaux64 != nullptr && m->ld == m->np && NNGP_KNOB(5) != 65;
    if (aux_too) a.nngp64 = m->kaux64;
    NNGP_TRY(launch_kernel_build(a, m->arch, s));
    if (aux_too) {
        NNGP_TRY(launch_zero_pad_f64(m->kaux64, m->np, m->n, m->np, s));
        m->aux_ready = true;
        m->i8.work.aux.ready = false;
    }
    NNGP_TRY(launch_zero_pad_f64(m->k64, m->ld, m->n, m->np, s));  // float64 GEMMs read the padded matrix
    m->built = true;  // the caller vouches for the remaining rows (all-gather) before factor
    m->factored = false;
    return 0;
}

int nngp_model_factor_begin(nngp_model* m, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->built, "factor: build the kernel rows first");
    m->alpha_solve.plan.invalidate();
    // a32 = float32(K) + reg I on the lower tiles; if the build already wrote it, only the last (partial + padding)
    // block row is left
    NNGP_TRY(launch_factor_input(m->k64, m->ld, m->a32, m->ld, m->n, m->np, m->reg_fac, m->reg_fac + m->trace_mean, s,
                                 m->a32_complete ? m->n : m->a32_built ? (m->n / TB) * TB : 0));  // (rows >= n: padding only, no read of k64)
    m->a32_built = false;  // the factorisation overwrites a32
    m->a32_complete = false;
    NNGP_HIP_CHECK(hipMemsetAsync(m->clamped, 0, sizeof(int32_t), s));
    m->tri.bs = triinv_block(m->np);
    m->factored = false;
    m->serving_ready = false;
    m->split.l_ready = m->split.lt_ready = false;  // set again by the look-ahead factorisation / factor_end
    m->split.split_panel = -1;
    return 0;
}

int nngp_model_factor_panel(nngp_model* m, int64_t col0, int64_t width, void* stream) {
    NNGP_REQUIRE(m != nullptr && m->built, "factor_panel: build the kernel rows first");
    // Exact-arithmetic pivots of K + reg I are >= reg; anything far below is float32 rounding noise.
    return potrf_panel_f32(m->a32, m->np, m->ld, m->dinv, m->clamped, (float)(0.25 * m->reg_fac), col0, width,
                           (hipStream_t)stream, &m->split);
}

int nngp_model_factor_update(nngp_model* m, int64_t panel_col0, int64_t panel_width, int64_t col0, int64_t width,
                             void* stream) {
    NNGP_REQUIRE(m != nullptr && m->built, "factor_update: build the kernel rows first");
    return potrf_update_f32(m->a32, m->np, m->ld, panel_col0, panel_width, col0, width, (hipStream_t)stream, &m->split);
}

int nngp_model_factor_update_cols(nngp_model* m, int64_t panel_col0, int64_t panel_width, const int64_t* cols, int32_t ncols,
                                  int64_t width, void* stream) {
    NNGP_REQUIRE(m != nullptr && m->built, "factor_update_cols: build the kernel rows first");
    NNGP_REQUIRE(ncols >= 0 && (ncols == 0 || cols != nullptr), "factor_update_cols: bad column list");
    return potrf_update_cols_f32(m->a32, m->np, m->ld, panel_col0, panel_width, cols, ncols, width, (hipStream_t)stream, &m->split);
}

int nngp_model_factor_input_rows(nngp_model* m, int64_t row_begin, int64_t row_end, double shift_scale, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->built, "factor_input_rows: build the kernel rows first");
    NNGP_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= m->n && shift_scale >= 1.0, "factor_input_rows: bad row range or shift");
    m->alpha_solve.plan.drop();
    m->reg_fac = m->reg * shift_scale;
    m->k64_partial = true;
    return launch_factor_input(m->k64, m->ld, m->a32, m->ld, m->n, m->np, m->reg_fac, m->reg_fac + m->trace_mean, s, row_begin, row_end);
}

int nngp_model_factor_input_complete(nngp_model* m) {
    NNGP_REQUIRE(m != nullptr && m->built, "factor_input_complete: build the kernel rows first");
    NNGP_REQUIRE(m->k64_partial, "factor_input_complete: no rows of the factor input were converted (nngp_model_factor_input_rows) since the last build");
    m->a32_complete = true;
    return 0;
}

int nngp_model_precond(nngp_model* m, const double* r, double* z, void* stream) {
    NNGP_REQUIRE(m != nullptr && m->factored, "precond: factor first");
    NNGP_REQUIRE(r != nullptr && z != nullptr, "precond: NULL argument");
    NNGP_TRY(tri_join(m, (hipStream_t)stream));
    return precond_apply(m->a32, m->ld, m->tri, m->n, m->np, r, z, m->pcg, (hipStream_t)stream);
}

int nngp_model_matvec_rows(nngp_model* m, const double* p, double* q, int64_t row_begin, int64_t row_end, void* stream) {
    NNGP_REQUIRE(m != nullptr && m->built, "matvec_rows: build the kernel rows first");
    NNGP_REQUIRE(p != nullptr && q != nullptr && 0 <= row_begin && row_begin <= row_end && row_end <= m->n, "matvec_rows: bad arguments");
    return launch_gemv_f64(m->k64 + row_begin * m->ld, m->ld, row_end - row_begin, m->n, p, 1, q, 1, 0.0, (hipStream_t)stream);
}

int nngp_model_factor_end(nngp_model* m, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->built, "factor_end: build the kernel rows first");
    m->tri.bs = triinv_block(m->np);
    m->tri_stale = true;  // built by the first reader (tri_join), or by a predict beside its cross-kernel build (tri_fork)
    m->tri_pending = false;
    // the float16-split copy of L by block column, if the factorisation did not leave one behind (recursion at
    // 4096 <= N, block-column ABI of the distributed factorisation): the posterior's solves use it
    if (!m->split.l_ready && m->split.planes != nullptr && m->np >= 4 * m->split.k_cap && m->tri.bs % m->split.k_cap == 0 &&
        m->split.rows_cap >= m->np + 256) {
        const int64_t bs = m->split.k_cap, ldp = 4 * bs;
        for (int64_t j = 0, o = 0; o + bs < m->np; ++j, o += bs)
            NNGP_TRY(launch_split_rows(m->a32 + (o + bs) * m->ld + o, m->ld, m->np - o - bs, bs, m->split.scale,
                                       m->split.planes + j * m->split.col_stride + (o + bs) * ldp, ldp, s));
        m->split.l_ready = true;
    }
    m->factored = true;
    // (neutral beside the plain "not solved" this was: factor_begin has dropped the solve, and nngp_model_solve is refused between
    // the two because `factored` is false)
    m->alpha_solve.plan.invalidate();
    m->lt_ready = false;
    return 0;  // (aux_ready follows the kernel, not the factor: nngp_model_build_rows / nngp_model_append reset it)
}

int nngp_model_factor_buffers(nngp_model* m, float** a32, int64_t* ld, float** dinv) {
    NNGP_REQUIRE(m != nullptr && m->have_train, "factor_buffers: call set_train first");
    if (a32) *a32 = m->a32;
    if (ld) *ld = m->ld;
    if (dinv) *dinv = m->dinv;
    return 0;
}

// Exact-arithmetic pivots of K + reg I are >= reg; the leaf clamps anything below reg / 4 (float32 rounding noise) and
// counts it.  A count > 0 means the float32 factorisation broke down -- cond(K + reg I) * eps32 >> 1: tiny diag_reg,
// low-dimensional encodings -- and what it left is useless as a preconditioner (entries blow up after a clamped pivot,
// the float16 split overflows: NaN in the first CG step).  The factor is then rebuilt from the float64 kernel with a
// 16x larger diagonal shift, up to four times.  K + reg_fac I preconditions K + reg I with eigenvalues in
// [reg / reg_fac, 1]: more CG iterations (~ sqrt of the ratio), same answers.  One 4-byte read-back per factorisation.
int nngp_model_factor(nngp_model* m, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->built, "factor: build the kernel rows first");
    if (!m->k64_partial) m->reg_fac = m->reg;  // (row-sharded layout: nngp_model_factor_input_rows chose the shift)
    set_split_scale(m);
    for (int attempt = 0;; ++attempt) {
        NNGP_TRY(nngp_model_factor_begin(m, stream));
        NNGP_TRY(potrf_lookahead_f32(m->a32, m->np, m->ld, m->dinv, m->clamped, (float)(0.25 * m->reg_fac), m->la, &m->split, s, &m->tri));
        int32_t cl = 0;
        NNGP_HIP_CHECK(hipMemcpyAsync(&cl, m->clamped, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        NNGP_HIP_CHECK(hipStreamSynchronize(s));
        if (cl == 0 || attempt == 4 || NNGP_KNOB(6) == 1 || m->k64_partial) break;  // (row-sharded layout: the caller redoes the exchange with a larger shift)
        m->reg_fac *= 16.0;
        set_split_scale(m);
    }
    return nngp_model_factor_end(m, stream);
}

double nngp_model_factor_shift(nngp_model* m) { return m != nullptr ? m->reg_fac : 0.0; }

// Appends b training rows to a fitted model without refactoring what is already there (the
// reference's active-learning loop refits from scratch, ActiveLearner.py:43-77).  With r0 = the last 128-aligned row
// count of the old fit:  kernel rows [n, n+b) are built against all rows and mirrored into the old rows' columns;
//   L10 = A[r0:, :r0] L00^-T  (blocked triangular solve with the old factor's inverted 1024-blocks),
//   L11 = chol(A[r0:, r0:] - L10 L10^T)  (SYRK + blocked Cholesky of the small trailing block).
// The relative regulariser changes with the trace, so L00 is the factor of the OLD A00 -- it is only the CG
// preconditioner; alpha and the refined covariances are computed against the float64 kernel with the new reg.
// Call nngp_model_solve afterwards.  Cost ~ b N^2 instead of N^3 / 3.
int nngp_model_append(nngp_model* m, const double* x_new, const double* y_new, int64_t b, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    NNGP_REQUIRE(m != nullptr && m->factored, "append: fit the model first");
    NNGP_REQUIRE(!m->k64_partial, "append: not with the row-sharded layout (the model holds only its own kernel rows)");
    NNGP_REQUIRE(x_new != nullptr && y_new != nullptr && b > 0, "append: bad arguments");
    NNGP_REQUIRE(m->n + b <= m->n_cap, "append: %lld + %lld rows exceed n_cap = %lld", (long long)m->n, (long long)b,
                 (long long)m->n_cap);
    const int64_t n0 = m->n, n1 = n0 + b, np0 = m->np, np1 = round_up(n1, TB), r0 = (n0 / TB) * TB, rows = np1 - r0;
    NNGP_REQUIRE(r0 > 0, "append: the fitted model must have at least 128 rows");
    m->alpha_solve.plan.invalidate();
    NNGP_TRY(ensure_predict_capacity(m, rows, false));  // b32 / trsm_tmp workspace of the blocked solve
    // 1. data, diagonal, regulariser
    NNGP_HIP_CHECK(hipMemcpyAsync(m->x + n0 * m->d, x_new, sizeof(double) * b * m->d, hipMemcpyDeviceToDevice, s));
    NNGP_HIP_CHECK(hipMemcpyAsync(m->y + n0 * m->ny, y_new, sizeof(double) * b * m->ny, hipMemcpyDeviceToDevice, s));
    NNGP_TRY(launch_row_sqnorm(m->x + n0 * m->d, b, m->d, m->q + n0, s));
    NNGP_TRY(launch_kernel_diag(m->x + n0 * m->d, m->q + n0, b, m->d, m->arch, m->get == NNGP_GET_NNGP ? m->kdiag + n0 : nullptr,
                                m->get == NNGP_GET_NTK ? m->kdiag + n0 : nullptr, s));
    hipLaunchKernelGGL(k_sum, dim3(1), dim3(1024), 0, s, m->kdiag, n1, m->pcg.scal + 6);
    NNGP_HIP_CHECK(hipMemcpyAsync(m->pcg.host_scal + 6, m->pcg.scal + 6, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    m->trace_mean = m->pcg.host_scal[7] / (double)n1;
    m->diag_max = m->pcg.host_scal[6];
    const double shift_ratio = (m->reg > 0.0 && m->reg_fac > m->reg) ? m->reg_fac / m->reg : 1.0;
    m->reg = m->absolute ? m->diag_reg : m->diag_reg * m->trace_mean;
    m->reg_fac = m->reg * shift_ratio;  // a fit that needed a larger shift in its factor keeps the ratio
    const float old_scale = m->split.scale;
    set_split_scale(m);
    m->n = n1;
    m->np = np1;
    m->serving_ready = false;
    i8s_kernel_changed(m);
    // 2. kernel rows [n0, n1) against all n1 rows, their mirror image, and the new padding
    BuildArgs a{};
    a.x1 = m->x; a.x2 = m->x; a.q1 = m->q; a.q2 = m->q;
    a.n1 = n1; a.n2 = n1; a.d = m->d;
    a.row_begin = n0; a.row_end = n1; a.sym = 0;
    a.ld64 = a.ld32 = m->ld;
    if (m->get == NNGP_GET_NNGP) a.nngp64 = m->k64; else a.ntk64 = m->k64;
    m->k64_symmetric = false;  // the appended rows' own block is built entry by entry
    NNGP_TRY(launch_kernel_build(a, m->arch, s));
    NNGP_TRY(launch_mirror_rows_f64(m->k64, m->ld, n0, n1, s));
    NNGP_TRY(launch_zero_pad_f64(m->k64, m->ld, n1, np1, s));
    // 3. factor rows [r0, np1)
    NNGP_TRY(launch_factor_input(m->k64, m->ld, m->a32, m->ld, n1, np1, m->reg_fac, m->reg_fac + m->trace_mean, s, r0));
    float* a10 = m->a32 + r0 * m->ld;
    NNGP_TRY(tri_join(m, s));
    NNGP_TRY(trsm_rlt_blocks_f32(a10, m->ld, rows, m->a32, m->ld, m->tri, r0, m->trsm_tmp, s));
    NNGP_TRY(launch_gemm_nt_f32(a10 + r0, m->ld, a10, m->ld, a10, m->ld, rows, rows, r0, -1.0f, 1.0f, true, s));
    NNGP_TRY(potrf_f32(a10 + r0, rows, m->ld, m->dinv + (r0 / TB) * TB * TB, m->clamped, (float)(0.25 * m->reg_fac), s));
    m->tri.bs = triinv_block(m->np);
    m->tri_stale = true;
    m->tri_pending = false;
    NNGP_TRY(tri_join(m, s));  // in order: the old blocks were read just above
    // 4. float16-split copies: rows >= r0 of every block column (same scale as the rest), L^T copies rebuilt lazily
    if (m->split.l_ready && m->split.scale == old_scale && m->split.rows_cap >= np1 + 256) {
        const int64_t bs = m->split.k_cap, ldp = 4 * bs;
        for (int64_t j = 0, o = 0; o + bs < np1; ++j, o += bs) {
            const int64_t first = (o + bs > r0) ? o + bs : r0;  // rows below the diagonal block, from r0 on
            NNGP_TRY(launch_split_rows(m->a32 + first * m->ld + o, m->ld, np1 - first, bs, m->split.scale,
                                       m->split.planes + j * m->split.col_stride + first * ldp, ldp, s));
        }
    } else {
        m->split.l_ready = false;
    }
    m->split.lt_ready = false;
    m->lt_ready = false;
    m->aux_ready = false;
    (void)np0;
    return 0;
}

int nngp_model_fit(nngp_model* m, const double* x, const double* y, int64_t n, void* stream) {
    NNGP_TRY(nngp_model_set_train(m, x, y, n, stream));
    NNGP_TRY(nngp_model_build_rows(m, 0, n, stream));
    NNGP_TRY(nngp_model_factor(m, stream));
    return nngp_model_solve(m, 0, 0.0, stream);
}

int nngp_model_kernel_buffer(nngp_model* m, double** k64, int64_t* ld) {
    NNGP_REQUIRE(m != nullptr && m->have_train, "kernel_buffer: call set_train first");
    if (k64) *k64 = m->k64;
    if (ld) *ld = m->ld;
    return 0;
}

int nngp_model_update_timer(nngp_model* m, int32_t enable) {
    NNGP_REQUIRE(m != nullptr, "update_timer: NULL model");
    NNGP_REQUIRE(m->la != nullptr, "update_timer: this model has no look-ahead factorisation (too small)");
    m->la->time_updates = enable != 0;
    m->la->tu_count = 0;
    return 0;
}

int nngp_model_update_timer_read(nngp_model* m, int64_t* launches, double* ms_total, double* flops_total) {
    NNGP_REQUIRE(m != nullptr && m->la != nullptr, "update_timer_read: no timer on this model");
    double ms = 0.0, fl = 0.0;
    for (int t = 0; t < m->la->tu_count; ++t) {
        NNGP_HIP_CHECK(hipEventSynchronize(m->la->tu1[t]));
        float e = 0.0f;
        NNGP_HIP_CHECK(hipEventElapsedTime(&e, m->la->tu0[t], m->la->tu1[t]));
        ms += e;
        fl += m->la->tu_flops[t];
    }
    if (launches) *launches = m->la->tu_count;
    if (ms_total) *ms_total = ms;
    if (flops_total) *flops_total = fl;
    return 0;
}

int nngp_model_residual_timer(nngp_model* m, int32_t enable) {
    NNGP_REQUIRE(m != nullptr, "residual_timer: NULL model");
    return i8s_timer_enable(m, enable);
}

int nngp_model_residual_timer_read(nngp_model* m, int64_t* launches, double* ms_total, double* flops_total, double* int8_ops_total) {
    NNGP_REQUIRE(m != nullptr, "residual_timer_read: NULL model");
    return i8s_timer_read(m, launches, ms_total, flops_total, int8_ops_total);
}

int nngp_model_trsm_timer(nngp_model* m, int32_t enable) {
    NNGP_REQUIRE(m != nullptr, "trsm_timer: NULL model");
    m->trsm_t.enable(enable != 0);
    return 0;
}

int nngp_model_trsm_timer_read(nngp_model* m, int64_t* solves, double* ms_total, double* flops_total) {
    NNGP_REQUIRE(m != nullptr, "trsm_timer_read: NULL model");
    auto& w = m->trsm_t;
    double ms = 0.0, fl = 0.0;
    NNGP_TRY(w.read(&ms));
    for (int t = 0; t < w.count; ++t) fl += m->trsm_flops[t];
    if (solves) *solves = w.count;
    if (ms_total) *ms_total = ms;
    if (flops_total) *flops_total = fl;
    w.count = 0;
    return 0;
}

int nngp_model_residual_floor(nngp_model* m, double* ratio, int32_t* distrusted) {
    NNGP_REQUIRE(m != nullptr, "residual_floor: NULL model");
    return i8s_residual_floor(m, ratio, distrusted);
}

int nngp_model_update_timer_bytes(nngp_model* m, double* bytes_total) {
    NNGP_REQUIRE(m != nullptr && m->la != nullptr && bytes_total != nullptr, "update_timer_bytes: no timer on this model");
    double b = 0.0;
    for (int t = 0; t < m->la->tu_count; ++t) b += m->la->tu_bytes[t];
    *bytes_total = b;
    return 0;
}

int nngp_model_info(nngp_model* m, nngp_fit_info* info) {
    NNGP_REQUIRE(m != nullptr && info != nullptr, "model_info: NULL argument");
    NNGP_TRY(tickets_check(m, true));
    NNGP_TRY(run_pending_solve(m, nullptr, false));
    int32_t cl = 0;
    if (m->factored) NNGP_HIP_CHECK(hipMemcpy(&cl, m->clamped, sizeof(int32_t), hipMemcpyDeviceToHost));
    info->reg = m->reg;
    info->trace_mean = m->trace_mean;
    info->rel_residual = m->alpha_solve.plan.relres;
    info->refine_iters = m->alpha_solve.plan.iters;
    info->clamped_pivots = cl;
    info->n = m->n;
    info->n_padded = m->np;
    return 0;
}

int nngp_model_cov_iters(nngp_model* m) {
    NNGP_REQUIRE(m != nullptr, "cov_iters: NULL model");
    return m->cov_iters;
}

int nngp_model_sweep_estimate(nngp_model* m, double* row_rel, double* var_rel) {
    NNGP_REQUIRE(m != nullptr, "sweep_estimate: NULL model");
    if (row_rel) *row_rel = m->sweep_est;
    if (var_rel) *var_rel = m->sweep_est_var;
    return 0;
}

int nngp_model_set_refine(nngp_model* m, int32_t sweeps) {
    NNGP_REQUIRE(m != nullptr && sweeps >= 0 && sweeps <= 8, "set_refine: level must be in [0, 8]");
    m->var_refine = sweeps;
    return 0;
}

}  // extern "C"
