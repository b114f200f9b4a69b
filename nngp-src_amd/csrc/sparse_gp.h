// Shared between the sparse NNGP posterior (sparse_gp.hip) and its evidence (sparse_evidence.hip): the handle of
// include/nngp_sparse.h and the two steps the evidence passes borrow from the fit.
#pragma once
#include "gp_f64.h"

#include <initializer_list>
#include <utility>
#include <vector>

// slots of nngp_sparse::scal.  [0, 4) are the fit's own; the rest belongs to the evidence (include/nngp_sparse_evidence.h)
constexpr int kSpYY = 4;           // y^T y of the rows added
constexpr int kSpQ = 8;            // [NNGP_MAX_DENSE] sum_i q_i^(l) of the rows added: tr dK_ff / dtheta in closed form
constexpr int kSpSums = 24;        // sum log (L_B)_ii, |C|^2, tr G, |gamma|^2, beta^T beta, tr B^-1
constexpr int kSpQu = 32;          // [NNGP_MAX_DENSE] the same sums over the inducing rows
constexpr int kSpAccFu = 48;       // [4 n_dense] the rectangular pass: per component the beta gamma^T half, then the matrix half
constexpr int kSpAccUu = 48 + 4 * NNGP_MAX_DENSE;  // [4 n_dense] the symmetric pass over K_uu
constexpr int kSpScal = kSpAccUu + 4 * NNGP_MAX_DENSE;

struct nngp_sparse {
    int64_t m_cap = 0, mp_cap = 0, chunk_rows = 0, test_cap = 0;
    int d = 0, ny = 1;
    nngp::ArchDev arch{};
    nngp::GroupsDev groups{};
    double diag_reg = 0.0, jitter = 0.0;
    int absolute = 0;

    int64_t m = 0, mp = 0;       // m = 0: no inducing set
    int64_t n = 0, chunks = 0;
    bool finished = false;
    double sigma2 = 0.0;         // host copy of scal[2] after a finish

    double* u = nullptr;         // [m_cap, d]
    double* uq = nullptr;        // [m_cap] |u|^2 / d
    double* lu = nullptr;        // [mp, mp] K_uu -> L_u
    double* gm = nullptr;        // [mp, mp] G, lower tiles
    double* lb = nullptr;        // [mp, mp] B -> L_B
    double* dinv_u = nullptr;    // [mp, 128]
    double* dinv_b = nullptr;
    double* rm = nullptr;        // [mp, ny] R
    double* ct = nullptr;        // [128, mp]: R^T, solved in place to C^T
    double* chunk = nullptr;     // [chunk_rows, mp] K(X_c, U) -> Vt
    double* pt = nullptr;        // [test_cap, mp] K(X_t, U) -> P
    double* qt = nullptr;        // [test_cap, mp] Q
    double* xq = nullptr;        // [max(chunk_rows, test_cap)] |x|^2 / d of a chunk / test block
    double* kd = nullptr;        // [same] K(x, x)
    double* t = nullptr;         // [t_rows, 128] solve scratch
    int64_t t_rows = 0;
    double* ws = nullptr;        // split partials of the Gram kernel: ws_doubles, enough for every mp up to mp_cap
    int64_t ws_doubles = 0;
    double* scal = nullptr;      // [kSpScal]: sum K_ii, jitter added, sigma2; from kSpYY on the evidence's sums
    int* status = nullptr;
    // full covariance only (grown on first use)
    int64_t full_cap = 0;
    double* fp = nullptr;        // [full_cap, mp_cap]
    double* fq = nullptr;
    double* fc = nullptr;        // [full_cap, full_cap]
    double* fxq = nullptr;       // [full_cap]
    // the evidence (nngp_sparse_reserve_evidence); all NULL on a handle that never reserves
    bool ev_reserved = false;
    double* ev_a = nullptr;      // [mp, mp] K~_uu^-1, then M' (the operand of D_c = K_cu M')
    double* ev_m = nullptr;      // [mp, mp] the matrix seed of the symmetric pass over K_uu
    double* ev_t = nullptr;      // [mp, mp] L_u^-T, then L_u^-T L_B^-T
    double* ev_d = nullptr;      // [chunk_rows, mp] D_c
    double* ev_vec = nullptr;    // [2 mp_cap + chunk_rows]: gamma, the row sums of squares of L_B^-T, beta_c
    double* ev_part = nullptr;   // [4 n_dense][ev_tiles]: one slot per tile of either pass
    int64_t ev_tiles = 0;
    bool have_terms = false;
    int n_terms = 0;
    double terms[2 * (2 * NNGP_MAX_DENSE + 1) + 7] = {};
    // per-feature relevances (nngp_sparse_reserve_ard, include/nngp_sparse_ard.h); all NULL / empty on a handle that never reserves
    bool ard_reserved = false;
    bool have_rel = false;       // nngp_sparse_set_relevance gave relevances: every entry point takes raw rows and scales them
    double* ard_s = nullptr;     // [2 d]: s, then sqrt(s) (taken on the host)
    double* ard_u = nullptr;     // [m_cap, d] the raw inducing rows (u holds them scaled)
    double* ard_xs = nullptr;    // [max(chunk_rows, test_cap), d] a chunk or a test block, scaled
    double* ard_fxs = nullptr;   // [ard_fcap, d] the test rows of a full-covariance predict, scaled (grown with fp / fq)
    int64_t ard_fcap = 0;
    double* ard_kb = nullptr;    // [chunk_rows, mp_cap] kbar of the rank-one seed (kbar of the dense seed overwrites ev_d)
    double* ard_qrow = nullptr;  // [2][column tiles][chunk_rows] RectArgs::qrow
    double* ard_qcol = nullptr;  // [2][row tiles of a chunk][mp_cap] RectArgs::qcol
    double* ard_qbar = nullptr;  // [2][tiles per side][mp_cap] MllArgs::qbar of the pass over K_uu
    double* ard_part = nullptr;  // [3][row blocks][d] per row block the contraction of either seed and sum x_ik^2 (a chunk, or U)
    double* ard_acc = nullptr;   // [8 d + 2 mp_cap]: the chunks' sums [3 d], the column terms [2 d], the K_uu half [3 d], then
                                 // per seed sum_i qbar2 over every row of every chunk [2][mp_cap]
    std::vector<double> ard_host, ard_terms;  // ard_acc's first 8 d on the host; nngp_sparse_ard_terms (4 d)
    bool have_ard_terms = false;
};

namespace nngp {
// What a new kernel or new relevances leave of a fit: no inducing set, no rows, no evidence terms
inline void sparse_drop_fit(nngp_sparse* h) {
    h->m = h->mp = h->n = h->chunks = 0;
    h->finished = h->have_terms = false;
    h->sigma2 = 0.0;
}
// For the stand-alone entry points that own no handle: one stream-ordered block of doubles carved into the named pieces (one
// hipMallocAsync, every pointer set), work() queued on s, and on the way out, whatever work returned, the block freed behind it
// and s synchronised.
template <class Work>
int with_stream_block(hipStream_t s, std::initializer_list<std::pair<double**, int64_t>> pieces, Work work) {
    int64_t total = 0;
    for (const auto& p : pieces) total += p.second;
    double* buf = nullptr;
    NNGP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&buf), sizeof(double) * total, s));
    double* next = buf;
    for (const auto& p : pieces) {
        *p.first = next;
        next += p.second;
    }
    const int rc = work();
    (void)hipFreeAsync(buf, s);
    NNGP_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
}
// sparse_gp.hip.  out [rp, mp] <- K(x [rows, d], U) L_u^-T: zero, cross build, solve in place (rp = rows rounded up to 128);
// skip & 1 leaves out the build, skip & 2 the solve (then out = K(x, U), zero beyond rows and m)
int sparse_cross(nngp_sparse* h, const double* x, const double* xq, int64_t rows, double* out, hipStream_t s, int skip = 0);
// sparse_evidence.hip.  scal[kSpYY] += |y_c|^2, scal[kSpQ + l] += sum_i q_i^(l) of the chunk (xq = |x_i|^2 / d): one workgroup,
// fixed order
int sparse_evidence_sums(nngp_sparse* h, const double* xq, const double* y, int64_t c, hipStream_t s);
void sparse_evidence_free(nngp_sparse* h);
// The evaluation behind nngp_sparse_evidence_grad and nngp_sparse_evidence_grad_ard.  grad_s: host, d values, or NULL for the
// pass without relevances' derivatives; x holds raw rows when the handle has relevances.
int sparse_evidence_grad_core(nngp_sparse* h, const double* x, const double* y, int64_t n, int bound, double* nlml, double* grad,
                              double* grad_s, const char* who, hipStream_t s);
// sparse_ard.hip (include/nngp_sparse_ard.h).  sparse_ard_scale: out [rows, d] = x o sqrt(s), one multiply per element.
// The gradient's steps, in call order: begin zeroes the accumulators; uu runs the symmetric pass over K_uu with ARD set (the
// layer partials land in ev_part as from the plain pass; cmat: an [mp, mp] scratch) and its contraction with the raw inducing
// rows; chunk runs the rectangular pass with ARD set over one chunk (layer partials in ev_part likewise; xs the scaled rows,
// x_raw the raw ones; ev_d holds D_c and is overwritten) and the contraction; end adds the column terms and queues the host copy;
// finish_host (after the stream is synchronised) assembles grad_s and the terms.
int sparse_ard_scale(const nngp_sparse* h, const double* x, int64_t rows, double* out, hipStream_t s);
int sparse_ard_begin(nngp_sparse* h, hipStream_t s);
int sparse_ard_uu(nngp_sparse* h, const double* seed, const double* gamma, double* cmat, hipStream_t s);
int sparse_ard_chunk(nngp_sparse* h, const double* x_raw, const double* xs, int64_t c, const double* beta, const double* gamma,
                     hipStream_t s);
int sparse_ard_end(nngp_sparse* h, hipStream_t s);
void sparse_ard_finish_host(nngp_sparse* h, bool vfe, double s2, double ts, double bb, double gg, double* grad_s);
int sparse_ard_full_reserve(nngp_sparse* h, int64_t cap, hipStream_t s);  // grows ard_fxs to cap rows
void sparse_ard_free(nngp_sparse* h);
}  // namespace nngp
