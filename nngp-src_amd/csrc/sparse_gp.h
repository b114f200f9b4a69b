// Shared between the sparse NNGP posterior (sparse_gp.hip) and its evidence (sparse_evidence.hip): the handle of
// include/nngp_sparse.h and the two steps the evidence passes borrow from the fit.
#pragma once
#include "gp_f64.h"

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
};

namespace nngp {
// sparse_gp.hip.  out [rp, mp] <- K(x [rows, d], U) L_u^-T: zero, cross build, solve in place (rp = rows rounded up to 128);
// skip & 1 leaves out the build, skip & 2 the solve (then out = K(x, U), zero beyond rows and m)
int sparse_cross(nngp_sparse* h, const double* x, const double* xq, int64_t rows, double* out, hipStream_t s, int skip = 0);
// sparse_evidence.hip.  scal[kSpYY] += |y_c|^2, scal[kSpQ + l] += sum_i q_i^(l) of the chunk (xq = |x_i|^2 / d): one workgroup,
// fixed order
int sparse_evidence_sums(nngp_sparse* h, const double* xq, const double* y, int64_t c, hipStream_t s);
void sparse_evidence_free(nngp_sparse* h);
}  // namespace nngp
