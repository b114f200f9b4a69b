"""Integer referee, float64 restatement, input families and per-entry gates for the sliced int8 product (csrc/gemm_i8s.hip) and its
stand-alone operators (include/nngp_i8s.h).  Test infrastructure only: never imported by the product.  CPU only.

Every step of the pipeline is exact or one counted rounding, so the referee is integer arithmetic:
  scale    scale_of restates the COMMENT above i8s_scale_of: the smallest power of two s with max|row| / s <= 126/256, found by
           comparing exact fractions; 1 for a zero row (and for a maximum below 2^-960), NaN for a row that is not finite or
           reaches 1e300 (include/nngp_i8s.h).  For the kernel-matrix cut the maximum is replaced by the bound
           sqrt(K_ii max_j K_jj) (1 + 1e-9) in 80-bit arithmetic; decision_margin says how far that bound is from the one place
           where an ulp of the device's sqrt could change the scale (f = 126/128), and the tests require 1e-12.
  digits   X = rint(x 2^(8 ns) / s) (ties to even; the scaling by a power of two is exact), and the planes of a row are accepted
           when sum_i dig_i 256^(ns-1-i) = X with every plane read as int8 -- the lower digits of such a sum are unique, and a
           top digit that wrapped gives a sum 256^ns off.  digits() also produces them, by floor division.
  sums     S_e = sum_{ia + ib = e} A_ia B_ib^T: one float64 matrix product per diagonal over the concatenated planes, exact
           (at most 7 pairs x k x 2^14 < 2^53), cast to int64.
  E        W sum_e 256^-e S_e + beta cin + gamma g, W = alpha s_a s_b 2^-16: every float64 is an integer times a power of
           two, so E is formed in Python integers at one common binary point and handed out as an unevaluated sum hi + lo of two
           float64 (hi = E correctly rounded, lo = the remainder correctly rounded: 2^-106 relative).

The restatement (combine, rowstats, floor_ratio) is the device's float64 arithmetic in NumPy: the Horner combination in the same
order with one IEEE operation per step (the library is built without contraction, so the device is expected to agree with it bit
for bit; the gates do not rely on that), the fused row sums and the floor estimate in NumPy's order.

Gates (no device number enters any of them):
  planes, scales, the written-back row and out32 = float32(out): bit for bit.
  out against E: the smaller of the counted bound (ndiag + 4) u unit, unit = |W| sum_e 256^-e |S_e| + |beta cin| + |gamma g|
      (ndiag Horner additions, w, w s_b, the product with t, beta cin and the sum; gamma g and its sum when gamma != 0 are
      covered by the same count because beta cin, gamma g are then two of four), and 4 x the worst error of the restatement
      against E for that plan and family (MEASURED, in the same unit; measured again by tests/test_i8s_host.py).
  var, delta, zstat[2 r] against exact sums over the device's own out: (cols + 8) u sum |g| |cin + out| (and its kin), or 4 x the
      restatement's figure when that is smaller; zstat[2 r + 1] bit for bit.
  the floor ratios against floor_reference (80-bit, with the EXACT var of the device's out): (cols + 2) u for the sum of squares,
      8 u for the expression's own roundings (two square roots, four products, pow, the division), and (cols + 8) u of var's unit
      over var for the device's own divisor.
A NaN or Inf in a result is an infinite error.
"""
import fractions
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PLANS = ((2, 2, 0), (2, 2, 2), (3, 5, 4), (5, 3, 4), (5, 5, 4), (4, 6, 3), (7, 7, 6), (4, 7, 7), (7, 4, 7))
COEFFS = ((-1.0, 1.0, 0.0), (0.7, 1.3, 0.0), (-1.0, 1.0, -1e-3))
TINY = 2.0 ** -960      # a row maximum below this counts as zero
HUGE = 1.0e300          # a row that reaches this (or is not finite) has the scale NaN


# ------------------------------------------------------------------------------------------------------------------ scales
def scale_of(mx):
    """The smallest power of two s with mx / s <= 126/256, by exact fractions; the rows the planes cannot hold as documented."""
    mx = float(mx)
    if not mx < HUGE:
        return float("nan")
    if not mx >= TINY:
        return 1.0
    m = fractions.Fraction(mx)
    s = fractions.Fraction(2) ** math.frexp(mx)[1]
    lim = fractions.Fraction(126, 256)
    while m / s > lim:
        s *= 2
    while m / (s / 2) <= lim:
        s /= 2
    return float(s)


def row_scales(x):
    x = np.asarray(x, dtype=np.float64)
    mag = np.where(np.abs(x) < HUGE, np.abs(x), np.inf)   # NaN counts as Inf
    return np.array([scale_of(v) for v in mag.max(axis=1)]) if x.shape[1] else np.ones(x.shape[0])


def kernel_bounds(k):
    """sqrt(|K_ii| max_j |K_jj|) (1 + 1e-9) per row in 80-bit arithmetic."""
    d = np.abs(np.diag(np.asarray(k, dtype=np.float64))).astype(LD)
    return np.sqrt(d * d.max()) * (LD(1) + LD("1e-9"))


def decision_margin(bounds):
    """min over the non-zero bounds of |f - 126/128| / f, f the mantissa in [0.5, 1): the relative distance to the only value
    at which the scale changes (a power of two itself is no such point: 0.999.. 2^e and 2^e take the same scale)."""
    b = np.asarray(bounds, dtype=LD)
    b = b[b > 0]
    if b.size == 0:
        return np.inf
    f, _ = np.frexp(b)
    return float(np.min(np.abs(f - LD(126) / LD(128)) / f))


def kernel_scales(k):
    return np.array([scale_of(float(b)) for b in kernel_bounds(k)])


# ------------------------------------------------------------------------------------------------------------------ digits
def fixed_point(x, scale, ns):
    """X = rint(x 2^(8 ns) / scale) as int64 [rows, cols]; scale [rows] powers of two."""
    x = np.asarray(x, dtype=np.float64)
    e = (8 * ns - np.frexp(scale)[1] + 1).astype(np.int64)   # scale = 2^(frexp exponent - 1)
    y = np.ldexp(x, e[:, None])
    assert np.all(np.abs(y) < 2.0 ** 62)
    return np.rint(y).astype(np.int64)


def digits(xint, ns):
    """The balanced base-256 digits of X, most significant first: int64 [ns, ...]; the top one is whatever is left."""
    out = np.empty((ns,) + xint.shape, dtype=np.int64)
    x = xint.copy()
    for s in range(ns - 1, 0, -1):
        d = np.mod(x + 128, 256) - 128
        out[s] = d
        x = (x - d) // 256
    out[0] = x
    return out


def planes_value(planes):
    """sum_i dig_i 256^(ns-1-i) with every plane read as int8."""
    p = np.asarray(planes)
    assert p.dtype == np.int8
    ns = p.shape[0]
    v = np.zeros(p.shape[1:], dtype=np.int64)
    for i in range(ns):
        v = v * 256 + p[i].astype(np.int64)
    return v


def check_planes(planes, xint):
    """The planes are the digits of X: returns the number of entries at which they are not (0 = accepted)."""
    return int(np.count_nonzero(planes_value(planes) != xint))


def rounded_rows(xint, scale, ns):
    """X scale 2^(-8 ns): what the write-back holds."""
    e = (np.frexp(scale)[1] - 1 - 8 * ns).astype(np.int64)
    return np.ldexp(xint.astype(np.float64), e[:, None])


def cut(x, ns, scale=None):
    """(scales, X, digit planes as int8 [ns, rows, cols]) of the rows of x."""
    scale = row_scales(x) if scale is None else np.asarray(scale, dtype=np.float64)
    assert np.all(np.isfinite(scale)), "a row the planes cannot hold has no digits"
    xi = fixed_point(x, scale, ns)
    d = digits(xi, ns)
    assert np.all(np.abs(d[0]) <= 127), "a top digit beyond int8: the scale is too small for this row"
    return scale, xi, d.astype(np.int8)


# ------------------------------------------------------------------------------------------------- plane sums and the exact E
def plan_diagonals(nsa, nsb, cut_):
    """[(e, [(ia, ib), ...])] for e = cut .. 0 (the order of the Horner combination), cut clamped to nsa + nsb - 2."""
    if not (1 <= nsa <= 7 and 1 <= nsb <= 7 and cut_ >= 0):
        raise ValueError("1..7 planes per operand")
    cut_ = min(cut_, nsa + nsb - 2)
    out = []
    for e in range(cut_, -1, -1):
        out.append((e, [(ia, e - ia) for ia in range(nsa) if 0 <= e - ia < nsb]))
    return out


def plane_sums(da, db, diags):
    """{e: S_e int64 [m, n]}: da [nsa, m, k], db [nsb, n, k] int8."""
    k = da.shape[2]
    assert 7 * k * 2 ** 14 < 2 ** 53
    fa, fb = da.astype(np.float64), db.astype(np.float64)
    out = {}
    for e, pairs in diags:
        a = np.concatenate([fa[ia] for ia, _ in pairs], axis=1)
        b = np.concatenate([fb[ib] for _, ib in pairs], axis=1)
        out[e] = (a @ b.T).astype(np.int64)
    return out


def _int_parts(x):
    """x = mant 2^exp with integer mant: (object array of Python ints, int64 exponents); zeros get exponent 0."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.isfinite(x))
    m, e = np.frexp(x)
    mant = np.ldexp(m, 53).astype(np.int64)
    exp = np.where(mant == 0, 0, e.astype(np.int64) - 53)
    return mant.astype(object), exp


def _shift(mant, sh):
    return np.frompyfunc(lambda a, b: a << b, 2, 1)(mant, sh.astype(object))


def _hi_lo(val, q):
    """val 2^-q for an object array of Python ints: (correctly rounded float64, the remainder correctly rounded)."""
    two_q = 1 << q

    def one(v):
        hi = v / two_q                       # int / int: correctly rounded
        num, den = hi.as_integer_ratio()     # den = 2^d
        d = den.bit_length() - 1
        if d <= q:
            return hi, (v - (num << (q - d))) / two_q
        return hi, ((v << (d - q)) - num) / den
    f = np.frompyfunc(one, 1, 2)
    hi, lo = f(val)
    return hi.astype(np.float64), lo.astype(np.float64)


class Exact:
    """A sum of products of float64 numbers, held per entry as a Python integer at one binary point 2^-q."""

    def __init__(self, shape):
        self.shape = shape
        self.terms = []   # (object mantissa array, int64 exponent array)

    def add(self, mant, exp):
        self.terms.append((np.broadcast_to(mant, self.shape), np.broadcast_to(exp, self.shape)))

    def add_product(self, *factors):
        mant, exp = None, None
        for f in factors:
            m, e = _int_parts(f)
            mant, exp = (m, e) if mant is None else (mant * m, exp + e)
        self.add(mant, exp)

    def value(self):
        q = int(max(0, max(int(-e.min()) for _, e in self.terms)))
        tot = None
        for m, e in self.terms:
            t = _shift(m, e + q)
            tot = t if tot is None else tot + t
        return tot, q

    def hi_lo(self):
        tot, q = self.value()
        return _hi_lo(tot, q)

    def row_sums_hi_lo(self):
        tot, q = self.value()
        return _hi_lo(tot.sum(axis=1), q)


def exact_combination(sums, diags, sa, sb, alpha, beta, cin, gamma, g):
    """(E_hi, E_lo, unit): E = alpha s_a s_b 2^-16 sum_e 256^-e S_e + beta cin + gamma g exactly, as hi + lo; unit as in the gates."""
    top = diags[0][0]
    shape = sums[top].shape
    t = np.zeros(shape, dtype=object)
    tabs = np.zeros(shape, dtype=np.float64)
    for e, _ in diags:
        t = t + (sums[e].astype(object) << (8 * (top - e)))
        tabs += np.abs(sums[e]).astype(np.float64) * 256.0 ** -e
    ex = Exact(shape)
    ma, ea = _int_parts(np.float64(alpha))
    pa = (np.frexp(sa)[1] - 1).astype(np.int64)[:, None]
    pb = (np.frexp(sb)[1] - 1).astype(np.int64)[None, :]
    ex.add(t * int(ma), int(ea) + pa + pb - 16 - 8 * top)
    unit = abs(alpha) * sa[:, None] * sb[None, :] * 2.0 ** -16 * tabs
    if beta != 0.0:
        ex.add_product(np.float64(beta), cin)
        unit = unit + np.abs(beta * cin)
    if gamma != 0.0:
        ex.add_product(np.float64(gamma), g)
        unit = unit + np.abs(gamma * g)
    hi, lo = ex.hi_lo()
    return hi, lo, unit


def worst(got, hi, lo, unit):
    """max over the entries of |got - (hi + lo)| / (u unit); a non-finite result, or an error where the unit is zero, is infinite."""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs((got - hi) - lo)
    bad = (unit == 0) & (err > 0)
    if bad.any():
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / (U * unit), 0.0)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------- the restatement
def combine(sums, diags, sa, sb, alpha, beta, cin, gamma, g):
    """The device's combination pass in float64 NumPy: Horner from the diagonal with the largest e, then w s_b t + beta cin + gamma g,
    one IEEE operation per step, left to right."""
    t = np.zeros(sums[diags[0][0]].shape)
    for e, _ in diags:
        t = t * 0.00390625 + sums[e].astype(np.float64)
    w = (alpha * sa) * (1.0 / 65536.0)
    v = (w[:, None] * sb[None, :]) * t
    if beta != 0.0:
        v = v + beta * cin
    if gamma != 0.0:
        v = v + gamma * g
    return v


def rowstats(base, g, cin, out):
    """(var, delta, zstat [rows, 2]) of the fused pass, in NumPy's order."""
    zs = np.stack([np.sum(g * g, axis=1), np.max(np.abs(g), axis=1)], axis=1)
    return base - np.sum(g * (cin + out), axis=1), np.sum(g * out, axis=1), zs


def rowstats_exact(base, g, cin, out):
    """Exact base - sum_c g (cin + out), sum_c g out, sum_c g^2 per row as (hi, lo) pairs, and their units |base| + sum |g| |cin + out|,
    sum |g out|, sum g^2."""
    first = np.zeros_like(g)
    first[:, 0] = 1.0
    res = []
    for terms in (((-g, cin), (-g, out), (first, np.asarray(base, dtype=np.float64)[:, None])), ((g, out),), ((g, g),)):
        ex = Exact(g.shape)
        for t in terms:
            ex.add_product(*t)
        res.append(ex.row_sums_hi_lo())
    units = (np.abs(base) + np.sum(np.abs(g) * np.abs(cin + out), axis=1), np.sum(np.abs(g * out), axis=1), np.sum(g * g, axis=1))
    return res, units


def dropped_pairs(nsa, nsb, cut_):
    """The comment above k_i8s_floor_ratio: the pairs on the first dropped diagonal, + 2 for the operands' own truncation."""
    c = min(cut_, nsa + nsb - 2)
    return c, 2 + sum(1 for ia in range(nsa) if 0 <= c + 1 - ia < nsb)


def floor_reference(z, var, kscale, nsa, nsb, cut_):
    """max_r 5404.7 sqrt(dropped) 256^-(cut+3) |z_r|_2 scale_of(max|z_r|) sqrt(sum s_k^2) / var_r in 80-bit arithmetic; rows with
    var <= 0 count 1e300 when their estimate is positive, else 0."""
    c, dropped = dropped_pairs(nsa, nsb, cut_)
    coef = LD("5404.7") * np.sqrt(LD(dropped)) * LD(256) ** LD(-(c + 3))
    z = np.asarray(z, dtype=np.float64).astype(LD)
    est = np.sqrt(np.sum(z * z, axis=1)) * coef * row_scales(z.astype(np.float64)).astype(LD) * np.sqrt(np.sum(kscale.astype(LD) ** 2))
    v = np.asarray(var).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(v > 0, est / np.where(v > 0, v, 1), np.where(est > 0, LD("1e300"), LD(0)))
    return ratio


def truncation_bound(a, b, sa, sb, nsa, nsb, cut_):
    """|exact digit-plane sum - a b^T| <= digit rounding + dropped pairs, per entry [m, n] (worst case)."""
    k = a.shape[1]
    ha, hb = sa * 256.0 ** -nsa / 2, sb * 256.0 ** -nsb / 2
    ma, mb = np.abs(a).max(axis=1), np.abs(b).max(axis=1)
    rounding = k * (ha[:, None] * mb[None, :] + hb[None, :] * ma[:, None] + ha[:, None] * hb[None, :])
    c = min(cut_, nsa + nsb - 2)
    drop = sum(128.0 ** 2 * k * 256.0 ** -(ia + ib + 2) for ia in range(nsa) for ib in range(nsb) if ia + ib > c)
    return rounding + drop * sa[:, None] * sb[None, :]


# ------------------------------------------------------------------------------------------------------------ input families
def edge_values(ns):
    """Chosen X of the digit_edges family for ns planes (the row scale is 1: x = X 2^(-8 ns)), and the ties X + 1/2."""
    top = 256 ** (ns - 1)
    low_min = sum(-128 * 256 ** (ns - 1 - i) for i in range(1, ns))
    low_max = sum(127 * 256 ** (ns - 1 - i) for i in range(1, ns))
    xs = [0, 1, -1, 127, -127, 128, -128, 129, -129, low_min, low_max, 5 * top + low_min, -5 * top + low_max, 5 * top + low_max,
          126 * top, -126 * top, 126 * top - 1, -126 * top + 1, 125 * top + 200 * (top // 256 if ns >= 2 else 0)]
    ties = [0.5, 1.5, 2.5, -0.5, -1.5, 127.5, 128.5, -128.5]      # small X: representable at every ns
    if ns <= 6:                                                   # X + 1/2 near the row maximum needs 8 ns - 1 + 1 bits <= 53
        ties += [100 * top + 0.5, 100 * top + 1.5, -(100 * top + 0.5), 125 * top + low_max + 0.5]
    return xs, ties


def digit_edges(rows, cols, ns, seed=0):
    """Rows of chosen X (edge_values) and ties, padded with random X, with a head of at least 126 256^(ns-1) somewhere in each row
    so that the head alone decides the scale (2^(-3 (r % 8)), the power of two row r is multiplied by, for the head 126 256^(ns-1);
    twice that for the other three heads).  The maximum's mantissa is 126/128 exactly, 1/2
    exactly, one ulp above 126/128 or one ulp below 1, by (r + cols) % 4.  (At ns = 7 the values 126 256^6 -+ 1 need 56 bits and are
    rounded to float64 before they enter the row; ties next to the row maximum exist for ns <= 6 only.)"""
    rng = np.random.default_rng(1000 * ns + cols + seed)
    top = 256 ** (ns - 1)
    xs, ties = edge_values(ns)
    vals = np.array([float(v) for v in xs] + ties)
    out = np.empty((rows, cols))
    for r in range(rows):
        x = rng.integers(-126 * top, 126 * top + 1, size=cols).astype(np.float64)
        idx = rng.permutation(cols)[:min(cols, vals.size)]
        x[idx] = vals[rng.permutation(vals.size)[:idx.size]]
        head = {0: 126.0 * top, 1: 128.0 * top, 2: float(np.nextafter(126.0 * top, np.inf)), 3: float(np.nextafter(128.0 * top, 0.0))}[(r + cols) % 4]
        x[cols - 1 if r % 2 == 0 else 0] = head if r % 3 else -head
        out[r] = np.ldexp(x, -8 * ns - 3 * (r % 8))
    return out


def spread(rows, cols, seed=0, row_spread=6):
    """Standard normals times 2^(-18..0) per entry and 2^(-row_spread..0) per row; row 1 (when there is one) is zero, row 2 has its only
    non-zero entry in the last column, and row 0 of such a block has its only one in column 4096 (when there is one)."""
    rng = np.random.default_rng(77 + 13 * rows + cols + seed)
    x = rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-18, 1, (rows, cols))) * np.exp2(rng.integers(-row_spread, 1, (rows, 1)))
    if rows > 1:
        x[1] = 0.0
    if rows > 2:
        v = x[2, -1]
        x[2] = 0.0
        x[2, -1] = v
    if rows > 2 and cols > 4096:
        v = x[0, 4096]
        x[0] = 0.0
        x[0, 4096] = v
    return x


def integers(rows, cols, seed=0, bound=126 * 2 ** 16):
    """Integers of up to 23 bits; 126 2^16 is the largest a row may hold and keep the scale 2^24, at which three planes are exact."""
    rng = np.random.default_rng(5 + rows + 3 * cols + seed)
    return rng.integers(-bound, bound + 1, (rows, cols)).astype(np.float64)


def kernel_matrix(kind, n, seed=0):
    """Bitwise symmetric PSD [n, n] with entries of both signs from an integer G (data rows: 300 of 384, 100 of 128; the rest is
    zero padding).  kind "gram": random G in [-40, 40]; "edges": rows 3 and 7 both carry the largest diagonal (|K_37| = the largest diagonal),
    row 11 = -row 3 (K_3,11 = -that), row 5 is zero (a zero diagonal entry inside the data); "psd_small": G G^T with |K| < 2^23."""
    rng = np.random.default_rng(31 + n + seed)
    nd, d = (300, 24) if n >= 384 else (n * 100 // 128, 24)
    hi = 40 if kind != "psd_small" else 12
    g = rng.integers(-hi, hi + 1, (nd, d)).astype(np.float64)
    if kind == "edges":
        g[3] = hi + 1 - (np.arange(d) % 2) * (2 * hi + 2)   # the longest row, alternating signs
        g[7] = g[3]
        g[11] = -g[3]
        g[5] = 0.0
        g[nd - 1] = g[3]
    k = np.zeros((n, n))
    k[:nd, :nd] = g @ g.T
    assert np.array_equal(k, k.T) and np.abs(k).max() < 2.0 ** 23
    return k


def product_inputs(family, mp, n, seed=0):
    """(z [mp, n], kmat [n, n], cin [mp, n]) of a residual product."""
    rng = np.random.default_rng(911 + mp + n + seed)
    if family == "integers":
        kmat = kernel_matrix("psd_small", n, seed)
        z = rng.integers(-2 ** 12, 2 ** 12 + 1, (mp, n)).astype(np.float64)
        cin = rng.integers(-2 ** 20, 2 ** 20 + 1, (mp, n)).astype(np.float64)
        return z, kmat, cin
    kmat = kernel_matrix("edges" if family == "digit_edges" else "gram", n, seed)
    if family == "digit_edges":
        z = digit_edges(mp, n, 5, seed)
    elif family == "spread":
        z = spread(mp, n, seed)
    else:
        z = rng.standard_normal((mp, n)) * 1e-3
    cin = rng.standard_normal((mp, n)) * np.abs(kmat).max() * 1e-2
    return z, kmat, cin


def gemm_inputs(family, m, n, k, seed=0):
    """(a [m, k], b [n, k], cin [m, n]) of a general product with own-row scales on both sides."""
    rng = np.random.default_rng(4242 + m + n + k + seed)
    if family == "integers":
        # |a . b| <= k 2^23 2^20 < 2^53 for k <= 512: the integer result is a float64
        return integers(m, k, seed), integers(n, k, seed + 1, 2 ** 20), rng.integers(-2 ** 20, 2 ** 20 + 1, (m, n)).astype(np.float64)
    if family == "digit_edges":
        return digit_edges(m, k, 5, seed), digit_edges(n, k, 7, seed + 1), rng.standard_normal((m, n))
    return spread(m, k, seed), spread(n, k, seed + 1), rng.standard_normal((m, n))


class ProductCase:
    """Referee quantities of one product: a [m, k] with scales sa (own rows), b [n, k] with scales sb (given, or own rows)."""

    def __init__(self, a, b, nsa, nsb, cut_, sb=None):
        self.a, self.b, self.nsa, self.nsb, self.cut = a, b, nsa, nsb, cut_
        self.sa, self.xa, self.da = cut(a, nsa)
        self.sb, self.xb, self.db = cut(b, nsb, sb)
        self.diags = plan_diagonals(nsa, nsb, cut_)
        self.sums = plane_sums(self.da, self.db, self.diags)
        self.a_rounded = rounded_rows(self.xa, self.sa, nsa)

    def exact(self, alpha, beta, cin, gamma=0.0, g=None):
        return exact_combination(self.sums, self.diags, self.sa, self.sb, alpha, beta, cin, gamma, g)

    def restated(self, alpha, beta, cin, gamma=0.0, g=None):
        return combine(self.sums, self.diags, self.sa, self.sb, alpha, beta, cin, gamma, g)

    def counted(self):
        return float(len(self.diags) + 4)

    def true_product(self):
        return (self.a.astype(LD) @ self.b.astype(LD).T)


def residual_case(family, mp, n, plan, seed=0):
    """(ProductCase of z against kmat with the kernel-matrix scales, cin) for nngp_i8s_residual."""
    z, kmat, cin = product_inputs(family, mp, n, seed)
    return ProductCase(z, kmat, plan[0], plan[1], plan[2], sb=kernel_scales(kmat)), cin


def gemm_case(family, m, n, k, plan, seed=0):
    """(ProductCase with own-row scales on both sides, cin) for nngp_gemm_nt_i8s."""
    a, b, cin = gemm_inputs(family, m, n, k, seed)
    return ProductCase(a, b, plan[0], plan[1], plan[2]), cin


MEASURE_SHAPE, MEASURE_GEMM_SHAPE = (128, 128), (128, 128, 200)
FAMILIES = ("integers", "digit_edges", "spread", "kernel")


def measure(plan, family):
    """Worst error of the restatement against E in u unit over the coefficient sets, on the residual route and (but for the
    kernel family, which has no general product) on the general product."""
    cases = [residual_case(family, *MEASURE_SHAPE, plan)]
    if family != "kernel":
        cases.append(gemm_case(family, *MEASURE_GEMM_SHAPE, plan))
    w = 0.0
    for i, (pc, cin) in enumerate(cases):
        for alpha, beta, gamma in COEFFS:
            if i == 1 and gamma != 0.0:
                continue
            g = pc.a_rounded if gamma != 0.0 else None
            w = max(w, worst(pc.restated(alpha, beta, cin, gamma, g), *pc.exact(alpha, beta, cin, gamma, g)))
    return w


# --------------------------------------------------------------------------------------------------------------------- gates
# (nsa, nsb, cut) -> family -> worst error of the restatement against E over the coefficient sets, in u unit (measure():
# the residual route at 128 x 128 and the general product at 128 x 128 x 200; tests/test_i8s_host.py measures and prints them again)
MEASURED = {
    (2, 2, 0): {"integers": 1.771, "digit_edges": 1.968, "spread": 1.943, "kernel": 1.941},
    (2, 2, 2): {"integers": 1.766, "digit_edges": 1.968, "spread": 1.938, "kernel": 1.936},
    (3, 5, 4): {"integers": 1.766, "digit_edges": 1.964, "spread": 1.926, "kernel": 1.956},
    (5, 3, 4): {"integers": 1.766, "digit_edges": 1.908, "spread": 1.940, "kernel": 1.976},
    (5, 5, 4): {"integers": 1.766, "digit_edges": 1.912, "spread": 1.951, "kernel": 1.976},
    (4, 6, 3): {"integers": 1.766, "digit_edges": 1.957, "spread": 1.960, "kernel": 1.954},
    (7, 7, 6): {"integers": 1.766, "digit_edges": 2.305, "spread": 2.364, "kernel": 2.143},
    (4, 7, 7): {"integers": 1.766, "digit_edges": 1.950, "spread": 1.968, "kernel": 1.954},
    (7, 4, 7): {"integers": 1.766, "digit_edges": 2.305, "spread": 2.344, "kernel": 2.187},
}


def gate(plan, family):
    """The gate of |out - E| in u unit: the smaller of the counted bound and 4 x the restatement's own figure."""
    nsa, nsb, c = plan
    counted = len(plan_diagonals(nsa, nsb, c)) + 4
    return min(float(counted), 4.0 * MEASURED[plan][family])
