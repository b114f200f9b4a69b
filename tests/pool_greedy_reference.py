"""NumPy float64 reference of the greedy pool selection by conditional variance (include/nngp_pool.h).  Test infrastructure only.

The selection is a partial pivoted Cholesky factorisation of cov + noise * I restricted to the picks, left-looking: with d = diag(cov)

    p_j = argmax d over the indices not picked yet (equal d: the lowest index; a NaN d never wins over a number)
    c_j = (cov[:, p_j] - sum_{t<j} c_t c_t[p_j]) / sqrt(d[p_j] + noise)        (zero where d[p_j] + noise > 0 does not hold)
    d  <- d - c_j^2

Products and sums are separate roundings, as in the library (built without fused multiply-add); the order of the sum over t is the
matrix product's, not the library's, which is why the comparison allows 1e-10 and demands equal indices only where the best and the
second-best conditional variance are further apart than that (``gaps``).
"""
from __future__ import annotations

import numpy as np


def _order_key(d, picked):
    """What the pick rule maximises: d, with NaN (and a diagonal of -inf) below every number and a picked index below those."""
    key = np.where(np.isnan(d) | (d == -np.inf), -np.finfo(np.float64).max, d)
    key[picked] = -np.inf
    return key


def greedy(cov, count, noise=0.0):
    """(indices [count] int64, gains [count], factor [count, m], gaps [count]).  gaps[j]: relative distance between the best and the
    second-best conditional variance at step j, (d1 - d2) / |d1| (inf at the last index of the pool, nan where either is NaN)."""
    cov = np.asarray(cov, dtype=np.float64)
    m = cov.shape[0]
    count = int(count)
    assert cov.shape == (m, m) and 0 <= count <= m and noise >= 0.0
    d = np.diag(cov).copy()
    picked = np.zeros(m, dtype=bool)
    indices = np.zeros(count, dtype=np.int64)
    gains, gaps, factor = np.zeros(count), np.zeros(count), np.zeros((count, m))
    for j in range(count):
        key = _order_key(d, picked)
        p = int(np.argmax(key))  # first occurrence of the maximum: the lowest index
        indices[j], gains[j] = p, d[p]
        rest = key.copy()
        rest[p] = -np.inf
        if picked.sum() + 1 == m:
            gaps[j] = np.inf
        else:
            second = d[int(np.argmax(rest))]
            with np.errstate(invalid="ignore", divide="ignore"):
                gaps[j] = (d[p] - second) / abs(d[p])
        piv = d[p] + noise
        if piv > 0.0:
            c = (cov[:, p] - factor[:j].T @ factor[:j, p]) / np.sqrt(piv)
            factor[j] = c
            d = d - c * c
        picked[p] = True
    return indices, gains, factor, gaps


def remaining_variance(cov, picks, noise=0.0):
    """trace(cov - cov[:, S] (cov[S, S] + noise I)^-1 cov[S, :]): what is left of the pool's variance once the picks are labelled."""
    cov = np.asarray(cov, dtype=np.float64)
    s = np.asarray(picks, dtype=np.int64)
    if s.size == 0:
        return float(np.trace(cov))
    a = cov[np.ix_(s, s)] + noise * np.eye(s.size)
    return float(np.trace(cov) - np.sum(cov[s, :] * np.linalg.solve(a, cov[s, :])))


def replay(cov, picks, noise=0.0):
    """For each pick, in order: (its conditional variance given the earlier picks, the largest conditional variance any unpicked index
    had at that step), both exact for `cov` whatever rule chose the picks."""
    cov = np.asarray(cov, dtype=np.float64)
    picks = np.asarray(picks, dtype=np.int64)
    m = cov.shape[0]
    d = np.diag(cov).copy()
    picked = np.zeros(m, dtype=bool)
    factor = np.zeros((picks.size, m))
    got, best = np.zeros(picks.size), np.zeros(picks.size)
    for j, p in enumerate(picks):
        got[j] = d[p]
        best[j] = np.max(d[~picked])
        piv = d[p] + noise
        if piv > 0.0:
            c = (cov[:, p] - factor[:j].T @ factor[:j, p]) / np.sqrt(piv)
            factor[j] = c
            d = d - c * c
        picked[p] = True
    return got, best


def top_k(cov, count):
    """The marginal rule the greedy one is compared with: the `count` largest variances."""
    return np.argsort(np.diag(cov), kind="stable")[::-1][:count].astype(np.int64)


def synthetic_spd(m, seed, rank=8):
    """A A^T + diag(linspace(1, 2, m)) with a seeded A of the given rank."""
    a = np.random.default_rng(seed).standard_normal((m, rank))
    return a @ a.T + np.diag(np.linspace(1.0, 2.0, m))
