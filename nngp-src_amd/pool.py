"""Batch-aware pool selection on the device (``include/nngp_pool.h``, ``csrc/pool_greedy.hip``): greedy picks by conditional
variance -- take the pool query with the largest posterior variance, condition the pool's covariance on observing it (with the
model's observation noise), pick again.  That is a partial pivoted Cholesky factorisation of the pool covariance; unlike the marginal
score of ``nngp_pool_select`` it does not spend two labels on two near-identical queries.

``GPModel.select_pool(..., method="greedy")`` is the way from a fitted model; ``pool_select_greedy`` below takes any symmetric
positive semi-definite covariance (a torch tensor or a NumPy array), for instance the one of the RBF GP.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib


def check_greedy_arguments(m: int, count: int, noise: float):
    """(count, noise) after the checks of include/nngp_pool.h: 0 <= count <= m, noise finite and >= 0."""
    count, noise = int(count), float(noise)
    if not 0 <= count <= int(m):
        raise ValueError("count must be in 0 .. m = %d, got %d" % (m, count))
    if not (noise >= 0.0 and math.isfinite(noise)):
        raise ValueError("noise must be finite and >= 0, got %r" % (noise,))
    return count, noise


def greedy_on_device(lib, cov, count: int, noise: float, want_gains: bool = True, want_factor: bool = False):
    """nngp_pool_select_greedy on a float64 CUDA tensor [m, m] whose rows are contiguous (any row stride >= m): device tensors
    (indices [count] int64, gains [count] or None, factor [count, m] or None).  Enqueues on the current stream; nothing is read back."""
    import torch
    m = int(cov.shape[0])
    assert cov.is_cuda and cov.dtype == torch.float64 and cov.dim() == 2 and cov.shape[1] == m
    assert m == 1 or (cov.stride(1) == 1 and cov.stride(0) >= m)
    count, noise = check_greedy_arguments(m, count, noise)
    idx = torch.empty((count,), dtype=torch.int64, device=cov.device)
    gains = torch.empty((count,), dtype=torch.float64, device=cov.device) if want_gains else None
    factor = torch.empty((count, m), dtype=torch.float64, device=cov.device) if want_factor else None
    if count > 0:
        _lib.check(lib.nngp_pool_select_greedy(_lib.ptr(cov), m, max(int(cov.stride(0)), m), noise, count, _lib.ptr(idx), _lib.ptr(gains),
                                               _lib.ptr(factor), m, _lib.stream_ptr()), lib)
    return idx, gains, factor


def pool_select_greedy(cov, count: int, noise: float = 0.0, return_factor: bool = False):
    """Greedy selection of ``count`` rows of a symmetric positive semi-definite ``cov`` [m, m] by conditional variance, on the GPU.

    Returns ``(indices, gains)``, or ``(indices, gains, factor)`` with ``return_factor``: the picks in the order taken, the
    conditional variance of each when it was taken (without the noise), and the [count, m] rows of the pivoted Cholesky factor.
    A torch tensor gives device tensors (a CUDA float64 tensor is used in place, row stride included); anything else goes through
    NumPy and gives NumPy arrays.  ``noise`` is the variance of the observation noise of a label (``GPModel.info()["reg"]``)."""
    import torch
    lib = _lib.load()
    as_torch = isinstance(cov, torch.Tensor)
    if not as_torch:
        cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 1:
        raise ValueError("cov must be [m, m] with m >= 1, got %s" % (tuple(cov.shape),))
    check_greedy_arguments(cov.shape[0], count, noise)
    device = _lib.require_gpu()
    if not (as_torch and cov.is_cuda and cov.dtype == torch.float64 and (cov.shape[0] == 1 or (cov.stride(1) == 1 and cov.stride(0) >= cov.shape[0]))):
        cov = _lib.to_device_f64(cov, device)
    out = greedy_on_device(lib, cov, count, noise, True, return_factor)
    out = out if return_factor else out[:2]
    return out if as_torch else tuple(t.cpu().numpy() for t in out)
