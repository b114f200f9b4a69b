"""Sparse NNGP: the inducing-point (DTC) posterior on the device (``include/nngp_sparse.h``, ``csrc/sparse_gp.hip``).

The exact models hold the N x N kernel; ``SparseGPModel`` keeps every label, summarises the inputs by m << N inducing rows and
pays O(N m^2) once and O(m^2) per served query with variance.  Training rows arrive in any number of calls and are uploaded
chunk by chunk, so X never has to fit on the device at once.  ``select_inducing`` chooses the inducing rows: greedy by
conditional variance of the prior kernel (``nngp_pool_select_greedy``), or at random.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from .kernel_spec import HasSpec, KernelSpec

_COV = {False: _lib.COV_NONE, None: _lib.COV_NONE, "none": _lib.COV_NONE, "diag": _lib.COV_DIAG, True: _lib.COV_FULL,
        "full": _lib.COV_FULL}
M_MAX = 16384


def check_sparse_arguments(m_cap, chunk_rows, test_cap, ny, diag_reg, jitter):
    """The checks of nngp_sparse_create, as ValueError."""
    if not 1 <= int(m_cap) <= M_MAX:
        raise ValueError("m_cap must be in 1 .. %d, got %r" % (M_MAX, m_cap))
    if int(chunk_rows) < 128 or int(chunk_rows) % 128 != 0:
        raise ValueError("chunk_rows must be a positive multiple of 128, got %r" % (chunk_rows,))
    if int(test_cap) < 1:
        raise ValueError("test_cap must be >= 1, got %r" % (test_cap,))
    if not 1 <= int(ny) <= 16:
        raise ValueError("ny must be in 1 .. 16, got %r" % (ny,))
    for name, v in (("diag_reg", diag_reg), ("jitter", jitter)):
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError("%s must be finite and >= 0, got %r" % (name, v))


class SparseGPModel(HasSpec):
    """Python owner of one ``nngp_sparse`` handle.  Keyword names and the input-scale handling follow ``GPModel``."""

    def __init__(self, m_cap: int, d: int, w_std, b_std, diag_reg: float = 1e-3, chunk_rows: int = 8192, jitter: float = 1e-8,
                 test_cap: int = 1024, diag_reg_absolute_scale: bool = False, ny: int = 1, activations=None, input_scale=None,
                 groups=None, group_weights=None, full_weight=1.0, knobs: bool = False):
        check_sparse_arguments(m_cap, chunk_rows, test_cap, ny, diag_reg, jitter)
        self.spec = KernelSpec(w_std, b_std, activations, input_scale, groups, group_weights, full_weight).resolve(d)
        self.lib = _lib.load(knobs)  # knobs=True: the timing-knob build (scripts/ only)
        self.device = _lib.require_gpu()
        self.m_cap, self.d, self.ny, self.chunk_rows = int(m_cap), int(d), int(ny), int(chunk_rows)
        self.handle = ctypes.c_void_p()
        self._check(self.spec.sparse_create(self.lib, ctypes.byref(self.handle), self.m_cap, self.chunk_rows, int(test_cap), self.d,
                                            self.ny, float(diag_reg), int(bool(diag_reg_absolute_scale)), float(jitter)))
        self.m = 0

    @classmethod
    def from_kernel_fn(cls, kernel_fn, m_cap: int, d: int, **kwargs):
        """The model of a ``stax`` kernel_fn (or a batch() wrapper of one, or a KernelSpec)."""
        return cls(m_cap, d, **KernelSpec.of(kernel_fn).as_keywords(), **kwargs)

    def _check(self, rc: int):
        _lib.check(rc, self.lib)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.nngp_sparse_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, x, what):
        if not hasattr(x, "shape") or len(x.shape) != 2 or int(x.shape[1]) != self.d:
            raise ValueError("%s must be [rows, %d], got %s" % (what, self.d, tuple(getattr(x, "shape", ()))))
        return int(x.shape[0])

    def _device_rows(self, x):
        return self.spec.scale(_lib.to_device_f64(x, self.device))

    def set_inducing(self, u):
        """u [m, d], 1 <= m <= m_cap: builds and factors K_uu + jitter; forgets every training row added before."""
        import torch
        u = u if isinstance(u, torch.Tensor) else np.asarray(u, dtype=np.float64)
        m = self._rows(u, "inducing rows")
        if not 1 <= m <= self.m_cap:
            raise ValueError("the model was created for 1..%d inducing rows, got %d" % (self.m_cap, m))
        self.m = 0
        ud = self._device_rows(u)
        self._check(self.lib.nngp_sparse_set_inducing(self.handle, _lib.ptr(ud), m, _lib.stream_ptr()))  # waits for the stream
        self.m = m
        return self

    def add_rows(self, x, y):
        """Training rows x [n, d], y [n] or [n, ny] (host or device), uploaded and accumulated chunk_rows at a time."""
        import torch
        x = x if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
        n = self._rows(x, "x")
        y = y if isinstance(y, torch.Tensor) else np.asarray(y, dtype=np.float64)
        y = y.reshape(n, -1)
        if int(y.shape[1]) != self.ny:
            raise ValueError("y must have %d column(s), got %s" % (self.ny, tuple(y.shape)))
        for r0 in range(0, n, self.chunk_rows):
            r1 = min(r0 + self.chunk_rows, n)
            xd = self._device_rows(x[r0:r1])
            yd = _lib.to_device_f64(y[r0:r1], self.device)
            self._check(self.lib.nngp_sparse_add_rows(self.handle, _lib.ptr(xd), _lib.ptr(yd), r1 - r0, _lib.stream_ptr()))
            torch.cuda.current_stream().synchronize()  # the chunk's upload goes out of scope
        return self

    def finish(self):
        self._check(self.lib.nngp_sparse_finish(self.handle, _lib.stream_ptr()))
        return self

    def fit(self, x, y, inducing):
        """set_inducing + add_rows + finish.  inducing: the rows themselves [m, d], or indices into x."""
        inducing = np.asarray(inducing) if not hasattr(inducing, "dtype") else inducing
        if inducing.ndim == 1:
            inducing = x[np.asarray(inducing, dtype=np.int64)]
        return self.set_inducing(inducing).add_rows(x, y).finish()

    def predict(self, x_test, cov="diag", as_numpy=True):
        """mean [M, ny] (+ var [M] for cov='diag', cov [M, M] for cov='full'/True): the latent function's, as in the exact model."""
        import torch
        mode = _COV[cov]
        xt = _lib.to_device_f64(x_test, self.device)
        mt = self._rows(xt, "x_test")
        xt = self._device_rows(xt)
        mean = torch.empty((mt, self.ny), dtype=torch.float64, device=self.device)
        out = None
        if mode == _lib.COV_DIAG:
            out = torch.empty((mt,), dtype=torch.float64, device=self.device)
        elif mode == _lib.COV_FULL:
            out = torch.empty((mt, mt), dtype=torch.float64, device=self.device)
        if mt > 0:
            self._check(self.lib.nngp_sparse_predict(self.handle, _lib.ptr(xt), mt, mode, _lib.ptr(mean), _lib.ptr(out),
                                                     _lib.stream_ptr()))
        if as_numpy:
            mean = mean.cpu().numpy()
            out = None if out is None else out.cpu().numpy()
        else:
            torch.cuda.current_stream().synchronize()  # xt goes out of scope
        return mean if out is None else (mean, out)

    def info(self) -> dict:
        fi = _lib.NngpSparseInfo()
        self._check(self.lib.nngp_sparse_info(self.handle, ctypes.byref(fi)))
        return {k: getattr(fi, k) for k, _ in fi._fields_}


def greedy_rows(cov, count: int):
    """The rule of nngp_pool_select_greedy with noise 0 in NumPy (``active.greedy_select``): where there is no device."""
    from .active import greedy_select
    return greedy_select(cov, int(count), 0.0)


def select_inducing(x, m: int, kernel_fn, method: str = "greedy", candidates: int = 16384, seed: int = 10):
    """Indices of m rows of x [N, d] to use as inducing rows.

    ``"random"``: m rows without replacement from ``numpy.random.RandomState(seed)``.  ``"greedy"``: the candidates are all rows
    when N <= candidates, else ``candidates`` rows drawn without replacement from ``numpy.random.RandomState(seed)``; their prior
    kernel is built on the device and ``nngp_pool_select_greedy`` with noise 0 -- the partial pivoted Cholesky of the prior --
    picks m of them.  Without a device the kernel comes from calling ``kernel_fn`` (which may be any callable
    ``kernel_fn(x, None, "nngp")`` then) and the same rule runs in NumPy."""
    x = np.asarray(x, dtype=np.float64)
    n, m, candidates = int(x.shape[0]), int(m), int(candidates)
    if x.ndim != 2 or not 1 <= m <= n:
        raise ValueError("x must be [N, d] and 1 <= m <= N (N = %d, m = %d)" % (n, m))
    if method not in ("greedy", "random"):
        raise ValueError("method must be 'greedy' or 'random', got %r" % (method,))
    if method == "random":
        return np.sort(np.random.RandomState(seed).choice(n, size=m, replace=False)).astype(np.int64)
    if candidates < m:
        raise ValueError("candidates = %d is below m = %d" % (candidates, m))
    cand = np.arange(n, dtype=np.int64)
    if n > candidates:
        cand = np.sort(np.random.RandomState(seed).choice(n, size=candidates, replace=False)).astype(np.int64)
    import torch
    if torch.cuda.is_available() and hasattr(kernel_fn, "spec"):
        from .pool import greedy_on_device
        k = kernel_fn(x[cand], None, "nngp", as_numpy=False)
        idx, _, _ = greedy_on_device(_lib.load(), k, m, 0.0, want_gains=False)
        picks = idx.cpu().numpy()
    else:
        picks = greedy_rows(np.asarray(kernel_fn(x[cand], None, "nngp"), dtype=np.float64), m)
    return cand[picks]


def sparse_mse_ensemble(kernel_fn, x_train, y_train, m: int, diag_reg: float = 1e-3, select: str = "greedy",
                        chunk_rows: int = 8192, jitter: float = 1e-8, candidates: int = 16384, seed: int = 10,
                        diag_reg_absolute_scale: bool = False):
    """The sparse counterpart of ``predict.gradient_descent_mse_ensemble``: a ``predict_fn(x_test=, get="nngp", compute_cov=)``
    over a ``SparseGPModel`` fitted on all training rows with m inducing rows chosen by ``select_inducing``.  NNGP only.
    ``predict_fn.model_for("nngp")`` is the model, ``predict_fn.inducing`` the chosen indices into x_train."""
    from .predict import Gaussian
    x_train = np.ascontiguousarray(x_train, dtype=np.float64)
    y_train = np.ascontiguousarray(y_train, dtype=np.float64).reshape(x_train.shape[0], -1)
    m = min(int(m), x_train.shape[0])
    inducing = select_inducing(x_train, m, kernel_fn, method=select, candidates=max(int(candidates), m), seed=seed)
    model = SparseGPModel.from_kernel_fn(kernel_fn, m, x_train.shape[1], diag_reg=diag_reg, chunk_rows=chunk_rows, jitter=jitter,
                                         diag_reg_absolute_scale=diag_reg_absolute_scale, ny=y_train.shape[1])
    model.fit(x_train, y_train, x_train[inducing])

    def model_for(get: str = "nngp") -> SparseGPModel:
        if get != "nngp":
            raise ValueError("the sparse model serves the NNGP posterior only, got get = %r" % (get,))
        return model

    def predict_fn(t=None, x_test=None, get="nngp", compute_cov=False):
        if t is not None:
            raise NotImplementedError("only the infinite-time posterior (t=None) is implemented, as the reference uses")
        mdl = model_for(get)
        if compute_cov:
            return Gaussian(*mdl.predict(x_test, cov="diag" if compute_cov == "diag" else "full"))
        return mdl.predict(x_test, cov=None)

    predict_fn.model_for = model_for
    predict_fn.inducing = inducing
    return predict_fn
