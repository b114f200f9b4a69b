"""Matrix-free exact NNGP: the exact posterior without the N x N kernel (``include/nngp_matfree.h``, ``csrc/matfree.hip``).

``GPModel`` stores K twice and pays N^3 / 3; ``SparseGPModel`` leaves the exact posterior.  ``MatrixFreeGPModel`` solves
(K + sigma2 I) alpha = y by preconditioned conjugate gradients: K is applied by a fused kernel that builds it tile by tile and
multiplies it into a block of vectors (``nngp_kmv_f64``), and the sparse model of ``m`` inducing rows is the preconditioner
(m = 0: none).  The footprint is O(N (d + m + rhs_cap)); means and variances are those of the exact model to the solver's
tolerance.  NNGP only, the plain kernel only (no feature groups, no input scale: ``matfree_additive.AdditiveMatrixFreeGPModel``
has them), ``cov`` = None or "diag".
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from .kernel_spec import HasSpec, KernelSpec

M_MAX = 16384
RHS_MAX = 4096


def check_matfree_spec(spec, get="nngp"):
    """ValueError for what the matrix-free model does not cover: the NTK, feature groups and an input scale."""
    if get != "nngp":
        raise ValueError("the matrix-free model solves the NNGP posterior only (the NTK has no GP prior), got get = %r" % (get,))
    if spec.groups is not None:
        raise ValueError("the matrix-free model does not cover the additive kernel over feature groups (groups is set)")
    if spec.input_scale is not None:
        raise ValueError("the matrix-free model does not cover an input_scale (per-feature relevances): scale the rows first")
    return spec


def check_cov(cov):
    """The covariance mode of ``predict``: None / False / "none" or "diag"; the full covariance is refused."""
    if cov in (None, False, "none"):
        return _lib.COV_NONE
    if cov == "diag":
        return _lib.COV_DIAG
    raise ValueError("the matrix-free model gives cov=None or cov='diag' (a full covariance would be M solves against K), got %r" % (cov,))


def check_matfree_arguments(n_cap, m, chunk_rows, rhs_cap, ny, diag_reg, jitter, tol, max_iter):
    """The checks of nngp_matfree_create and of the solver's tolerance, as ValueError."""
    if int(n_cap) < 1:
        raise ValueError("n_cap must be >= 1, got %r" % (n_cap,))
    if not 0 <= int(m) <= M_MAX:
        raise ValueError("m must be in 0 .. %d, got %r" % (M_MAX, m))
    if int(chunk_rows) < 128 or int(chunk_rows) % 128 != 0:
        raise ValueError("chunk_rows must be a positive multiple of 128, got %r" % (chunk_rows,))
    if not 1 <= int(rhs_cap) <= RHS_MAX:
        raise ValueError("rhs_cap must be in 1 .. %d, got %r" % (RHS_MAX, rhs_cap))
    if not 1 <= int(ny) <= 16:
        raise ValueError("ny must be in 1 .. 16, got %r" % (ny,))
    for name, v in (("diag_reg", diag_reg), ("jitter", jitter)):
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
    check_tolerance(tol, max_iter)


def check_tolerance(tol, max_iter):
    if not (math.isfinite(float(tol)) and 0.0 < float(tol) < 1.0):
        raise ValueError("tol must be finite and in (0, 1), got %r" % (tol,))
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1, got %r" % (max_iter,))


class MatrixFreeGPModel(HasSpec):
    """Python owner of one ``nngp_matfree`` handle.  Keyword names follow ``SparseGPModel``."""

    def __init__(self, n_cap: int, d: int, w_std, b_std, m: int = 1024, diag_reg: float = 1e-3, tol: float = 1e-10,
                 max_iter: int = 1000, rhs_cap: int = 64, chunk_rows: int = 8192, jitter: float = 1e-8,
                 diag_reg_absolute_scale: bool = False, ny: int = 1, activations=None, input_scale=None, groups=None,
                 group_weights=None, full_weight=1.0, get: str = "nngp", allow_unconverged: bool = False, knobs: bool = False):
        spec = self._check_spec(KernelSpec(w_std, b_std, activations, input_scale, groups, group_weights, full_weight), get)
        chunk_rows = min(int(chunk_rows), -(-int(n_cap) // 128) * 128) if int(n_cap) >= 1 else int(chunk_rows)
        check_matfree_arguments(n_cap, m, chunk_rows, rhs_cap, ny, diag_reg, jitter, tol, max_iter)
        self.spec = spec.resolve(d)
        self.lib = _lib.load(knobs)
        self.device = _lib.require_gpu()
        self.n_cap, self.d, self.ny, self.m_cap = int(n_cap), int(d), int(ny), min(int(m), int(n_cap))
        self.rhs_cap, self.chunk_rows = int(rhs_cap), int(chunk_rows)
        self.tol, self.max_iter, self.allow_unconverged = float(tol), int(max_iter), bool(allow_unconverged)
        self.kernel_fn = None  # from_kernel_fn keeps it for select_inducing
        self.n = 0
        self.inducing = None
        self.handle = ctypes.c_void_p()
        self._check(self._create(float(diag_reg), int(bool(diag_reg_absolute_scale)), float(jitter)))

    # ---- what a model of another kernel gives anew (matfree_additive.py): the spec's check, the create call, the rows' scale and
    # the kernel_fn that chooses inducing rows when from_kernel_fn kept none ----
    _check_spec = staticmethod(check_matfree_spec)

    def _create(self, diag_reg, absolute, jitter):
        return self.lib.nngp_matfree_create(ctypes.byref(self.handle), self.n_cap, self.m_cap, self.chunk_rows, self.rhs_cap, self.d,
                                            self.ny, ctypes.byref(self.spec.arch_act()), None, _lib.GET_NNGP, diag_reg, absolute,
                                            jitter)

    def _scaled(self, xd):
        return xd  # this model takes no input_scale

    def _spec_kernel_fn(self):
        from . import mll
        return mll.rebuild_kernel_fn(list(self.spec.w_std), list(self.spec.b_std), self.spec.activations)

    @classmethod
    def from_kernel_fn(cls, kernel_fn, n_cap: int, d: int, **kwargs):
        """The model of a ``stax`` kernel_fn (or a batch() wrapper of one, or a KernelSpec)."""
        model = cls(n_cap, d, **KernelSpec.of(kernel_fn).as_keywords(), **kwargs)
        model.kernel_fn = kernel_fn if callable(kernel_fn) else None
        return model

    def _check(self, rc: int):
        _lib.check(rc, self.lib)

    def _solved(self, rc: int, what: str):
        """rc of fit / solve / predict: 1 (tol not reached within max_iter) raises RuntimeError unless allow_unconverged."""
        if rc == 1:
            info = self.info()
            if self.allow_unconverged:
                return
            raise RuntimeError("%s: the solver stopped after %d iterations at a true relative residual of %.3e, above tol = %.3e "
                               "(raise max_iter, or pass allow_unconverged=True)" % (what, info["iterations"], info["rel_residual"],
                                                                                   self.tol))
        self._check(rc)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.nngp_matfree_destroy(self.handle)
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

    def _select(self, x):
        kernel_fn = self.kernel_fn
        if kernel_fn is None:
            kernel_fn = self._spec_kernel_fn()
        from .sparse import select_inducing
        return select_inducing(np.asarray(x, dtype=np.float64), min(self.m_cap, int(x.shape[0])), kernel_fn, "greedy")

    def fit(self, x, y, inducing=None):
        """x [n, d], y [n] or [n, ny].  inducing: the rows themselves [m, d], or indices into x; None: ``m`` rows chosen by
        ``sparse.select_inducing(..., "greedy")`` (no rows at all when the model was created with m = 0)."""
        import torch
        n = self._rows(x, "x")
        if not 1 <= n <= self.n_cap:
            raise ValueError("the model was created for 1..%d training rows, got %d" % (self.n_cap, n))
        if inducing is None and self.m_cap > 0:
            inducing = self._select(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
        u = None
        if inducing is not None:
            inducing = inducing if hasattr(inducing, "dtype") else np.asarray(inducing)
            if inducing.ndim == 1:
                self.inducing = np.asarray(inducing, dtype=np.int64)
                inducing = x[torch.as_tensor(self.inducing, device=x.device)] if isinstance(x, torch.Tensor) else x[self.inducing]
            if int(inducing.shape[0]) > 0:
                if self._rows(inducing, "inducing rows") > self.m_cap:
                    raise ValueError("the model was created for up to %d inducing rows, got %d" % (self.m_cap, int(inducing.shape[0])))
                u = self._scaled(_lib.to_device_f64(inducing, self.device))
        xd = self._scaled(_lib.to_device_f64(x, self.device))
        yd = _lib.to_device_f64(y, self.device).reshape(n, -1)
        if int(yd.shape[1]) != self.ny:
            raise ValueError("y must have %d column(s), got %s" % (self.ny, tuple(yd.shape)))
        self.n = 0
        rc = self.lib.nngp_matfree_fit(self.handle, _lib.ptr(xd), _lib.ptr(yd.contiguous()), n, _lib.ptr(u),
                                       0 if u is None else int(u.shape[0]), self.tol, self.max_iter, _lib.stream_ptr())
        if rc >= 0:
            self.n = n
        self._solved(rc, "fit")
        return self

    def alpha(self, as_numpy=True):
        """alpha = (K + sigma2 I)^-1 y, [n, ny]."""
        import torch
        out = torch.empty((self.n, self.ny), dtype=torch.float64, device=self.device)
        self._check(self.lib.nngp_matfree_alpha(self.handle, _lib.ptr(out), _lib.stream_ptr()))
        return out.cpu().numpy() if as_numpy else out

    def solve(self, b, as_numpy=True):
        """(K + sigma2 I)^-1 applied to the rows of b [r, n] (RHS-major: one right-hand side per row), r <= rhs_cap."""
        import torch
        bd = _lib.to_device_f64(b, self.device)
        if bd.ndim != 2 or int(bd.shape[1]) != self.n or not 1 <= int(bd.shape[0]) <= self.rhs_cap:
            raise ValueError("b must be [r, %d] with 1 <= r <= rhs_cap = %d, got %s" % (self.n, self.rhs_cap, tuple(bd.shape)))
        out = torch.empty_like(bd)
        rc = self.lib.nngp_matfree_solve(self.handle, _lib.ptr(bd), self.n, int(bd.shape[0]), _lib.ptr(out), self.n, self.tol,
                                         self.max_iter, _lib.stream_ptr())
        self._solved(rc, "solve")
        return out.cpu().numpy() if as_numpy else out

    def predict(self, x_test, cov="diag", as_numpy=True):
        """mean [M, ny] (+ var [M] for cov='diag'): the latent function's, as in the exact model."""
        import torch
        mode = check_cov(cov)
        xt = self._scaled(_lib.to_device_f64(x_test, self.device))
        mt = self._rows(xt, "x_test")
        mean = torch.empty((mt, self.ny), dtype=torch.float64, device=self.device)
        var = torch.empty((mt,), dtype=torch.float64, device=self.device) if mode == _lib.COV_DIAG else None
        if mt > 0:
            rc = self.lib.nngp_matfree_predict(self.handle, _lib.ptr(xt), mt, mode, _lib.ptr(mean), _lib.ptr(var), self.tol,
                                               self.max_iter, _lib.stream_ptr())  # waits for the stream
            self._solved(rc, "predict")
        if as_numpy:
            mean = mean.cpu().numpy()
            var = None if var is None else var.cpu().numpy()
        return mean if var is None else (mean, var)

    def info(self) -> dict:
        fi = _lib.NngpMatfreeInfo()
        self._check(self.lib.nngp_matfree_info(self.handle, ctypes.byref(fi)))
        out = {k: getattr(fi, k) for k, _ in fi._fields_}
        out["converged"] = bool(out["converged"])
        return out


def matfree_mse_ensemble(kernel_fn, x_train, y_train, m: int, diag_reg: float = 1e-3, tol: float = 1e-10, max_iter: int = 1000,
                         rhs_cap: int = 64, chunk_rows: int = 8192, jitter: float = 1e-8, diag_reg_absolute_scale: bool = False,
                         allow_unconverged: bool = False, model_class=None):
    """The matrix-free counterpart of ``sparse.sparse_mse_ensemble``: a ``predict_fn(x_test=, get="nngp", compute_cov=)`` over a
    ``MatrixFreeGPModel`` fitted on all training rows with m greedy inducing rows as preconditioner.  NNGP only; compute_cov may
    be False or "diag".  ``predict_fn.model_for("nngp")`` is the model, ``predict_fn.inducing`` the chosen indices.
    ``model_class``: the model to fit, MatrixFreeGPModel (the default) or a subclass of it."""
    from .predict import Gaussian
    x_train = np.ascontiguousarray(x_train, dtype=np.float64)
    y_train = np.ascontiguousarray(y_train, dtype=np.float64).reshape(x_train.shape[0], -1)
    model = (model_class or MatrixFreeGPModel).from_kernel_fn(
        kernel_fn, x_train.shape[0], x_train.shape[1], m=min(int(m), x_train.shape[0]), diag_reg=diag_reg, tol=tol, max_iter=max_iter,
        rhs_cap=rhs_cap, chunk_rows=chunk_rows, jitter=jitter, diag_reg_absolute_scale=diag_reg_absolute_scale, ny=y_train.shape[1],
        allow_unconverged=allow_unconverged)
    model.fit(x_train, y_train)

    def model_for(get: str = "nngp") -> MatrixFreeGPModel:
        if get != "nngp":
            raise ValueError("the matrix-free model serves the NNGP posterior only, got get = %r" % (get,))
        return model

    def predict_fn(t=None, x_test=None, get="nngp", compute_cov=False):
        if t is not None:
            raise NotImplementedError("only the infinite-time posterior (t=None) is implemented, as the reference uses")
        mdl = model_for(get)
        if compute_cov:
            if compute_cov != "diag":
                raise ValueError("the matrix-free model gives compute_cov=False or 'diag', got %r" % (compute_cov,))
            return Gaussian(*mdl.predict(x_test, cov="diag"))
        return mdl.predict(x_test, cov=None)

    predict_fn.model_for = model_for
    predict_fn.inducing = model.inducing
    return predict_fn
