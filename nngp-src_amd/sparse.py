"""Sparse NNGP: the inducing-point (DTC) posterior on the device (``include/nngp_sparse.h``, ``csrc/sparse_gp.hip``).

The exact models hold the N x N kernel; ``SparseGPModel`` keeps every label, summarises the inputs by m << N inducing rows and
pays O(N m^2) once and O(m^2) per served query with variance.  Training rows arrive in any number of calls and are uploaded
chunk by chunk, so X never has to fit on the device at once.  ``select_inducing`` chooses the inducing rows: greedy by
conditional variance of the prior kernel (``nngp_pool_select_greedy``), or at random.

The model's evidence and its gradient (``include/nngp_sparse_evidence.h``) tune W_std / b_std / diag_reg at the N the sparse model
is for: ``SparseGPModel.evidence`` / ``evidence_grad``, the evaluator ``SparseEvidence`` and ``tune_hyperparameters``.

Per-feature relevances (ARD, ``include/nngp_sparse_ard.h``): ``SparseGPModel.reserve_evidence_ard`` / ``set_relevance`` put one
s_k >= 0 per input feature on the handle, K(x o sqrt(s), x' o sqrt(s)), and ``evidence_grad(..., ard=True)`` also returns the
evidence's derivative with respect to every s_k, at the same O(N m^2); ``tune_hyperparameters(ard=True)`` tunes them.
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
        self.absolute = bool(diag_reg_absolute_scale)
        self.handle = ctypes.c_void_p()
        self._check(self.spec.sparse_create(self.lib, ctypes.byref(self.handle), self.m_cap, self.chunk_rows, int(test_cap), self.d,
                                            self.ny, float(diag_reg), int(bool(diag_reg_absolute_scale)), float(jitter)))
        self.m = 0
        self.relevance = None  # set_relevance: the handle then scales the raw rows itself

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

    # ---- the evidence (include/nngp_sparse_evidence.h) ----
    def reserve_evidence(self):
        """Allocate what the evidence's gradient needs (nngp_sparse_reserve_evidence); the evidence calls after it allocate nothing."""
        check_evidence_spec(self.spec)
        self._check(self.lib.nngp_sparse_reserve_evidence(self.handle))
        return self

    def set_kernel(self, kernel_fn_or_params, diag_reg, diag_reg_absolute_scale=None):
        """New W_std / b_std / activations (the same number of Dense layers) and diag_reg on this handle, without reallocation.
        Forgets the inducing rows and the training rows: set_inducing, add_rows and finish follow."""
        spec = check_evidence_spec(KernelSpec.of(kernel_fn_or_params))
        if spec.n_dense != self.spec.n_dense:
            raise ValueError("the model was created for %d Dense layers, got %d" % (self.spec.n_dense, spec.n_dense))
        if diag_reg_absolute_scale is not None:
            self.absolute = bool(diag_reg_absolute_scale)
        self._check(self.lib.nngp_sparse_set_kernel(self.handle, ctypes.byref(spec.arch_act()), float(diag_reg), int(self.absolute)))
        self.spec = spec.replace(input_scale=self.spec.input_scale, groups=self.spec.groups, group_weights=self.spec.group_weights,
                                 full_weight=self.spec.full_weight)
        self.m = 0
        return self

    def evidence(self, bound="vfe"):
        """The negative log evidence of the fitted model (after finish; ny = 1): ``"dtc"``, or Titsias' collapsed bound ``"vfe"``."""
        nlml = ctypes.c_double()
        self._check(self.lib.nngp_sparse_evidence(self.handle, bound_code(bound), ctypes.byref(nlml), _lib.stream_ptr()))
        return nlml.value

    # ---- per-feature relevances (include/nngp_sparse_ard.h) ----
    def reserve_evidence_ard(self):
        """reserve_evidence plus what the relevances and their gradient need (nngp_sparse_reserve_ard); repeatable."""
        self.reserve_evidence()
        self._check(self.lib.nngp_sparse_reserve_ard(self.handle))
        return self

    def set_relevance(self, s):
        """One relevance s_k >= 0 per input feature (None: none again): K(x o sqrt(s), x' o sqrt(s)).  Forgets the inducing rows
        and the training rows; from then on every method takes raw rows and the handle scales them.  A model whose spec carries
        an input_scale refuses: one mechanism or the other."""
        if self.spec.input_scale is not None:
            raise ValueError("set_relevance on a model with an input_scale: use one mechanism or the other")
        if s is None:
            self._check(self.lib.nngp_sparse_set_relevance(self.handle, None))
            self.relevance = None
        else:
            s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
            if s.shape[0] != self.d:
                raise ValueError("relevances need one value per feature (%d), got %d" % (self.d, s.shape[0]))
            self._check(self.lib.nngp_sparse_set_relevance(self.handle, s.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
            self.relevance = s.copy()
        self.m = 0
        return self

    def evidence_ard_terms(self):
        """Of the last evidence_grad(ard=True) (nngp_sparse_ard_terms): ``quad[k]``, ``trace[k]`` with grad_s = -quad / 2 + trace / 2
        per feature, ``tr_dkff`` = tr dK_ff/ds_k and ``tr_dkuu`` = tr dK_uu/ds_k."""
        d = self.d
        out = (ctypes.c_double * (4 * d))()
        self._check(self.lib.nngp_sparse_ard_terms(self.handle, out, 4 * d))
        v = np.array(out[:], dtype=np.float64)
        return {"quad": v[0:2 * d:2], "trace": v[1:2 * d:2], "tr_dkff": v[2 * d:3 * d], "tr_dkuu": v[3 * d:4 * d]}

    def evidence_grad(self, x, y, bound="vfe", ard=False):
        """(nlml, grad): x, y are the rows that were added, handed again.  grad (numpy, 2 n_dense + 1 values): d/dsigma_w,l^2,
        d/dsigma_b,l^2 for every Dense layer l, then d/dlambda, with the inducing rows held fixed.  ``ard``: (nlml, grad, grad_s)
        with grad_s (d values) the derivatives with respect to the relevances of set_relevance."""
        code = bound_code(bound)
        xd = _lib.to_device_f64(x, self.device)
        n = self._rows(xd, "x")
        xd = self._device_rows(xd)
        yd = _lib.to_device_f64(y, self.device).reshape(-1)
        if int(yd.shape[0]) != n:
            raise ValueError("y must have one value per row of x (%d), got %s" % (n, tuple(yd.shape)))
        nlml = ctypes.c_double()
        g = (ctypes.c_double * (2 * self.spec.n_dense + 1))()
        if ard:
            gs = (ctypes.c_double * self.d)()
            self._check(self.lib.nngp_sparse_evidence_grad_ard(self.handle, _lib.ptr(xd), _lib.ptr(yd), n, code, ctypes.byref(nlml), g,
                                                               gs, _lib.stream_ptr()))  # synchronises: xd, yd may go
            return nlml.value, np.array(g[:], dtype=np.float64), np.array(gs[:], dtype=np.float64)
        self._check(self.lib.nngp_sparse_evidence_grad(self.handle, _lib.ptr(xd), _lib.ptr(yd), n, code, ctypes.byref(nlml), g,
                                                       _lib.stream_ptr()))  # synchronises: xd, yd may go
        return nlml.value, np.array(g[:], dtype=np.float64)

    def evidence_terms(self):
        """Of the last evidence_grad (nngp_sparse_evidence_terms): ``quad[p]``, ``trace[p]`` with grad = -quad / 2 + trace / 2, and
        the scalar sums."""
        nc = 2 * self.spec.n_dense
        count = 2 * (nc + 1) + 7
        out = (ctypes.c_double * count)()
        self._check(self.lib.nngp_sparse_evidence_terms(self.handle, out, count))
        v = np.array(out[:], dtype=np.float64)
        t = v[2 * (nc + 1):]
        return {"quad": v[0:2 * (nc + 1):2], "trace": v[1:2 * (nc + 1):2], "logdet_half": t[0], "yy_cc": t[1], "tr_kff": t[2],
                "tr_g": t[3], "sigma2": t[4], "tr_binv": t[5], "b_b": t[6]}

    def info(self) -> dict:
        fi = _lib.NngpSparseInfo()
        self._check(self.lib.nngp_sparse_info(self.handle, ctypes.byref(fi)))
        return {k: getattr(fi, k) for k, _ in fi._fields_}


def bound_code(bound):
    if bound not in _lib.BOUNDS:
        raise ValueError("bound must be 'vfe' or 'dtc', got %r" % (bound,))
    return _lib.BOUNDS[bound]


def check_evidence_spec(spec):
    """ValueError for what the sparse evidence does not cover: feature groups and an input_scale."""
    if spec.groups is not None:
        raise ValueError("the sparse evidence does not cover the additive kernel over feature groups (groups is set): "
                         "tune the plain kernel_fn, then add the groups with kernel_fn.with_groups(...)")
    if spec.input_scale is not None:
        raise ValueError("the sparse evidence does not cover an input_scale (per-feature relevances): scale the rows first "
                         "and tune the kernel_fn without it")
    return spec


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


class SparseEvidence:
    """The sparse evidence of (x, y) with fixed inducing rows as an evaluator of ``mll.tune_loop``: every ``evaluate`` runs
    set_kernel -> set_inducing -> add_rows -> finish -> evidence[_grad] on one handle, with the rows kept on the device.
    ``inducing``: the rows themselves [m, d], or indices into x."""

    def __init__(self, x, y, inducing, bound="vfe", chunk_rows: int = 8192, jitter: float = 1e-8, ard: bool = False):
        """``ard``: ``evaluate`` also takes ``relevance=`` (d values) and returns ``(value, grad, grad_s)``, the shape
        ``mll.tune_loop`` expects from an evaluator with relevances; x and the inducing rows are the raw rows."""
        bound_code(bound)
        self.ard = bool(ard)
        x = np.ascontiguousarray(x, dtype=np.float64)
        inducing = np.asarray(inducing)
        if inducing.ndim == 1:
            inducing = x[inducing.astype(np.int64)]
        self.device = _lib.require_gpu()
        self.x, self.u = _lib.to_device_f64(x, self.device), _lib.to_device_f64(inducing, self.device)
        self.y = _lib.to_device_f64(np.asarray(y, dtype=np.float64).reshape(-1), self.device)
        if self.x.ndim != 2 or int(self.x.shape[0]) != int(self.y.shape[0]) or int(self.u.shape[1]) != int(self.x.shape[1]):
            raise ValueError("x must be [N, d] with one y per row and inducing rows of d features")
        self.bound, self.jitter = bound, float(jitter)
        self.chunk_rows = min(int(chunk_rows), -(-int(self.x.shape[0]) // 128) * 128)
        self.model = None

    def evaluate(self, params, diag_reg=1e-3, absolute=False, with_grad=True, relevance=None):
        """(nlml, grad) at ``params`` = a kernel_fn or (w_std, b_std, activations); grad is None without ``with_grad``.  With
        ``relevance`` (an evaluator made with ``ard=True``): (nlml, grad, grad_s) at these relevances."""
        spec = check_evidence_spec(KernelSpec.of(params))
        if relevance is not None and not self.ard:
            raise ValueError("relevance= needs SparseEvidence(..., ard=True)")
        if self.model is None:
            self.model = SparseGPModel(int(self.u.shape[0]), int(self.x.shape[1]), diag_reg=diag_reg, chunk_rows=self.chunk_rows,
                                       jitter=self.jitter, test_cap=128, diag_reg_absolute_scale=absolute,
                                       **spec.as_keywords()).reserve_evidence()
            if self.ard:
                self.model.reserve_evidence_ard()
        self.model.set_kernel(spec, diag_reg, absolute)
        if self.ard:
            self.model.set_relevance(relevance)
        self.model.set_inducing(self.u).add_rows(self.x, self.y).finish()
        if relevance is not None:
            if with_grad:
                return self.model.evidence_grad(self.x, self.y, self.bound, ard=True)
            return self.model.evidence(self.bound), None, None
        if with_grad:
            return self.model.evidence_grad(self.x, self.y, self.bound)
        return self.model.evidence(self.bound), None

    def ard_terms(self):
        return self.model.evidence_ard_terms()

    def terms(self):
        return self.model.evidence_terms()

    def close(self):
        if self.model is not None:
            self.model.close()
            self.model = None


def tune_hyperparameters(kernel_fn, x_train, y_train, m: int, bound: str = "vfe", select: str = "greedy", steps: int = 50,
                         lr: float = 0.05, b_std_init=None, min_diag_reg: float = 1e-6, report=print, evaluator=None,
                         diag_reg: float = 1e-3, diag_reg_absolute_scale: bool = False, chunk_rows: int = 8192,
                         jitter: float = 1e-8, candidates: int = 16384, seed: int = 10, inducing=None, ard: bool = False,
                         ard_groups=None, relevance_init=None):
    """``mll.tune_hyperparameters`` on the sparse evidence: adaptive gradient steps over log sigma_w,l^2, log sigma_b,l^2 and
    log lambda, at O(N m^2) per step instead of O(N^3).  The m inducing rows are chosen once, by ``select_inducing`` with the
    starting kernel (or given as ``inducing``: indices into x_train), and held fixed.  ``bound``: ``"vfe"`` (Titsias' collapsed
    bound) or ``"dtc"``.  Reports ``"Step: %d, neg marginal likelihood: %f"`` after each step.  Returns ``(kernel_fn_tuned,
    diag_reg_tuned, history)``, ready for ``sparse_mse_ensemble``.  ``evaluator``: an object with ``evaluate(params, diag_reg,
    absolute, with_grad)`` to use instead of the GPU (tests drive the same loop with the NumPy reference); it brings its own
    inducing rows.  A kernel_fn with feature groups is refused, and without ``ard`` one with an input_scale.

    ``ard``, ``ard_groups``, ``relevance_init``: as in ``mll.tune_hyperparameters`` -- one relevance s_k >= 0 per input feature
    joins the tuned values as log s_k (start: ``relevance_init``, default the square of kernel_fn.input_scale, else 1), W_std of
    Dense layer 0 is held fixed during the run, ``ard_groups`` ties features (labels, or ``"pairs"``), and the returned kernel_fn
    carries ``input_scale = sqrt(s)``, ready for ``sparse_mse_ensemble``.  The result is normalised: the tuned relevances are
    divided by their geometric mean g and W_std of Dense layer 0 is multiplied by sqrt(g) -- the same kernel, since a common factor
    on s is the same thing as sigma_w,0^2 -- so the returned relevances have geometric mean 1 and compare across runs.  The inducing rows are chosen with the starting kernel (its
    input_scale included) and held fixed as raw rows.  The evaluator then also takes ``relevance=`` and returns
    ``(value, grad, grad_s)``."""
    from . import mll
    bound_code(bound)
    w0, b0, acts = mll.check_supported(kernel_fn)
    spec = KernelSpec.of(kernel_fn)
    check_evidence_spec(spec.replace(input_scale=None) if ard else spec)
    x, y = mll._train_arrays(x_train, y_train)
    if ard:
        x, _, relevance_init = mll.split_input_scale(kernel_fn, x, True, relevance_init)
    index = mll.relevance_groups(ard_groups, x.shape[1])[0] if ard else None
    params = mll._Params(w0, b0, diag_reg, b_std_init, min_diag_reg, index, relevance_init)
    own = evaluator is None
    if own:
        if inducing is None:
            m = min(int(m), x.shape[0])
            inducing = select_inducing(x, m, kernel_fn, method=select, candidates=max(int(candidates), m), seed=seed)
        evaluator = SparseEvidence(x, y, inducing, bound=bound, chunk_rows=chunk_rows, jitter=jitter, ard=bool(ard))
    try:
        raw, history = mll.tune_loop(params, evaluator, acts, diag_reg_absolute_scale, steps, lr, report)
    finally:
        if own:
            evaluator.close()
    w, b, lam, _ = params.unpack(raw)
    rel = params.relevance(raw)
    if rel is not None:
        g = float(np.exp(np.mean(np.log(rel))))
        rel, w = rel / g, [w[0] * math.sqrt(g)] + list(w[1:])
    return mll.rebuild_kernel_fn(w, b, acts, rel), lam, history
