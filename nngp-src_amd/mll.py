"""Marginal likelihood of the NNGP posterior and hyperparameter tuning on it (include/nngp_mll.h).

neural-tangents users pick ``W_std``, ``b_std`` and ``diag_reg`` by differentiating the GP negative log marginal likelihood
(NLML) through ``kernel_fn`` with JAX autodiff.  Here ``kernel_fn`` is a HIP kernel, so the NLML and its gradient with
respect to every Dense layer's ``sigma_w^2 = W_std^2``, ``sigma_b^2 = b_std^2`` and the regulariser ``lambda`` come from
their own float64 path on the MI355X (``nngp_mll_*``): the kernel build, a float64 Cholesky, and one fused pass that
contracts the adjoint of the layer recursion with ``alpha alpha^T - A^-1``.

    A = K + r I,  r = lambda tr(K) / N  (relative, the default)  or  lambda  (diag_reg_absolute_scale)
    NLML = 1/2 y^T A^-1 y + 1/2 log det A + (N/2) log 2 pi        (y uncentred: the posterior's zero-mean prior)

Only the NNGP posterior (``get='nngp'``) of networks whose hidden layers are Relu, ABRelu, LeakyRelu or Abs is covered:
the NTK ensemble's posterior is not a GP with prior Theta, and Erf layers have no gradient here.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib, stax
from .gp import F64Handle, train_hyperparameters


def _arch_of(kernel_fn_or_params):
    """(w_std, b_std, activations) of a KernelFn (or batch() wrapper of one) or of a (w_std, b_std[, activations]) tuple."""
    if hasattr(kernel_fn_or_params, "w_std"):
        w, b = kernel_fn_or_params.w_std, kernel_fn_or_params.b_std
        acts = getattr(kernel_fn_or_params, "activations", None)
    else:
        w, b = kernel_fn_or_params[0], kernel_fn_or_params[1]
        acts = kernel_fn_or_params[2] if len(kernel_fn_or_params) > 2 else None
    w = [float(v) for v in w]
    b = [float(v) for v in b]
    acts = [("relu",)] * (len(w) - 1) if acts is None else [_lib.canonical_activation(a) for a in acts]
    return w, b, acts


def check_supported(kernel_fn_or_params, get="nngp"):
    """ValueError (no GPU call) for what the marginal likelihood does not cover: the NTK and Erf layers."""
    if get != "nngp":
        raise ValueError("the marginal likelihood is that of the NNGP posterior (get='nngp'); the NTK ensemble posterior "
                         "is not a GP with prior Theta, got get=%r" % (get,))
    w, b, acts = _arch_of(kernel_fn_or_params)
    for l, a in enumerate(acts):
        if a[0] == "erf":
            raise ValueError("hidden layer %d is Erf: the marginal-likelihood gradient covers Relu, ABRelu, LeakyRelu and "
                             "Abs only" % l)
    return w, b, acts


class NNGPMarginalLikelihood(F64Handle):
    """Handle of one float64 NNGP evidence evaluator on the GPU (nngp_mll_*)."""

    _prefix = "nngp_mll_"

    def __init__(self, n_cap: int, d: int):
        super().__init__(d, int(n_cap), int(d))
        self.n_dense = 0

    def evaluate(self, kernel_fn_or_params, diag_reg=1e-3, absolute=False, with_grad=True):
        """(nlml, grad) at the architecture of ``kernel_fn_or_params``.  grad (numpy, 2 n_dense + 1 values): d/dsigma_w,l^2,
        d/dsigma_b,l^2 for every Dense layer l, then d/dlambda; None without ``with_grad``."""
        w, b, acts = _arch_of(kernel_fn_or_params)
        arch = _lib.make_arch_act(w, b, acts)
        nlml = ctypes.c_double()
        g = (ctypes.c_double * (2 * len(w) + 1))()
        self._check(self.lib.nngp_mll_evaluate(self._h, ctypes.byref(arch), float(diag_reg), int(bool(absolute)),
                                               ctypes.byref(nlml), g if with_grad else None, _lib.stream_ptr()))
        self.n_dense = len(w)
        return nlml.value, (np.array(g[:], dtype=np.float64) if with_grad else None)

    def terms(self):
        """The cancelling halves of the last gradient (include/nngp_mll.h, nngp_mll_terms): ``quad[p]`` = alpha^T dA_p alpha,
        ``trace[p]`` = tr(A^-1 dA_p), and the scalar sums."""
        nc = 2 * self.n_dense
        count = 2 * (nc + 1) + 5 + nc
        out = (ctypes.c_double * count)()
        self._check(self.lib.nngp_mll_terms(self._h, out, count))
        v = np.array(out[:], dtype=np.float64)
        t = v[2 * (nc + 1):]
        return {"quad": v[0:2 * (nc + 1):2], "trace": v[1:2 * (nc + 1):2], "logdet_half": t[0], "y_ainv_y": t[1],
                "tr_k": t[2], "a_a": t[3], "tr_ainv": t[4], "tr_dk": t[5:5 + nc]}


def _grad_dict(g, n_dense):
    return {"w_std2": [float(v) for v in g[0:2 * n_dense:2]], "b_std2": [float(v) for v in g[1:2 * n_dense:2]],
            "diag_reg": float(g[2 * n_dense])}


def _train_arrays(x_train, y_train):
    x = np.ascontiguousarray(x_train, dtype=np.float64)
    y = np.asarray(y_train, dtype=np.float64)
    if y.ndim == 2 and y.shape[1] != 1:
        raise ValueError("the marginal likelihood takes one output column, y_train has %d" % y.shape[1])
    y = np.ascontiguousarray(y.reshape(-1))
    if x.ndim != 2 or x.shape[0] != y.shape[0]:
        raise ValueError("x_train must be [N, d] with one y per row")
    return x, y


def marginal_likelihood(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, with_grad=True):
    """NLML of the NNGP posterior of ``kernel_fn`` on (x_train, y_train); with ``with_grad`` also
    ``{'w_std2': [...], 'b_std2': [...], 'diag_reg': g}``, the derivatives with respect to W_std^2, b_std^2 per Dense layer
    and diag_reg."""
    w, _, _ = check_supported(kernel_fn)
    x, y = _train_arrays(x_train, y_train)
    m = NNGPMarginalLikelihood(x.shape[0], x.shape[1])
    try:
        m.set_train(x, y)
        nlml, g = m.evaluate(kernel_fn, diag_reg, diag_reg_absolute_scale, with_grad)
    finally:
        m.close()
    return (nlml, _grad_dict(g, len(w))) if with_grad else nlml


class _Params:
    """The tuned parameters as log-values: log sigma_w,l^2 for every layer, log sigma_b,l^2 for the free biases, log lambda."""

    def __init__(self, w_std, b_std, diag_reg, b_std_init=None, min_diag_reg=1e-6):
        nd = len(w_std)
        if b_std_init is not None:
            init = [float(b_std_init)] * nd if np.isscalar(b_std_init) else [float(v) for v in b_std_init]
            if len(init) != nd:
                raise ValueError("b_std_init needs one value per Dense layer (%d)" % nd)
            b_std = [b if b > 0.0 else i for b, i in zip(b_std, init)]
        if any(not (w > 0.0) for w in w_std) or any(b < 0.0 for b in b_std) or not diag_reg > 0.0:
            raise ValueError("tuning needs W_std > 0, b_std >= 0 and diag_reg > 0")
        self.nd = nd
        self.free_b = [l for l in range(nd) if b_std[l] > 0.0]
        self.b_fixed = list(b_std)
        self.min_diag_reg = float(min_diag_reg)
        self.raw0 = np.array([math.log(w * w) for w in w_std] + [math.log(b_std[l] ** 2) for l in self.free_b] +
                             [math.log(diag_reg)], dtype=np.float64)

    def unpack(self, raw):
        """(w_std, b_std, diag_reg, clamped) of a raw vector; diag_reg never drops below min_diag_reg."""
        raw = np.asarray(raw, dtype=np.float64)
        w = [math.exp(0.5 * v) for v in raw[:self.nd]]
        b = list(self.b_fixed)
        for e, l in enumerate(self.free_b):
            b[l] = math.exp(0.5 * raw[self.nd + e])
        lam = math.exp(raw[-1])
        clamped = lam < self.min_diag_reg
        return w, b, (self.min_diag_reg if clamped else lam), clamped

    def grad_raw(self, g, raw):
        """d NLML / d raw from the gradient with respect to (sigma_w^2, sigma_b^2, lambda): chain rule through exp."""
        w, b, lam, clamped = self.unpack(raw)
        out = [g[2 * l] * w[l] ** 2 for l in range(self.nd)]
        out += [g[2 * l + 1] * b[l] ** 2 for l in self.free_b]
        out.append(0.0 if clamped else g[2 * self.nd] * lam)
        return np.array(out, dtype=np.float64)


def rebuild_kernel_fn(w_std, b_std, activations):
    """stax.serial(Dense, (act, Dense)*) with these W_std / b_std and activations (widths do not enter the kernel)."""
    layers = []
    for l, (w, b) in enumerate(zip(w_std, b_std)):
        layers.append(stax.Dense(1 if l == len(w_std) - 1 else 512, W_std=w, b_std=b))
        if l < len(w_std) - 1:
            a = _lib.canonical_activation(activations[l])
            layers.append(stax.Relu() if a[0] == "relu" else stax.ABRelu(a[1], a[2]))
    return stax.serial(*layers)[2]


def tune_hyperparameters(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, steps=50, lr=0.05,
                         b_std_init=None, min_diag_reg=1e-6, report=print, evaluator=None):
    """Adaptive gradient steps on the NLML over log sigma_w,l^2, log sigma_b,l^2 and log lambda (the update rule of
    gp.train_hyperparameters, the reference's GP rule).  A layer whose b_std is 0 keeps it unless ``b_std_init`` (a value,
    or one per Dense layer) gives a start; lambda never drops below ``min_diag_reg``.  Reports
    ``"Step: %d, neg marginal likelihood: %f"`` after each step.  Returns ``(kernel_fn_tuned, diag_reg_tuned, history)``:
    a stax.serial kernel_fn with the same activations and the tuned W_std / b_std, ready for
    predict.gradient_descent_mse_ensemble with ``diag_reg=diag_reg_tuned``.  A factorisation that fails raises naming
    the column.  ``evaluator``: an object with ``evaluate(params, diag_reg, absolute, with_grad)`` to use instead of the GPU
    (tests drive the same loop with the NumPy oracle)."""
    w0, b0, acts = check_supported(kernel_fn)
    x, y = _train_arrays(x_train, y_train)
    params = _Params(w0, b0, diag_reg, b_std_init, min_diag_reg)
    own = evaluator is None
    ev = NNGPMarginalLikelihood(x.shape[0], x.shape[1]).set_train(x, y) if own else evaluator
    try:
        def evaluate(raw, with_grad):
            w, b, lam, _ = params.unpack(raw)
            nlml, g = ev.evaluate((w, b, acts), lam, diag_reg_absolute_scale, with_grad)
            return nlml, (params.grad_raw(g, raw) if with_grad else None)

        raw, history = train_hyperparameters(evaluate, params.raw0, steps=steps, lr=lr, report=report)
    finally:
        if own:
            ev.close()
    w, b, lam, _ = params.unpack(raw)
    return rebuild_kernel_fn(w, b, acts), lam, history
