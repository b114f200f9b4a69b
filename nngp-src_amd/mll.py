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
from .kernel_spec import KernelSpec
from .gp import F64Handle, train_hyperparameters


def _arch_of(kernel_fn_or_params):
    """(w_std, b_std, activations) of a KernelFn (or batch() wrapper of one) or of a (w_std, b_std[, activations]) tuple."""
    spec = KernelSpec.of(kernel_fn_or_params)
    return list(spec.w_std), list(spec.b_std), list(spec.activations)


def reject_groups(kernel_fn_or_params, what):
    """ValueError for a kernel_fn that carries feature groups (stax.additive): the evidence and leave-one-out passes build the
    plain kernel (additive_mll.py has the additive kernel's evidence and its gradient in the group weights)."""
    if KernelSpec.of(kernel_fn_or_params).groups is not None:
        raise ValueError("%s does not cover the additive kernel over feature groups (kernel_fn.groups is set): evaluate or "
                         "tune the plain kernel_fn, then add the groups with kernel_fn.with_groups(...); the marginal likelihood of the "
                         "additive kernel itself, term weights included, is additive_mll.marginal_likelihood / "
                         "additive_mll.tune_hyperparameters" % what)


def check_supported(kernel_fn_or_params, get="nngp"):
    """ValueError (no GPU call) for what the marginal likelihood does not cover: the NTK and Erf layers."""
    if get != "nngp":
        raise ValueError("the marginal likelihood is that of the NNGP posterior (get='nngp'); the NTK ensemble posterior "
                         "is not a GP with prior Theta, got get=%r" % (get,))
    reject_groups(kernel_fn_or_params, "the marginal likelihood")
    w, b, acts = _arch_of(kernel_fn_or_params)
    for l, a in enumerate(acts):
        if a[0] == "erf":
            raise ValueError("hidden layer %d is Erf: the marginal-likelihood gradient covers Relu, ABRelu, LeakyRelu and "
                             "Abs only" % l)
    return w, b, acts


def _reserve_ard(self):
    """Allocate what relevances need (nngp_mll_reserve_ard); nothing is allocated by the evaluations after it."""
    self._check(self.lib.nngp_mll_reserve_ard(self._h))
    return self


def _relevance_arg(self, relevance):
    s = np.ascontiguousarray(relevance, dtype=np.float64).reshape(-1)
    if s.shape[0] != self.d:
        raise ValueError("relevance needs one value per feature (%d), got %d" % (self.d, s.shape[0]))
    return (ctypes.c_double * self.d)(*s)


def _ard_terms(self):
    """Of the last evaluation with relevances and a gradient (nngp_mll_ard_terms): ``half1[k]``, ``half2[k]`` the cancelling
    halves of d/ds_k (the ``quad`` / ``trace`` of terms(), or the ``half1`` / ``half2`` of loo.LeaveOneOut.terms()) and
    ``tr_dk[k]`` = tr dK/ds_k."""
    out = (ctypes.c_double * (3 * self.d))()
    self._check(self.lib.nngp_mll_ard_terms(self._h, out, 3 * self.d))
    v = np.array(out[:], dtype=np.float64)
    return {"half1": v[0:2 * self.d:2], "half2": v[1:2 * self.d:2], "tr_dk": v[2 * self.d:]}


class NNGPMarginalLikelihood(F64Handle):
    """Handle of one float64 NNGP evidence evaluator on the GPU (nngp_mll_*)."""

    _prefix = "nngp_mll_"

    def __init__(self, n_cap: int, d: int, ard: bool = False):
        super().__init__(d, int(n_cap), int(d))
        self.n_dense = 0
        if ard:
            self.reserve_ard()

    def evaluate(self, kernel_fn_or_params, diag_reg=1e-3, absolute=False, with_grad=True, relevance=None):
        """(nlml, grad) at the architecture of ``kernel_fn_or_params``.  grad (numpy, 2 n_dense + 1 values): d/dsigma_w,l^2,
        d/dsigma_b,l^2 for every Dense layer l, then d/dlambda; None without ``with_grad``.  ``relevance`` (d values >= 0, on
        a handle made with ``ard=True``): the evidence of K(x o sqrt(s), x' o sqrt(s)), and a third result, d/ds_k (numpy, d
        values; None without ``with_grad``)."""
        spec = KernelSpec.of(kernel_fn_or_params)
        arch = spec.arch_act()
        nlml = ctypes.c_double()
        g = (ctypes.c_double * (2 * spec.n_dense + 1))()
        if relevance is None:
            self._check(self.lib.nngp_mll_evaluate(self._h, ctypes.byref(arch), float(diag_reg), int(bool(absolute)),
                                                   ctypes.byref(nlml), g if with_grad else None, _lib.stream_ptr()))
            self.n_dense = spec.n_dense
            return nlml.value, (np.array(g[:], dtype=np.float64) if with_grad else None)
        s = self._relevance(relevance)
        gs = (ctypes.c_double * self.d)()
        self._check(self.lib.nngp_mll_evaluate_ard(self._h, ctypes.byref(arch), s, float(diag_reg), int(bool(absolute)),
                                                   ctypes.byref(nlml), g if with_grad else None, gs if with_grad else None,
                                                   _lib.stream_ptr()))
        self.n_dense = spec.n_dense
        if not with_grad:
            return nlml.value, None, None
        return nlml.value, np.array(g[:], dtype=np.float64), np.array(gs[:], dtype=np.float64)

    reserve_ard = _reserve_ard
    _relevance = _relevance_arg
    ard_terms = _ard_terms

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


def relevance_groups(ard_groups, d):
    """One integer label per feature from ``ard_groups``: None (every feature its own), ``"pairs"`` (features 2i and 2i + 1
    share one: the two ends of a column's range) or d labels.  Returns ``(index, n_groups)`` with index[k] in 0 .. n_groups-1,
    groups numbered by first appearance."""
    if ard_groups is None:
        labels = list(range(d))
    elif isinstance(ard_groups, str):
        if ard_groups != "pairs":
            raise ValueError("ard_groups must be None, 'pairs' or one integer label per feature, got %r" % (ard_groups,))
        labels = [k // 2 for k in range(d)]
    else:
        labels = [int(v) for v in ard_groups]
        if len(labels) != d:
            raise ValueError("ard_groups needs one label per feature (%d), got %d" % (d, len(labels)))
    seen = {}
    index = np.array([seen.setdefault(v, len(seen)) for v in labels], dtype=np.int64)
    return index, len(seen)


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


def relevance_of(kernel_fn, d):
    """The relevances input_scale^2 that a kernel_fn carries (None without an input_scale), checked against d features."""
    scale = KernelSpec.of(kernel_fn).input_scale
    if scale is None:
        return None
    if scale.shape[0] != d:
        raise ValueError("input_scale has %d values, x has %d features" % (scale.shape[0], d))
    return scale * scale  # sqrt gives the scale back exactly


def evaluate_once(handle, kernel_fn, x, y, diag_reg, absolute, with_grad, **kw):
    """One evaluation on a fresh handle; a kernel_fn with an input_scale is evaluated at its relevances and its gradient
    dict gets ``'relevance'``, the derivatives with respect to them."""
    try:
        rel = relevance_of(kernel_fn, x.shape[1])
        if rel is not None:
            handle.reserve_ard()
        handle.set_train(x, y)
        if rel is None:
            val, g = handle.evaluate(kernel_fn, diag_reg, absolute, with_grad, **kw)
            gd = _grad_dict(g, len(kernel_fn.w_std)) if with_grad else None
        else:
            val, g, g_s = handle.evaluate(kernel_fn, diag_reg, absolute, with_grad, relevance=rel, **kw)
            gd = dict(_grad_dict(g, len(kernel_fn.w_std)), relevance=[float(v) for v in g_s]) if with_grad else None
    finally:
        handle.close()
    return val, gd


def marginal_likelihood(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, with_grad=True):
    """NLML of the NNGP posterior of ``kernel_fn`` on (x_train, y_train); with ``with_grad`` also
    ``{'w_std2': [...], 'b_std2': [...], 'diag_reg': g}``, the derivatives with respect to W_std^2, b_std^2 per Dense layer
    and diag_reg (and ``'relevance'`` when kernel_fn carries an input_scale)."""
    check_supported(kernel_fn)
    x, y = _train_arrays(x_train, y_train)
    nlml, gd = evaluate_once(NNGPMarginalLikelihood(x.shape[0], x.shape[1]), kernel_fn, x, y, diag_reg, diag_reg_absolute_scale,
                             with_grad)
    return (nlml, gd) if with_grad else nlml


class _Params:
    """The tuned parameters as log-values: log sigma_w,l^2 for every layer, log sigma_b,l^2 for the free biases, log lambda."""

    def __init__(self, w_std, b_std, diag_reg, b_std_init=None, min_diag_reg=1e-6, ard_index=None, relevance_init=None):
        """``ard_index`` (relevance_groups): log s of every group joins the vector, before log lambda, and W_std of Dense layer 0
        is held fixed -- a common factor on s is the same thing as sigma_w,0^2, so tuning both would leave one direction free."""
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
        self.ard_index = None if ard_index is None else np.asarray(ard_index, dtype=np.int64)
        self.w0_fixed = float(w_std[0])
        self.free_w = list(range(nd)) if ard_index is None else list(range(1, nd))
        log_s = []
        if ard_index is not None:
            d, ng = self.ard_index.shape[0], int(self.ard_index.max()) + 1
            s0 = np.ones(d) if relevance_init is None else np.asarray(relevance_init, dtype=np.float64).reshape(-1)
            if s0.shape[0] != d or not np.all(np.isfinite(s0)) or np.any(s0 <= 0.0):
                raise ValueError("relevance_init needs one finite value > 0 per feature (%d)" % d)
            for gidx in range(ng):
                members = s0[self.ard_index == gidx]
                if np.any(members != members[0]):
                    raise ValueError("relevance_init must be equal within a group of ard_groups")
                log_s.append(math.log(members[0]))
        self.n_groups = len(log_s)
        self.raw0 = np.array([math.log(w_std[l] * w_std[l]) for l in self.free_w] + [math.log(b_std[l] ** 2) for l in self.free_b] +
                             log_s + [math.log(diag_reg)], dtype=np.float64)

    def unpack(self, raw):
        """(w_std, b_std, diag_reg, clamped) of a raw vector; diag_reg never drops below min_diag_reg."""
        raw = np.asarray(raw, dtype=np.float64)
        w = [self.w0_fixed] * self.nd
        for e, l in enumerate(self.free_w):
            w[l] = math.exp(0.5 * raw[e])
        b = list(self.b_fixed)
        for e, l in enumerate(self.free_b):
            b[l] = math.exp(0.5 * raw[len(self.free_w) + e])
        lam = math.exp(raw[-1])
        clamped = lam < self.min_diag_reg
        return w, b, (self.min_diag_reg if clamped else lam), clamped

    def relevance(self, raw):
        """The d relevances of a raw vector (None without ARD): exp of each feature's group value."""
        if self.ard_index is None:
            return None
        raw = np.asarray(raw, dtype=np.float64)
        o = len(self.free_w) + len(self.free_b)
        return np.exp(raw[o:o + self.n_groups])[self.ard_index]

    def grad_raw(self, g, raw, g_s=None):
        """d NLML / d raw from the gradient with respect to (sigma_w^2, sigma_b^2, lambda) and, with ARD, the relevances
        (``g_s``, d values; the members of a group add): chain rule through exp."""
        w, b, lam, clamped = self.unpack(raw)
        out = [g[2 * l] * w[l] ** 2 for l in self.free_w]
        out += [g[2 * l + 1] * b[l] ** 2 for l in self.free_b]
        if self.ard_index is not None:
            s = self.relevance(raw)
            out += list(np.bincount(self.ard_index, weights=np.asarray(g_s, dtype=np.float64) * s, minlength=self.n_groups))
        out.append(0.0 if clamped else g[2 * self.nd] * lam)
        return np.array(out, dtype=np.float64)


def rebuild_kernel_fn(w_std, b_std, activations, relevance=None):
    """stax.serial(Dense, (act, Dense)*) with these W_std / b_std and activations (widths do not enter the kernel); with
    ``relevance`` it carries input_scale = sqrt(relevance)."""
    layers = []
    for l, (w, b) in enumerate(zip(w_std, b_std)):
        layers.append(stax.Dense(1 if l == len(w_std) - 1 else 512, W_std=w, b_std=b))
        if l < len(w_std) - 1:
            a = _lib.canonical_activation(activations[l])
            layers.append(stax.Relu() if a[0] == "relu" else stax.ABRelu(a[1], a[2]))
    kernel_fn = stax.serial(*layers)[2]
    return kernel_fn if relevance is None else kernel_fn.with_input_scale(np.sqrt(np.asarray(relevance, dtype=np.float64)))


def split_input_scale(kernel_fn, x, ard, relevance_init):
    """What a tuning run does with kernel_fn.input_scale: ``(x, fixed_scale, relevance_init)``.  With ``ard`` its square is the
    default start of the relevances; without, the rows are scaled by it once and the result carries it on (fixed_scale)."""
    rel = relevance_of(kernel_fn, x.shape[1])
    if rel is None:
        return x, None, relevance_init
    if ard:
        return x, None, (rel if relevance_init is None else relevance_init)
    return x * kernel_fn.input_scale, kernel_fn.input_scale, relevance_init


def finish_kernel_fn(kernel_fn, fixed_scale):
    return kernel_fn if fixed_scale is None else kernel_fn.with_input_scale(fixed_scale)


def tune_loop(params, ev, acts, absolute, steps, lr, report, label="neg marginal likelihood"):
    """gp.train_hyperparameters over ``params`` (_Params) on the evaluator ``ev``; returns (raw, history)."""
    def evaluate(raw, with_grad):
        w, b, lam, _ = params.unpack(raw)
        rel = params.relevance(raw)
        if rel is None:
            val, g = ev.evaluate((w, b, acts), lam, absolute, with_grad)
            return val, (params.grad_raw(g, raw) if with_grad else None)
        val, g, g_s = ev.evaluate((w, b, acts), lam, absolute, with_grad, relevance=rel)
        return val, (params.grad_raw(g, raw, g_s) if with_grad else None)

    return train_hyperparameters(evaluate, params.raw0, steps=steps, lr=lr, report=report, label=label)


def tune_hyperparameters(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, steps=50, lr=0.05,
                         b_std_init=None, min_diag_reg=1e-6, report=print, evaluator=None, ard=False, ard_groups=None,
                         relevance_init=None):
    """Adaptive gradient steps on the NLML over log sigma_w,l^2, log sigma_b,l^2 and log lambda (the update rule of
    gp.train_hyperparameters, the reference's GP rule).  A layer whose b_std is 0 keeps it unless ``b_std_init`` (a value,
    or one per Dense layer) gives a start; lambda never drops below ``min_diag_reg``.  Reports
    ``"Step: %d, neg marginal likelihood: %f"`` after each step.  Returns ``(kernel_fn_tuned, diag_reg_tuned, history)``:
    a stax.serial kernel_fn with the same activations and the tuned W_std / b_std, ready for
    predict.gradient_descent_mse_ensemble with ``diag_reg=diag_reg_tuned``.  A factorisation that fails raises naming
    the column.  ``evaluator``: an object with ``evaluate(params, diag_reg, absolute, with_grad)`` to use instead of the GPU
    (tests drive the same loop with the NumPy oracle).

    ``ard``: one relevance s_k >= 0 per input feature, K(x o sqrt(s), x' o sqrt(s)), joins the tuned values as log s_k
    (start: ``relevance_init``, default the square of kernel_fn.input_scale, else 1).  W_std of Dense layer 0 is
    then held fixed, since a common factor on s is the same thing as sigma_w,0^2.  ``ard_groups``: an integer label per
    feature -- features with one label share one relevance and their gradients add -- or ``"pairs"`` for features 2i and
    2i + 1.  The returned kernel_fn carries ``input_scale = sqrt(s)``; the evaluator then also takes ``relevance=`` and
    returns ``(value, grad, grad_s)``.  Without ``ard`` an input_scale of kernel_fn is kept as it is: the rows are scaled by
    it before the run and the returned kernel_fn carries it."""
    w0, b0, acts = check_supported(kernel_fn)
    x, y = _train_arrays(x_train, y_train)
    x, fixed_scale, relevance_init = split_input_scale(kernel_fn, x, ard, relevance_init)
    index = relevance_groups(ard_groups, x.shape[1])[0] if ard else None
    params = _Params(w0, b0, diag_reg, b_std_init, min_diag_reg, index, relevance_init)
    own = evaluator is None
    ev = NNGPMarginalLikelihood(x.shape[0], x.shape[1], ard=bool(ard)).set_train(x, y) if own else evaluator
    try:
        raw, history = tune_loop(params, ev, acts, diag_reg_absolute_scale, steps, lr, report)
    finally:
        if own:
            ev.close()
    w, b, lam, _ = params.unpack(raw)
    return finish_kernel_fn(rebuild_kernel_fn(w, b, acts, params.relevance(raw)), fixed_scale), lam, history
