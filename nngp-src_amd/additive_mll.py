"""Marginal likelihood of the additive NNGP kernel over feature groups, and tuning on it (include/nngp_additive_mll.h).

``mll.py`` covers the plain kernel and refuses a ``kernel_fn`` that carries groups.  This module is the evidence of the kernel
such a ``kernel_fn`` fits,

    K = w0 K(x, x') + sum_g w_g K(x_g, x'_g),   A = K + r I,   NLML as in mll.py,

with its gradient with respect to every Dense layer's ``sigma_w^2`` and ``sigma_b^2``, ``lambda`` and every term weight, from
the float64 path of ``mll.py`` with one fused pass that walks the terms tile by tile (``nngp_mll_evaluate_additive``).  A term
of weight 0 is not in K and still gets its derivative: "would adding this group help?".

A common factor on all weights is the last Dense layer's ``sigma_w^2`` and ``sigma_b^2``
(``sum_t w_t dNLML/dw_t = v_last dNLML/dv_last + c_last dNLML/dc_last``), so the tuner holds the last layer's ``W_std`` fixed
while it tunes weights.  Relevances together with groups, the leave-one-out objectives and Erf layers are not covered.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib, mll
from .gp import train_hyperparameters
from .kernel_spec import KernelSpec


def grouped_spec(kernel_fn, d):
    """The spec of a kernel_fn that carries groups, bound to d features; ValueError (no GPU call) for what this evidence does
    not cover: no groups, an input_scale, Erf layers."""
    spec = KernelSpec.of(kernel_fn)
    if spec.groups is None:
        raise ValueError("the additive marginal likelihood needs a kernel_fn with feature groups (stax.additive, "
                         "kernel_fn.with_groups); mll.marginal_likelihood covers the plain kernel")
    if spec.input_scale is not None:
        raise ValueError("relevances (input_scale) together with feature groups are not covered by the additive marginal likelihood")
    mll.check_supported(spec.replace(groups=None, group_weights=None, full_weight=1.0))
    return spec.resolve(d)


def _weights_of(spec):
    return np.array((spec.full_weight,) + tuple(spec.group_weights), dtype=np.float64)


class AdditiveMarginalLikelihood(mll.NNGPMarginalLikelihood):
    """mll.NNGPMarginalLikelihood with a group table reserved on it (nngp_mll_reserve_additive): ``groups`` are (begin, end)
    ranges or "pairs"; the weights come with every evaluation."""

    def __init__(self, n_cap: int, d: int, groups):
        super().__init__(n_cap, d)
        self.groups = _lib.check_groups(groups, d=d)[0]
        self.n_terms = 1 + len(self.groups)
        table = _lib.make_groups(self.groups, (1.0,) * len(self.groups), 1.0)
        self._check(self.lib.nngp_mll_reserve_additive(self._h, ctypes.byref(table)))

    def evaluate(self, kernel_fn_or_params, diag_reg=1e-3, absolute=False, with_grad=True, weights=None):
        """(nlml, grad, grad_w) at the architecture of ``kernel_fn_or_params`` and the term weights ``weights`` (w0, then one
        per group; default: those of a kernel_fn that carries this handle's groups).  grad as mll's (2 n_dense + 1 values),
        grad_w: d/dw_t, 1 + n_groups values; both None without ``with_grad``."""
        spec = KernelSpec.of(kernel_fn_or_params)
        if weights is None:
            if spec.groups is None:
                raise ValueError("weights are needed: the parameters carry no feature groups")
            spec = spec.resolve(self.d)
            if spec.groups != self.groups:
                raise ValueError("the kernel_fn's groups are not the ones reserved on this handle")
            weights = _weights_of(spec)
        wt = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if wt.shape[0] != self.n_terms:
            raise ValueError("weights needs the whole-input weight and one per group (%d values), got %d" % (self.n_terms, wt.shape[0]))
        arch = spec.arch_act()
        nlml = ctypes.c_double()
        g = (ctypes.c_double * (2 * spec.n_dense + 1))()
        gw = (ctypes.c_double * self.n_terms)()
        self._check(self.lib.nngp_mll_evaluate_additive(self._h, ctypes.byref(arch), (ctypes.c_double * self.n_terms)(*wt),
                                                        float(diag_reg), int(bool(absolute)), ctypes.byref(nlml),
                                                        g if with_grad else None, gw if with_grad else None, _lib.stream_ptr()))
        self.n_dense = spec.n_dense
        if not with_grad:
            return nlml.value, None, None
        return nlml.value, np.array(g[:], dtype=np.float64), np.array(gw[:], dtype=np.float64)

    def additive_terms(self):
        """Of the last evaluation with a gradient (nngp_mll_additive_terms): ``half1[t]``, ``half2[t]`` the cancelling halves of
        d/dw_t (grad_w = -half1 / 2 + half2 / 2) and ``tr_k_term[t]`` = tr K^(t)."""
        nt = self.n_terms
        out = (ctypes.c_double * (3 * nt))()
        self._check(self.lib.nngp_mll_additive_terms(self._h, out, 3 * nt))
        v = np.array(out[:], dtype=np.float64)
        return {"half1": v[0:2 * nt:2], "half2": v[1:2 * nt:2], "tr_k_term": v[2 * nt:]}


def marginal_likelihood(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, with_grad=True):
    """NLML of the NNGP posterior of a ``kernel_fn`` that carries groups on (x_train, y_train); with ``with_grad`` also the
    gradient dict of mll.marginal_likelihood with ``'full_weight'`` (d/dw0) and ``'group_weights'`` (d/dw_g per group)."""
    x, y = mll._train_arrays(x_train, y_train)
    spec = grouped_spec(kernel_fn, x.shape[1])
    handle = AdditiveMarginalLikelihood(x.shape[0], x.shape[1], spec.groups)
    try:
        nlml, g, gw = handle.set_train(x, y).evaluate(spec, diag_reg, diag_reg_absolute_scale, with_grad)
    finally:
        handle.close()
    if not with_grad:
        return nlml
    return nlml, dict(mll._grad_dict(g, spec.n_dense), full_weight=float(gw[0]), group_weights=[float(v) for v in gw[1:]])


class _Params:
    """The tuned values as one raw vector: mll._Params' log sigma_w,l^2 and log sigma_b,l^2, then log w_t of the tuned term
    weights, then log lambda.  With ``tune_weights`` the last Dense layer's W_std is held fixed (a common factor on the weights
    is that layer's variances).  A weight that starts at 0 stays 0.  ``tie_groups``: one shared log multiplier for all group
    weights instead of one value each; w0 stays separate."""

    def __init__(self, w_std, b_std, diag_reg, weights, b_std_init=None, min_diag_reg=1e-6, tune_weights=True, tie_groups=False):
        self.layers = mll._Params(w_std, b_std, diag_reg, b_std_init, min_diag_reg)
        self.nd = self.layers.nd
        self.weights0 = np.array(weights, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(self.weights0)) or np.any(self.weights0 < 0.0) or not np.any(self.weights0 > 0.0):
            raise ValueError("tuning needs finite term weights >= 0, not all zero")
        self.fix_last = bool(tune_weights)
        self.log_v_last = math.log(float(w_std[-1]) ** 2)
        self.tie = bool(tune_weights and tie_groups)
        free = [t for t in range(self.weights0.shape[0]) if self.weights0[t] > 0.0] if tune_weights else []
        if self.tie:
            self.free_t = [t for t in free if t == 0]
            self.tied_t = [t for t in free if t > 0]
            log_w = [math.log(self.weights0[0])] * len(self.free_t) + [0.0] * (1 if self.tied_t else 0)
        else:
            self.free_t, self.tied_t = free, []
            log_w = [math.log(self.weights0[t]) for t in free]
        self.n_w = len(log_w)
        lay = self.layers.raw0
        head = np.delete(lay[:-1], self.nd - 1) if self.fix_last else lay[:-1]
        self.raw0 = np.concatenate([head, np.array(log_w, dtype=np.float64), lay[-1:]])

    def _layer_raw(self, raw):
        raw = np.asarray(raw, dtype=np.float64)
        head = raw[:raw.shape[0] - 1 - self.n_w]
        if self.fix_last:
            head = np.insert(head, self.nd - 1, self.log_v_last)
        return np.concatenate([head, raw[-1:]])

    def unpack(self, raw):
        """(w_std, b_std, diag_reg, clamped) as mll._Params.unpack."""
        return self.layers.unpack(self._layer_raw(raw))

    def weights(self, raw):
        """The 1 + n_groups term weights of a raw vector."""
        raw = np.asarray(raw, dtype=np.float64)
        lw = raw[raw.shape[0] - 1 - self.n_w:raw.shape[0] - 1]
        wt = self.weights0.copy()
        for e, t in enumerate(self.free_t):
            wt[t] = math.exp(lw[e])
        if self.tied_t:
            wt[self.tied_t] = self.weights0[self.tied_t] * math.exp(lw[-1])
        return wt

    def grad_raw(self, g, raw, g_w):
        """d NLML / d raw from the gradients with respect to (sigma_w^2, sigma_b^2, lambda) and the term weights: chain rule
        through exp; the tied groups' derivatives add."""
        gl = self.layers.grad_raw(g, self._layer_raw(raw))
        head = np.delete(gl[:-1], self.nd - 1) if self.fix_last else gl[:-1]
        wt = self.weights(raw)
        g_w = np.asarray(g_w, dtype=np.float64)
        gw = [g_w[t] * wt[t] for t in self.free_t]
        if self.tied_t:
            gw.append(float(np.sum(g_w[self.tied_t] * wt[self.tied_t])))
        return np.concatenate([head, np.array(gw, dtype=np.float64), gl[-1:]])


def tune_hyperparameters(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, steps=50, lr=0.05,
                         b_std_init=None, min_diag_reg=1e-6, report=print, tune_weights=True, tie_groups=False, evaluator=None):
    """mll.tune_hyperparameters on the evidence of the additive kernel that ``kernel_fn`` carries: the update rule of
    gp.train_hyperparameters over log sigma_w,l^2, log sigma_b,l^2, log w_t (before log lambda) and log lambda.

    ``tune_weights``: the term weights join the tuned values, from kernel_fn's own as the start, and W_std of the LAST Dense
    layer is held fixed (a common factor on all weights is that layer's variances); a weight that starts at 0 stays 0, as a
    b_std of 0 does.  ``tie_groups``: all groups share one multiplier; w0 stays separate.  ``evaluator``: an object with
    ``evaluate(params, diag_reg, absolute, with_grad, weights=) -> (nlml, grad, grad_w)`` to use instead of the GPU (tests
    drive the same loop with the NumPy oracle).  Returns ``(kernel_fn_tuned, diag_reg_tuned, history)``: the tuned layers
    with ``with_groups(groups, tuned weights, full_weight=tuned w0)``."""
    x, y = mll._train_arrays(x_train, y_train)
    spec = grouped_spec(kernel_fn, x.shape[1])
    acts = list(spec.activations)
    params = _Params(list(spec.w_std), list(spec.b_std), diag_reg, _weights_of(spec), b_std_init, min_diag_reg, tune_weights,
                     tie_groups)
    own = evaluator is None
    ev = AdditiveMarginalLikelihood(x.shape[0], x.shape[1], spec.groups).set_train(x, y) if own else evaluator

    def evaluate(raw, with_grad):
        w, b, lam, _ = params.unpack(raw)
        val, g, g_w = ev.evaluate((w, b, acts), lam, diag_reg_absolute_scale, with_grad, weights=params.weights(raw))
        return val, (params.grad_raw(g, raw, g_w) if with_grad else None)

    try:
        raw, history = train_hyperparameters(evaluate, params.raw0, steps=steps, lr=lr, report=report)
    finally:
        if own:
            ev.close()
    w, b, lam, _ = params.unpack(raw)
    wt = params.weights(raw)
    tuned = mll.rebuild_kernel_fn(w, b, acts).with_groups(spec.groups, [float(v) for v in wt[1:]], full_weight=float(wt[0]))
    return tuned, lam, history
