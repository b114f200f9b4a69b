"""Leave-one-out cross-validation of the NNGP posterior (include/nngp_loo.h): LOO predictions, the LOO objectives and
hyperparameter tuning on them.

The LOO residual of a GP at a training query is that query's log2 q-error had it been held out, and it comes in closed form
from the float64 evidence core the marginal likelihood already runs on (Rasmussen & Williams, section 5.4.2):

    A = K + r I,  B = A^-1,  alpha = B y,  b_i = B_ii
    residual r_i = alpha_i / b_i,  mean mu_i = y_i - r_i,  variance s_i = 1 / b_i   (of y_i: the regulariser is the noise)
    mse = mean r_i^2,   nlpd = mean [1/2 log(2 pi s_i) + r_i^2 / (2 s_i)]

``r = lambda tr(K) / N`` (or ``lambda``) keeps its full-data value when a point is left out.  So a user trains on every
query and still gets a q-error profile (``loo_predict``), a calibration check of ``pred_std`` (``nlpd``), and two more
objectives to tune ``W_std`` / ``b_std`` / ``diag_reg`` by (``tune_hyperparameters``).  ``get='ntk'`` gives the LOO means of
kernel ridge regression with Theta and the ``mse`` value: no variance, no ``nlpd``, no gradient.  Erf layers are not covered.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .kernel_spec import KernelSpec
from .gp import F64Handle, train_hyperparameters
from .mll import (_Params, _arch_of, _ard_terms, _relevance_arg, _reserve_ard, _train_arrays, rebuild_kernel_fn,
                  evaluate_once, finish_kernel_fn, reject_groups, relevance_groups, relevance_of, split_input_scale, tune_loop)

OBJECTIVES = {"nlpd": _lib.LOO_NLPD, "mse": _lib.LOO_MSE}
_GET = {"nngp": _lib.GET_NNGP, "ntk": _lib.GET_NTK}


def check_supported(kernel_fn_or_params, get="nngp", objective="mse", with_grad=False):
    """ValueError (no GPU call) for what leave-one-out does not cover: Erf layers, an unknown ``get`` / ``objective``, and for
    the NTK the nlpd objective and every gradient."""
    if get not in _GET:
        raise ValueError("get must be 'nngp' or 'ntk', got %r" % (get,))
    if objective not in OBJECTIVES:
        raise ValueError("objective must be 'nlpd' or 'mse', got %r" % (objective,))
    if get == "ntk" and objective == "nlpd":
        raise ValueError("the NTK mean is kernel ridge regression with Theta: it has no leave-one-out variance, so no nlpd")
    if get == "ntk" and with_grad:
        raise ValueError("no leave-one-out gradient for the NTK (its ensemble posterior is not a GP with prior Theta)")
    reject_groups(kernel_fn_or_params, "leave-one-out")
    w, b, acts = _arch_of(kernel_fn_or_params)
    for l, a in enumerate(acts):
        if a[0] == "erf":
            raise ValueError("hidden layer %d is Erf: leave-one-out covers Relu, ABRelu, LeakyRelu and Abs only" % l)
    return w, b, acts


class LeaveOneOut(F64Handle):
    """Handle of one float64 evaluator on the GPU (the ``nngp_mll_`` handle: it serves the marginal likelihood as well, see
    mll.NNGPMarginalLikelihood) with the leave-one-out entry points."""

    _prefix = "nngp_mll_"

    def __init__(self, n_cap: int, d: int, objective="nlpd", get="nngp", ard: bool = False):
        if objective not in OBJECTIVES or get not in _GET or (get == "ntk" and objective == "nlpd"):
            raise ValueError("objective must be 'nlpd' or 'mse' and get 'nngp' or 'ntk' ('ntk' has no nlpd)")
        super().__init__(d, int(n_cap), int(d))
        self.objective, self.get = objective, get
        self.n_dense = 0
        if ard:
            self.reserve_ard()

    reserve_ard = _reserve_ard
    _relevance = _relevance_arg
    ard_terms = _ard_terms

    def evaluate(self, kernel_fn_or_params, diag_reg=1e-3, absolute=False, with_grad=True, objective=None, get=None,
                 relevance=None):
        """(value, grad) of the objective at the architecture of ``kernel_fn_or_params``; grad as in
        mll.NNGPMarginalLikelihood.evaluate, None without ``with_grad``.  With ``relevance`` (d values >= 0, handle made with
        ``ard=True``): ``(value, grad, grad_s)`` as there."""
        objective, get = objective or self.objective, get or self.get
        w, b, acts = check_supported(kernel_fn_or_params, get, objective, with_grad)
        arch = KernelSpec.of(kernel_fn_or_params).arch_act()
        val = ctypes.c_double()
        g = (ctypes.c_double * (2 * len(w) + 1))()
        if relevance is None:
            self._check(self.lib.nngp_mll_loo_evaluate(self._h, ctypes.byref(arch), _GET[get], float(diag_reg), int(bool(absolute)),
                                                       OBJECTIVES[objective], ctypes.byref(val), g if with_grad else None,
                                                       _lib.stream_ptr()))
        else:
            s = self._relevance(relevance)
            gs = (ctypes.c_double * self.d)()
            self._check(self.lib.nngp_mll_loo_evaluate_ard(self._h, ctypes.byref(arch), _GET[get], s, float(diag_reg),
                                                           int(bool(absolute)), OBJECTIVES[objective], ctypes.byref(val),
                                                           g if with_grad else None, gs if with_grad else None,
                                                           _lib.stream_ptr()))
        self.n_dense = len(w)
        self._last_get = get
        grad = np.array(g[:], dtype=np.float64) if with_grad else None
        if relevance is None:
            return val.value, grad
        return val.value, grad, (np.array(gs[:], dtype=np.float64) if with_grad else None)

    def predictions(self):
        """(mean, var) of the last evaluation, numpy [n]; var is None after an NTK evaluation."""
        import torch
        mean = torch.empty(self.n, dtype=torch.float64, device=self.device)
        var = torch.empty(self.n, dtype=torch.float64, device=self.device) if getattr(self, "_last_get", self.get) == "nngp" else None
        self._check(self.lib.nngp_mll_loo_predictions(self._h, _lib.ptr(mean), _lib.ptr(var), _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        return mean.cpu().numpy(), (None if var is None else var.cpu().numpy())

    def terms(self):
        """The cancelling halves of the last gradient (nngp_mll_loo_terms): ``half1[p]`` = sum 1/2 (alpha_i u_j + u_i alpha_j)
        dA_p,ij, ``half2[p]`` = sum C_ij dA_p,ij, and the scalar sums."""
        nc = 2 * self.n_dense
        count = 2 * (nc + 1) + 3 + nc
        out = (ctypes.c_double * count)()
        self._check(self.lib.nngp_mll_loo_terms(self._h, out, count))
        v = np.array(out[:], dtype=np.float64)
        t = v[2 * (nc + 1):]
        return {"half1": v[0:2 * (nc + 1):2], "half2": v[1:2 * (nc + 1):2], "a_u": t[0], "tr_c": t[1], "tr_k": t[2],
                "tr_dk": t[3:3 + nc]}


def loo_predict(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, get="nngp"):
    """Leave-one-out mean and variance at every training point: ``(mean [N], var [N] or None)``; ``y_train - mean`` are the
    LOO residuals (log2 q-errors when y is log2 of the cardinality).  ``get='ntk'``: the means of kernel ridge regression
    with Theta, var None."""
    check_supported(kernel_fn, get, "mse", False)
    x, y = _train_arrays(x_train, y_train)
    rel = relevance_of(kernel_fn, x.shape[1])
    m = LeaveOneOut(x.shape[0], x.shape[1], "mse", get, ard=rel is not None)
    try:
        m.set_train(x, y)
        m.evaluate(kernel_fn, diag_reg, diag_reg_absolute_scale, with_grad=False, relevance=rel)
        return m.predictions()
    finally:
        m.close()


def loo_objective(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, objective="nlpd", with_grad=True,
                  get="nngp"):
    """The LOO objective (``'nlpd'`` or ``'mse'``, per-query means) of ``kernel_fn`` on (x_train, y_train); with ``with_grad``
    also ``{'w_std2': [...], 'b_std2': [...], 'diag_reg': g}`` as mll.marginal_likelihood returns it."""
    check_supported(kernel_fn, get, objective, with_grad)
    x, y = _train_arrays(x_train, y_train)
    val, gd = evaluate_once(LeaveOneOut(x.shape[0], x.shape[1], objective, get), kernel_fn, x, y, diag_reg,
                            diag_reg_absolute_scale, with_grad)
    return (val, gd) if with_grad else val


def tune_hyperparameters(kernel_fn, x_train, y_train, diag_reg=1e-3, diag_reg_absolute_scale=False, steps=50, lr=0.05,
                         b_std_init=None, min_diag_reg=1e-6, report=print, evaluator=None, objective="nlpd", ard=False,
                         ard_groups=None, relevance_init=None):
    """mll.tune_hyperparameters with a leave-one-out objective in place of the NLML: the same parameters (log sigma_w,l^2,
    log sigma_b,l^2 of the free biases, log lambda and, with ``ard``, log s_k), the same update rule
    (gp.train_hyperparameters) and the same return value ``(kernel_fn_tuned, diag_reg_tuned, history)``.  Reports
    ``"Step: %d, LOO %s: %f"`` after each step.  ``evaluator``: an object with ``evaluate(params, diag_reg, absolute,
    with_grad)`` to use instead of the GPU."""
    w0, b0, acts = check_supported(kernel_fn, "nngp", objective, True)
    x, y = _train_arrays(x_train, y_train)
    x, fixed_scale, relevance_init = split_input_scale(kernel_fn, x, ard, relevance_init)
    index = relevance_groups(ard_groups, x.shape[1])[0] if ard else None
    params = _Params(w0, b0, diag_reg, b_std_init, min_diag_reg, index, relevance_init)
    own = evaluator is None
    ev = LeaveOneOut(x.shape[0], x.shape[1], objective, ard=bool(ard)).set_train(x, y) if own else evaluator
    try:
        raw, history = tune_loop(params, ev, acts, diag_reg_absolute_scale, steps, lr, report, "LOO %s" % objective)
    finally:
        if own:
            ev.close()
    w, b, lam, _ = params.unpack(raw)
    return finish_kernel_fn(rebuild_kernel_fn(w, b, acts, params.relevance(raw)), fixed_scale), lam, history
