"""``--kernel_type gp``: the reference's float64 RBF Gaussian process (train.py:60-150, ``GP_train_and_test``).

The reference trains three hyperparameters -- amplitude, noise and length scale, each ``softplus`` of a raw value --
by ten adaptive gradient steps on the negative log marginal likelihood (NLML), then predicts with them and prints the
q-error profile per ``num_predicates``.  Here the NLML, its analytic gradient and the posterior run in float64 on the
MI355X through ``libnngp_hip.so`` (include/nngp_rbf_gp.h); the update rule stays on the host
(:func:`train_hyperparameters`), where it can be driven by any evaluator.
"""
from __future__ import annotations

import ctypes
import datetime

import numpy as np

from . import _lib
from .util import PredictionStatistics

RAW0 = (0.0, -5.0, 0.0)  # (amplitude, noise, lengthscale) before softplus, train.py:129-131
STEPS = 10
LR = 0.01

_COV = {None: _lib.COV_NONE, False: _lib.COV_NONE, "none": _lib.COV_NONE, "diag": _lib.COV_DIAG,
        True: _lib.COV_FULL, "full": _lib.COV_FULL}


def softplus(x):
    return np.logaddexp(x, 0.)


def train_hyperparameters(evaluate, raw0=RAW0, steps=STEPS, lr=LR, report=print, label="neg marginal likelihood"):
    """The reference's ``train_step`` loop (train.py:136-148) over ``evaluate(raw, with_grad) -> (nlml, grad or None)``.

    Per raw parameter (any number of them; mll.tune_hyperparameters drives it too): ``m = 0.9 m + 0.1 g``, ``s = 0.9 s + 0.1 g^2``, ``p -= lr m / sqrt(s + 1e-5)``, from ``m = 0``
    and ``s = 1`` (the reference's ``scales = p * 0. + 1.``).  After each step the NLML at the new point is reported as
    ``"Step: %d, neg marginal likelihood: %f"``; that point's gradient comes from the same evaluation, so ``steps`` steps
    cost ``steps + 1`` evaluations.  ``label`` names the objective in that line (loo.tune_hyperparameters: ``"LOO nlpd"``).
    Returns the final raw parameters and the list of reported NLMLs."""
    raw = np.array(raw0, dtype=np.float64)
    m = np.zeros_like(raw)
    s = np.ones_like(raw)
    _, g = evaluate(raw, True)
    history = []
    for i in range(steps):
        g = np.asarray(g, dtype=np.float64)
        m = 0.9 * m + 0.1 * g
        s = 0.9 * s + 0.1 * g ** 2
        raw = raw - lr * m / np.sqrt(s + 1e-5)
        nlml, g = evaluate(raw, i + 1 < steps)
        history.append(nlml)
        if report is not None:
            report("Step: %%d, %s: %%f" % label % (i, nlml))
    return raw, history


class F64Handle:
    """create / close / set_train / factor of a float64 evidence handle on the GPU (``<prefix>create`` ... of the C ABI: the RBF
    GP's ``nngp_rbf_gp_`` and the NNGP marginal likelihood's ``nngp_mll_``).  Inputs are numpy or torch arrays; outputs numpy."""

    _prefix = None

    def __init__(self, d: int, *create_args):
        self.lib = _lib.load()
        self.device = _lib.require_gpu()
        self.d = int(d)
        self._h = ctypes.c_void_p()
        self._check(self._fn("create")(ctypes.byref(self._h), *create_args))
        self.n = 0

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    def _check(self, rc):
        _lib.check(rc, self.lib)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_train(self, x, y):
        xd = _lib.to_device_f64(x, self.device)
        yd = _lib.to_device_f64(y, self.device)
        if xd.dim() != 2 or xd.shape[1] != self.d:
            raise ValueError("x must be [n, %d]" % self.d)
        ny = 1 if yd.dim() == 1 else yd.shape[1]
        self._check(self._fn("set_train")(self._h, _lib.ptr(xd), _lib.ptr(yd), xd.shape[0], ny, _lib.stream_ptr()))
        self.n = xd.shape[0]
        return self

    def factor(self):
        """The device factor of the last evaluation as a zero-copy torch view [n_padded, ld] (read its lower triangle;
        valid until the next evaluation or close)."""
        from .model import _wrap_device
        p, ld, npad = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._fn("factor_buffer")(self._h, ctypes.byref(p), ctypes.byref(ld), ctypes.byref(npad)))
        return _wrap_device(p.value, npad.value * ld.value, self.device, "<f8").view(npad.value, ld.value)


class RBFGP(F64Handle):
    """Handle of one float64 RBF GP on the GPU (nngp_rbf_gp_*)."""

    _prefix = "nngp_rbf_gp_"

    def __init__(self, n_cap: int, d: int, m_cap: int = 0):
        import torch
        self._torch = torch
        super().__init__(d, int(n_cap), int(m_cap), int(d))

    def evaluate(self, raw, with_grad: bool = True):
        """NLML (and its gradient with respect to the raw parameters) at ``raw`` = (amplitude, noise, lengthscale)."""
        r = (ctypes.c_double * 3)(*[float(v) for v in np.ravel(raw)[:3]])
        nlml = ctypes.c_double()
        g = (ctypes.c_double * 3)()
        self._check(self.lib.nngp_rbf_gp_evaluate(self._h, r, ctypes.byref(nlml), g if with_grad else None, _lib.stream_ptr()))
        return nlml.value, (np.array(g[:], dtype=np.float64) if with_grad else None)

    def terms(self):
        """Reduced sums of the last gradient evaluation (include/nngp_rbf_gp.h, nngp_rbf_gp_terms)."""
        out = (ctypes.c_double * 8)()
        self._check(self.lib.nngp_rbf_gp_terms(self._h, out))
        keys = ("logdet_half", "y_ainv_y", "a_k_a", "tr_ainv_k", "a_kd_a", "tr_ainv_kd", "a_a", "tr_ainv")
        return dict(zip(keys, out[:]))

    def predict(self, x_test, cov="diag"):
        """Posterior mean [M, 1] and, by ``cov`` ('diag' / 'full' / None), the variance [M] or covariance [M, M]."""
        torch = self._torch
        xt = _lib.to_device_f64(x_test, self.device)
        mt = xt.shape[0]
        mode = _COV[cov]
        mean = torch.empty(mt, dtype=torch.float64, device=self.device)
        out = None
        if mode == _lib.COV_DIAG:
            out = torch.empty(mt, dtype=torch.float64, device=self.device)
        elif mode == _lib.COV_FULL:
            out = torch.empty(mt, mt, dtype=torch.float64, device=self.device)
        self._check(self.lib.nngp_rbf_gp_predict(self._h, _lib.ptr(xt), mt, mode, _lib.ptr(mean), _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        return mean.cpu().numpy().reshape(mt, 1), (None if out is None else out.cpu().numpy())


def kernel(x1, x2, ls):
    """K(x1, x2) = exp(-|x1_i / ls - x2_j / ls|^2) on the GPU (nngp_rbf_gp_kernel); x2 None: x1 against itself."""
    import torch
    lib = _lib.load()
    dev = _lib.require_gpu()
    a = _lib.to_device_f64(x1, dev)
    b = None if x2 is None else _lib.to_device_f64(x2, dev)
    n1, d = a.shape
    n2 = n1 if b is None else b.shape[0]
    out = torch.empty(n1, n2, dtype=torch.float64, device=dev)
    _lib.check(lib.nngp_rbf_gp_kernel(_lib.ptr(a), n1, _lib.ptr(b), 0 if b is None else n2, d, float(ls), _lib.ptr(out), n2,
                                      _lib.stream_ptr()), lib)
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy()


def GP_train_and_test(X_train, Y_train, X_test, Y_test, query_infos_train=None, query_infos_test=None, cov="diag",
                      pred_stat=None):
    """train.py:60-150: train the three hyperparameters, predict twice (timed as the reference does), print the
    q-error profile per num_predicates.  The reference forms the full covariance but only its diagonal is used
    (``std``); ``cov='full'`` forms it too."""
    pred_stat = pred_stat or PredictionStatistics()
    X_train = np.asarray(X_train, dtype=np.float64)
    X_test = np.asarray(X_test, dtype=np.float64)
    gp = RBFGP(X_train.shape[0], X_train.shape[1], X_test.shape[0])
    try:
        gp.set_train(X_train, np.asarray(Y_train, dtype=np.float64).reshape(-1, 1))
        raw, history = train_hyperparameters(gp.evaluate)

        start = datetime.datetime.now()
        pred_mean, var = gp.predict(X_test, cov)
        duration = (datetime.datetime.now() - start).total_seconds()
        print('Kernel construction in %s seconds.' % duration)
        start = datetime.datetime.now()
        pred_mean, var = gp.predict(X_test, cov)
        duration = (datetime.datetime.now() - start).total_seconds()
        print('GP Inference in %s seconds.' % duration)
    finally:
        gp.close()
    var_diag = np.diag(var) if cov in (True, "full") else var
    std = np.sqrt(var_diag)
    errors = np.ravel(np.array(pred_mean - np.asarray(Y_test)))
    pred_stat.get_prediction_details(errors, query_infos_test, partition_keys='num_predicates')
    amp, noise, ls = softplus(raw)
    return {"raw": raw, "amplitude": amp, "noise": noise, "lengthscale": ls, "nlml": history,
            "pred_mean": np.ravel(pred_mean), "pred_var": var_diag, "pred_cov": var if cov in (True, "full") else None,
            "pred_std": std, "errors": errors}
