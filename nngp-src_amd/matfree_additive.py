"""Matrix-free exact NNGP on the additive kernel over feature groups (``include/nngp_matfree_additive.h``).

``MatrixFreeGPModel`` (matfree.py) refuses feature groups and an input scale.  ``AdditiveMatrixFreeGPModel`` is that model on
K = w0 K(x, x') + sum_g w_g K(x_g, x'_g): the fused operator runs its additive tile body, the preconditioner is the sparse model
of the summed kernel, the diagonal and the cross block are the grouped ones.  Every CG iteration evaluates one layer map per live
group and entry on top of the plain operator's one, so a pass costs about (G + 1) plain passes: this is the expensive exact model,
for users who tuned group weights (additive_mll.py) or relevances and want the exact posterior past the sizes ``GPModel`` holds.
``input_scale`` needs no kernel: rows are scaled once in float64, as ``GPModel`` does.  NNGP only, ``cov`` = None or "diag".
"""
from __future__ import annotations

import ctypes

from . import _lib
from .matfree import MatrixFreeGPModel, matfree_mse_ensemble


def check_matfree_additive_spec(spec, get="nngp"):
    """ValueError for what the additive matrix-free model does not cover: the NTK."""
    if get != "nngp":
        raise ValueError("the matrix-free model solves the NNGP posterior only (the NTK has no GP prior), got get = %r" % (get,))
    return spec


class AdditiveMatrixFreeGPModel(MatrixFreeGPModel):
    """``MatrixFreeGPModel`` with ``groups`` ("pairs" or (begin, end) ranges), ``group_weights``, ``full_weight`` and
    ``input_scale``.  Without groups the table is the plain one and the handle computes the plain model's bytes."""

    _check_spec = staticmethod(check_matfree_additive_spec)

    def _create(self, diag_reg, absolute, jitter):
        table = self.spec.group_table()
        if table is None:
            table = _lib.make_groups((), (), 1.0)
        return self.lib.nngp_matfree_create_additive(ctypes.byref(self.handle), self.n_cap, self.m_cap, self.chunk_rows, self.rhs_cap,
                                                     self.d, self.ny, ctypes.byref(self.spec.arch_act()), ctypes.byref(table),
                                                     diag_reg, absolute, jitter)

    def _scaled(self, xd):
        return self.spec.scale(xd)

    def _spec_kernel_fn(self):
        kernel_fn = super()._spec_kernel_fn()
        if self.spec.groups is not None:
            kernel_fn = kernel_fn.with_groups(self.spec.groups, self.spec.group_weights, self.spec.full_weight)
        if self.spec.input_scale is not None:
            kernel_fn = kernel_fn.with_input_scale(self.spec.input_scale)
        return kernel_fn


def matfree_additive_mse_ensemble(kernel_fn, x_train, y_train, m: int, **kwargs):
    """``matfree.matfree_mse_ensemble`` over an ``AdditiveMatrixFreeGPModel``: ``kernel_fn`` may carry groups and an input scale, and
    the inducing rows are chosen by ``sparse.select_inducing`` on the same kernel_fn."""
    return matfree_mse_ensemble(kernel_fn, x_train, y_train, m, model_class=AdditiveMatrixFreeGPModel, **kwargs)
