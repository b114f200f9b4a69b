"""ctypes binding of ``libnngp_hip.so`` (C ABI in ``include/nngp_hip.h``).

There is no CPU fallback: every compute entry point raises if the HIP library is missing or no
MI355X is visible.  PyTorch is used only as the owner of device memory and streams.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnngp_hip.so")
KNOBS_LIB_PATH = os.path.join(_HERE, "libnngp_hip_knobs.so")  # same sources + timing knobs; scripts/ and A/B tests only

GET_NNGP, GET_NTK = 1, 2
DTYPE_F32, DTYPE_F64 = 0, 1
COV_NONE, COV_DIAG, COV_FULL = 0, 1, 2
MAX_DENSE = 16

# every symbol include/nngp_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = (
    "nngp_version", "nngp_last_error", "nngp_kernel_build", "nngp_kernel_diag", "nngp_model_create",
    "nngp_model_destroy", "nngp_model_fit", "nngp_model_set_train", "nngp_model_build_rows",
    "nngp_model_factor", "nngp_model_factor_begin", "nngp_model_factor_panel", "nngp_model_factor_update",
    "nngp_model_factor_end", "nngp_model_factor_buffers", "nngp_model_solve", "nngp_model_append", "nngp_model_kernel_buffer", "nngp_model_info",
    "nngp_model_alpha", "nngp_model_predict", "nngp_model_set_refine", "nngp_model_cov_iters", "nngp_model_sweep_estimate", "nngp_model_factor_shift", "nngp_model_prepare_serving", "nngp_potrf_f32", "nngp_gemm_nt_f32",
    "nngp_gemm_nt_h3", "nngp_gemm_nt_f64", "nngp_trsm_rlt_f32", "nngp_model_apply_factor",
    "nngp_model_factor_input_rows", "nngp_model_factor_input_complete", "nngp_model_precond", "nngp_model_matvec_rows", "nngp_model_set_alpha", "nngp_encoder_create", "nngp_encoder_destroy", "nngp_encoder_dim",
    "nngp_encoder_encode", "nngp_comm_unique_id", "nngp_comm_create", "nngp_comm_destroy", "nngp_comm_library",
    "nngp_allgather_rows", "nngp_bcast", "nngp_model_update_timer", "nngp_model_update_timer_read", "nngp_symv_f64",
    "nngp_pool_select", "nngp_model_update_timer_bytes", "nngp_model_factor_update_cols", "nngp_gemm_nt_i8s", "nngp_model_residual_timer", "nngp_model_residual_timer_read", "nngp_model_trsm_timer", "nngp_model_trsm_timer_read", "nngp_model_residual_floor",
    "nngp_trsm_ticket_order", "nngp_trsm_ticket_queues", "nngp_model_reserve", "nngp_alloc_count",
)

# include/nngp_rbf_gp.h: the float64 RBF GP (--kernel_type gp) and the float64 Cholesky; GPU library only (no host build)
GP_ABI_SYMBOLS = (
    "nngp_rbf_gp_create", "nngp_rbf_gp_destroy", "nngp_rbf_gp_set_train", "nngp_rbf_gp_evaluate", "nngp_rbf_gp_terms",
    "nngp_rbf_gp_predict", "nngp_rbf_gp_kernel", "nngp_rbf_gp_factor_buffer", "nngp_potrf_f64",
    "nngp_potrf_dinv_f64", "nngp_trsm_fwd_f64", "nngp_factor_solve_f64",
)


# include/nngp_activations.h: networks with other activations than ReLU; GPU library only (no host build)
ACT_ABI_SYMBOLS = ("nngp_kernel_build_act", "nngp_kernel_diag_act", "nngp_model_create_act")
ACT_RELU, ACT_ABRELU, ACT_ERF = 0, 1, 2
ACTIVATIONS = {"relu": (ACT_RELU, 0), "abrelu": (ACT_ABRELU, 2), "erf": (ACT_ERF, 3)}  # kind: (code, number of parameters)

# include/nngp_mll.h: the NNGP marginal likelihood and its gradient; GPU library only (no host build)
MLL_ABI_SYMBOLS = ("nngp_mll_create", "nngp_mll_destroy", "nngp_mll_set_train", "nngp_mll_evaluate", "nngp_mll_terms",
                   "nngp_mll_factor_buffer")


# include/nngp_loo.h: leave-one-out cross-validation on the nngp_mll handle; GPU library only (no host build)
LOO_ABI_SYMBOLS = ("nngp_mll_loo_evaluate", "nngp_mll_loo_predictions", "nngp_mll_loo_terms")
LOO_NLPD, LOO_MSE = 0, 1

# include/nngp_ard.h: per-feature input relevances on the nngp_mll handle; GPU library only (no host build)
ARD_ABI_SYMBOLS = ("nngp_mll_reserve_ard", "nngp_mll_evaluate_ard", "nngp_mll_loo_evaluate_ard", "nngp_mll_ard_terms")

# include/nngp_additive.h: additive kernels over feature groups; GPU library only (no host build)
ADDITIVE_ABI_SYMBOLS = ("nngp_kernel_build_additive", "nngp_kernel_diag_additive", "nngp_model_create_additive")
MAX_GROUPS = 1024

# include/nngp_additive_mll.h: the additive kernel's evidence and its gradient, term weights included, on the nngp_mll handle
ADDITIVE_MLL_ABI_SYMBOLS = ("nngp_mll_reserve_additive", "nngp_mll_evaluate_additive", "nngp_mll_additive_terms")

# include/nngp_pool.h: batch-aware pool selection (greedy by conditional variance); GPU library only (no host build)
POOL_ABI_SYMBOLS = ("nngp_pool_select_greedy",)

# include/nngp_sparse.h: the sparse (inducing-point, DTC) NNGP posterior and its Gram kernel; GPU library only (no host build)
SPARSE_ABI_SYMBOLS = ("nngp_sparse_create", "nngp_sparse_destroy", "nngp_sparse_set_inducing", "nngp_sparse_add_rows",
                      "nngp_sparse_finish", "nngp_sparse_predict", "nngp_sparse_info", "nngp_syrk_tn_f64")

# include/nngp_sparse_evidence.h: the sparse model's evidence and its gradient, on the nngp_sparse handle; GPU library only
SPARSE_EVIDENCE_ABI_SYMBOLS = ("nngp_sparse_reserve_evidence", "nngp_sparse_set_kernel", "nngp_sparse_evidence",
                               "nngp_sparse_evidence_grad", "nngp_sparse_evidence_terms", "nngp_sparse_adjoint_rect")
# include/nngp_sparse_ard.h: per-feature relevances on the nngp_sparse handle and the evidence's derivative with respect to them
SPARSE_ARD_ABI_SYMBOLS = ("nngp_sparse_reserve_ard", "nngp_sparse_set_relevance", "nngp_sparse_evidence_grad_ard",
                          "nngp_sparse_ard_terms", "nngp_sparse_ard_rect")
# include/nngp_i8s.h: the stand-alone operators of the sliced int8 product (cuts, residual, fused statistics); GPU library only
I8S_ABI_SYMBOLS = ("nngp_i8s_cut_rows", "nngp_i8s_cut_sym", "nngp_i8s_residual")
# include/nngp_matfree.h: the matrix-free exact NNGP posterior and its fused K.V operator; GPU library only (no host build)
MATFREE_ABI_SYMBOLS = ("nngp_matfree_create", "nngp_matfree_destroy", "nngp_matfree_fit", "nngp_matfree_solve",
                       "nngp_matfree_predict", "nngp_matfree_alpha", "nngp_matfree_info", "nngp_kmv_f64")
# include/nngp_matfree_additive.h: the matrix-free model and its operator on the additive kernel over feature groups
MATFREE_ADDITIVE_ABI_SYMBOLS = ("nngp_matfree_create_additive", "nngp_kmv_additive_f64")
BOUND_DTC, BOUND_VFE = 0, 1
BOUNDS = {"dtc": BOUND_DTC, "vfe": BOUND_VFE}


class NngpArch(ctypes.Structure):
    _fields_ = [("n_dense", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("w_std", ctypes.c_double * MAX_DENSE), ("b_std", ctypes.c_double * MAX_DENSE)]


class NngpArchAct(ctypes.Structure):
    _fields_ = [("base", NngpArch), ("act", ctypes.c_int32 * (MAX_DENSE - 1)),
                ("p", (ctypes.c_double * 3) * (MAX_DENSE - 1))]


class NngpGroups(ctypes.Structure):
    _fields_ = [("n_groups", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("begin", ctypes.POINTER(ctypes.c_int32)), ("end", ctypes.POINTER(ctypes.c_int32)),
                ("weight", ctypes.POINTER(ctypes.c_double)), ("full_weight", ctypes.c_double)]


class NngpFitInfo(ctypes.Structure):
    _fields_ = [("reg", ctypes.c_double), ("trace_mean", ctypes.c_double), ("rel_residual", ctypes.c_double),
                ("refine_iters", ctypes.c_int32), ("clamped_pivots", ctypes.c_int32),
                ("n", ctypes.c_int64), ("n_padded", ctypes.c_int64)]


class NngpSparseInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("m", ctypes.c_int64), ("m_padded", ctypes.c_int64), ("chunks", ctypes.c_int64),
                ("sigma2", ctypes.c_double), ("trace_mean", ctypes.c_double), ("jitter_added", ctypes.c_double)]


class NngpMatfreeInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("m", ctypes.c_int64), ("sigma2", ctypes.c_double), ("iterations", ctypes.c_int32),
                ("k_passes", ctypes.c_int32), ("rel_residual", ctypes.c_double), ("converged", ctypes.c_int32),
                ("restarts", ctypes.c_int32)]


class NngpError(RuntimeError):
    pass


_libs = {}


def load(knobs: bool = False):
    """Load libnngp_hip.so (no GPU needed to load; compute calls need one).

    ``knobs=True`` loads libnngp_hip_knobs.so instead -- the same sources built with -DNNGP_TIMING_KNOBS, which adds
    ``nngp_debug_set`` (ablations for scripts/ and the A/B tests; some produce wrong results on purpose).  The product
    library has no such entry point.  NNGP_KNOBS=1 in the environment makes it the default (scripts/ only)."""
    knobs = bool(knobs) or os.environ.get("NNGP_KNOBS", "0") == "1"
    if knobs in _libs:
        return _libs[knobs]
    path = KNOBS_LIB_PATH if knobs else LIB_PATH
    if not os.path.exists(path):
        raise NngpError(
            "%s is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C nngp-src_amd/csrc`; there is no CPU fallback." % (os.path.basename(path), path))
    # torch first: its wheel carries its own libamdhip64 / libhsa-runtime64.  Loaded in that order the library's
    # DT_NEEDED entries resolve to the copies torch already mapped (same SONAME); the other way round the process ends
    # up with two HSA runtimes and the second one reports "no ROCm-capable device" (seen on the GPU box).
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    bind_prototypes(lib, knobs)
    bind_gp_prototypes(lib)
    bind_act_prototypes(lib)
    bind_mll_prototypes(lib)
    bind_loo_prototypes(lib)
    bind_ard_prototypes(lib)
    bind_additive_prototypes(lib)
    bind_additive_mll_prototypes(lib)
    bind_pool_prototypes(lib)
    bind_sparse_prototypes(lib)
    bind_sparse_evidence_prototypes(lib)
    bind_sparse_ard_prototypes(lib)
    bind_i8s_prototypes(lib)
    bind_matfree_prototypes(lib)
    bind_matfree_additive_prototypes(lib)
    _libs[knobs] = lib
    return lib


def bind_prototypes(lib, knobs: bool = False):
    """Argument and result types of every entry point of include/nngp_hip.h on a loaded library.  Also applied by the test
    infrastructure to its host build of the same ABI, so that both sit behind one interface."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    archp = ctypes.POINTER(NngpArch)
    lib.nngp_version.restype = ctypes.c_int
    lib.nngp_last_error.restype = ctypes.c_char_p
    if knobs:
        lib.nngp_debug_set.argtypes = [i32, i32]
        lib.nngp_debug_set.restype = ctypes.c_int
    lib.nngp_kernel_build.argtypes = [vp, i64, vp, i64, i32, archp, i32, vp, vp, i64, i64, i64, vp]
    lib.nngp_kernel_diag.argtypes = [vp, i64, i32, archp, vp, vp, vp]
    lib.nngp_model_create.argtypes = [ctypes.POINTER(vp), i64, i64, i32, i32, archp, i32, dbl, i32]
    lib.nngp_model_destroy.argtypes = [vp]
    lib.nngp_model_fit.argtypes = [vp, vp, vp, i64, vp]
    lib.nngp_model_set_train.argtypes = [vp, vp, vp, i64, vp]
    lib.nngp_model_build_rows.argtypes = [vp, i64, i64, vp]
    lib.nngp_model_factor.argtypes = [vp, vp]
    lib.nngp_model_factor_begin.argtypes = [vp, vp]
    lib.nngp_model_factor_panel.argtypes = [vp, i64, i64, vp]
    lib.nngp_model_factor_update.argtypes = [vp, i64, i64, i64, i64, vp]
    lib.nngp_model_factor_end.argtypes = [vp, vp]
    lib.nngp_model_factor_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(vp)]
    lib.nngp_model_solve.argtypes = [vp, i32, dbl, vp]
    lib.nngp_model_kernel_buffer.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64)]
    lib.nngp_model_info.argtypes = [vp, ctypes.POINTER(NngpFitInfo)]
    lib.nngp_model_alpha.argtypes = [vp, vp, vp]
    lib.nngp_model_predict.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    lib.nngp_encoder_create.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p, i32, i32]
    lib.nngp_encoder_destroy.argtypes = [vp]
    lib.nngp_encoder_dim.argtypes = [vp]
    lib.nngp_encoder_encode.argtypes = [vp, ctypes.c_char_p, i64, i32, vp, vp, i64, ctypes.POINTER(i64)]
    lib.nngp_model_set_refine.argtypes = [vp, i32]
    lib.nngp_model_cov_iters.argtypes = [vp]
    lib.nngp_model_prepare_serving.argtypes = [vp, vp]
    lib.nngp_model_factor_shift.argtypes = [vp]
    lib.nngp_model_factor_shift.restype = ctypes.c_double
    lib.nngp_model_cov_iters.restype = ctypes.c_int
    lib.nngp_model_sweep_estimate.argtypes = [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    lib.nngp_model_append.argtypes = [vp, vp, vp, i64, vp]
    lib.nngp_gemm_nt_f64.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, dbl, dbl, vp]
    lib.nngp_gemm_nt_i8s.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, dbl, dbl, i32, i32, i32, vp]
    lib.nngp_potrf_f32.argtypes = [vp, i64, i64, vp, vp, vp]
    lib.nngp_gemm_nt_f32.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, i64, ctypes.c_float, ctypes.c_float, i32, vp]
    lib.nngp_gemm_nt_h3.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, i64, ctypes.c_float, ctypes.c_float,
                                    ctypes.c_float, i32, vp]
    lib.nngp_trsm_rlt_f32.argtypes = [vp, i64, i64, vp, i64, vp, i64, vp]
    lib.nngp_model_apply_factor.argtypes = [vp, vp, i64, i32, vp]
    lib.nngp_model_factor_input_rows.argtypes = [vp, i64, i64, ctypes.c_double, vp]
    lib.nngp_model_factor_input_complete.argtypes = [vp]
    lib.nngp_model_precond.argtypes = [vp, vp, vp, vp]
    lib.nngp_model_matvec_rows.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.nngp_model_set_alpha.argtypes = [vp, vp, i32, ctypes.c_double, vp]
    lib.nngp_comm_unique_id.argtypes = [vp]
    lib.nngp_comm_create.argtypes = [ctypes.POINTER(vp), vp, i32, i32]
    lib.nngp_comm_destroy.argtypes = [vp]
    lib.nngp_comm_library.restype = ctypes.c_char_p
    lib.nngp_allgather_rows.argtypes = [vp, i64, i64, i32, vp, vp]
    lib.nngp_bcast.argtypes = [vp, i64, i32, i32, vp, vp]
    lib.nngp_symv_f64.argtypes = [vp, i64, i64, vp, vp, dbl, vp]
    lib.nngp_pool_select.argtypes = [vp, i64, i32, vp, i64, i32, ctypes.c_uint64, vp, vp]
    lib.nngp_model_update_timer.argtypes = [vp, i32]
    lib.nngp_model_update_timer_read.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    lib.nngp_model_update_timer_bytes.argtypes = [vp, ctypes.POINTER(dbl)]
    lib.nngp_model_residual_timer.argtypes = [vp, i32]
    lib.nngp_model_residual_floor.argtypes = [vp, ctypes.POINTER(dbl), ctypes.POINTER(i32)]
    lib.nngp_model_residual_timer_read.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(dbl), ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    lib.nngp_model_trsm_timer.argtypes = [vp, i32]
    lib.nngp_model_trsm_timer_read.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    lib.nngp_model_reserve.argtypes = [vp, i64, i32]
    lib.nngp_alloc_count.argtypes = []
    lib.nngp_trsm_ticket_order.argtypes = [i32, i32, i32, i32, i32, i32, vp, i64, ctypes.POINTER(i64)]
    lib.nngp_trsm_ticket_queues.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, i64, ctypes.POINTER(i64)]
    lib.nngp_model_factor_update_cols.argtypes = [vp, i64, i64, ctypes.POINTER(i64), i32, i64, vp]
    for name in ABI_SYMBOLS:
        if name not in ("nngp_last_error", "nngp_model_factor_shift", "nngp_comm_library", "nngp_alloc_count"):
            getattr(lib, name).restype = ctypes.c_int
    lib.nngp_alloc_count.restype = ctypes.c_int64
    return lib


def bind_gp_prototypes(lib):
    """Argument and result types of include/nngp_rbf_gp.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    lib.nngp_rbf_gp_create.argtypes = [ctypes.POINTER(vp), i64, i64, i32]
    lib.nngp_rbf_gp_destroy.argtypes = [vp]
    lib.nngp_rbf_gp_set_train.argtypes = [vp, vp, vp, i64, i32, vp]
    lib.nngp_rbf_gp_evaluate.argtypes = [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl), ctypes.POINTER(dbl), vp]
    lib.nngp_rbf_gp_terms.argtypes = [vp, ctypes.POINTER(dbl)]
    lib.nngp_rbf_gp_predict.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    lib.nngp_rbf_gp_kernel.argtypes = [vp, i64, vp, i64, i32, dbl, vp, i64, vp]
    lib.nngp_rbf_gp_factor_buffer.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.nngp_potrf_f64.argtypes = [vp, i64, i64, vp]
    lib.nngp_potrf_dinv_f64.argtypes = [vp, i64, i64, vp, vp]
    lib.nngp_trsm_fwd_f64.argtypes = [vp, i64, i64, vp, i64, vp, i64, i32, vp]
    lib.nngp_factor_solve_f64.argtypes = [vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp]
    for name in GP_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_act_prototypes(lib):
    """Argument and result types of include/nngp_activations.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    archp = ctypes.POINTER(NngpArchAct)
    lib.nngp_kernel_build_act.argtypes = [vp, i64, vp, i64, i32, archp, i32, vp, vp, i64, i64, i64, vp]
    lib.nngp_kernel_diag_act.argtypes = [vp, i64, i32, archp, vp, vp, vp]
    lib.nngp_model_create_act.argtypes = [ctypes.POINTER(vp), i64, i64, i32, i32, archp, i32, dbl, i32]
    for name in ACT_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_mll_prototypes(lib):
    """Argument and result types of include/nngp_mll.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    lib.nngp_mll_create.argtypes = [ctypes.POINTER(vp), i64, i32]
    lib.nngp_mll_destroy.argtypes = [vp]
    lib.nngp_mll_set_train.argtypes = [vp, vp, vp, i64, i32, vp]
    lib.nngp_mll_evaluate.argtypes = [vp, ctypes.POINTER(NngpArchAct), dbl, i32, ctypes.POINTER(dbl), ctypes.POINTER(dbl), vp]
    lib.nngp_mll_terms.argtypes = [vp, ctypes.POINTER(dbl), i32]
    lib.nngp_mll_factor_buffer.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    for name in MLL_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_loo_prototypes(lib):
    """Argument and result types of include/nngp_loo.h (the HIP library only)."""
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    lib.nngp_mll_loo_evaluate.argtypes = [vp, ctypes.POINTER(NngpArchAct), i32, dbl, i32, i32, ctypes.POINTER(dbl),
                                          ctypes.POINTER(dbl), vp]
    lib.nngp_mll_loo_predictions.argtypes = [vp, vp, vp, vp]
    lib.nngp_mll_loo_terms.argtypes = [vp, ctypes.POINTER(dbl), i32]
    for name in LOO_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_ard_prototypes(lib):
    """Argument and result types of include/nngp_ard.h (the HIP library only)."""
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    pd = ctypes.POINTER(dbl)
    lib.nngp_mll_reserve_ard.argtypes = [vp]
    lib.nngp_mll_evaluate_ard.argtypes = [vp, ctypes.POINTER(NngpArchAct), pd, dbl, i32, pd, pd, pd, vp]
    lib.nngp_mll_loo_evaluate_ard.argtypes = [vp, ctypes.POINTER(NngpArchAct), i32, pd, dbl, i32, i32, pd, pd, pd, vp]
    lib.nngp_mll_ard_terms.argtypes = [vp, pd, i32]
    for name in ARD_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_additive_prototypes(lib):
    """Argument and result types of include/nngp_additive.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    archp, groupsp = ctypes.POINTER(NngpArchAct), ctypes.POINTER(NngpGroups)
    lib.nngp_kernel_build_additive.argtypes = [vp, i64, vp, i64, i32, archp, groupsp, i32, vp, vp, i64, i64, i64, vp]
    lib.nngp_kernel_diag_additive.argtypes = [vp, i64, i32, archp, groupsp, vp, vp, vp]
    lib.nngp_model_create_additive.argtypes = [ctypes.POINTER(vp), i64, i64, i32, i32, archp, groupsp, i32, dbl, i32]
    for name in ADDITIVE_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_additive_mll_prototypes(lib):
    """Argument and result types of include/nngp_additive_mll.h (the HIP library only)."""
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    pd = ctypes.POINTER(dbl)
    lib.nngp_mll_reserve_additive.argtypes = [vp, ctypes.POINTER(NngpGroups)]
    lib.nngp_mll_evaluate_additive.argtypes = [vp, ctypes.POINTER(NngpArchAct), pd, dbl, i32, pd, pd, pd, vp]
    lib.nngp_mll_additive_terms.argtypes = [vp, pd, i32]
    for name in ADDITIVE_MLL_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_pool_prototypes(lib):
    """Argument and result types of include/nngp_pool.h (the HIP library only)."""
    vp, i64, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    lib.nngp_pool_select_greedy.argtypes = [vp, i64, i64, dbl, i64, vp, vp, vp, i64, vp]
    for name in POOL_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_sparse_prototypes(lib):
    """Argument and result types of include/nngp_sparse.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    lib.nngp_sparse_create.argtypes = [ctypes.POINTER(vp), i64, i64, i64, i32, i32, ctypes.POINTER(NngpArchAct),
                                       ctypes.POINTER(NngpGroups), dbl, i32, dbl]
    lib.nngp_sparse_destroy.argtypes = [vp]
    lib.nngp_sparse_set_inducing.argtypes = [vp, vp, i64, vp]
    lib.nngp_sparse_add_rows.argtypes = [vp, vp, vp, i64, vp]
    lib.nngp_sparse_finish.argtypes = [vp, vp]
    lib.nngp_sparse_predict.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    lib.nngp_sparse_info.argtypes = [vp, ctypes.POINTER(NngpSparseInfo)]
    lib.nngp_syrk_tn_f64.argtypes = [vp, i64, vp, vp, i64, vp, i64, i64, i32, dbl, vp]
    for name in SPARSE_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_sparse_evidence_prototypes(lib):
    """Argument and result types of include/nngp_sparse_evidence.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    pd, archp = ctypes.POINTER(dbl), ctypes.POINTER(NngpArchAct)
    lib.nngp_sparse_reserve_evidence.argtypes = [vp]
    lib.nngp_sparse_set_kernel.argtypes = [vp, archp, dbl, i32]
    lib.nngp_sparse_evidence.argtypes = [vp, i32, pd, vp]
    lib.nngp_sparse_evidence_grad.argtypes = [vp, vp, vp, i64, i32, pd, pd, vp]
    lib.nngp_sparse_evidence_terms.argtypes = [vp, pd, i32]
    lib.nngp_sparse_adjoint_rect.argtypes = [vp, i64, vp, i64, i32, archp, vp, i64, vp, vp, pd, vp]
    for name in SPARSE_EVIDENCE_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_sparse_ard_prototypes(lib):
    """Argument and result types of include/nngp_sparse_ard.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    pd, archp = ctypes.POINTER(dbl), ctypes.POINTER(NngpArchAct)
    lib.nngp_sparse_reserve_ard.argtypes = [vp]
    lib.nngp_sparse_set_relevance.argtypes = [vp, pd]
    lib.nngp_sparse_evidence_grad_ard.argtypes = [vp, vp, vp, i64, i32, pd, pd, pd, vp]
    lib.nngp_sparse_ard_terms.argtypes = [vp, pd, i32]
    lib.nngp_sparse_ard_rect.argtypes = [vp, i64, vp, i64, i32, archp, pd, vp, i64, vp, vp, pd, vp]
    for name in SPARSE_ARD_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_matfree_prototypes(lib):
    """Argument and result types of include/nngp_matfree.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    archp = ctypes.POINTER(NngpArchAct)
    lib.nngp_matfree_create.argtypes = [ctypes.POINTER(vp), i64, i64, i64, i64, i32, i32, archp, ctypes.POINTER(NngpGroups), i32, dbl,
                                        i32, dbl]
    lib.nngp_matfree_destroy.argtypes = [vp]
    lib.nngp_matfree_fit.argtypes = [vp, vp, vp, i64, vp, i64, dbl, i32, vp]
    lib.nngp_matfree_solve.argtypes = [vp, vp, i64, i32, vp, i64, dbl, i32, vp]
    lib.nngp_matfree_predict.argtypes = [vp, vp, i64, i32, vp, vp, dbl, i32, vp]
    lib.nngp_matfree_alpha.argtypes = [vp, vp, vp]
    lib.nngp_matfree_info.argtypes = [vp, ctypes.POINTER(NngpMatfreeInfo)]
    lib.nngp_kmv_f64.argtypes = [vp, i64, vp, i64, i32, vp, i64, i32, archp, dbl, vp]
    for name in MATFREE_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_matfree_additive_prototypes(lib):
    """Argument and result types of include/nngp_matfree_additive.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    archp, groupsp = ctypes.POINTER(NngpArchAct), ctypes.POINTER(NngpGroups)
    lib.nngp_matfree_create_additive.argtypes = [ctypes.POINTER(vp), i64, i64, i64, i64, i32, i32, archp, groupsp, dbl, i32, dbl]
    lib.nngp_kmv_additive_f64.argtypes = [vp, i64, vp, i64, i32, vp, i64, i32, archp, groupsp, dbl, vp]
    for name in MATFREE_ADDITIVE_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def bind_i8s_prototypes(lib):
    """Argument and result types of include/nngp_i8s.h (the HIP library only)."""
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    lib.nngp_i8s_cut_rows.argtypes = [vp, i64, i64, i64, i32, vp, vp, vp, i64, vp, vp]
    lib.nngp_i8s_cut_sym.argtypes = [vp, i64, i64, i32, vp, vp, i64, i32, vp, vp]
    lib.nngp_i8s_residual.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, dbl, dbl, dbl, i32, i32, i32, i32, i32,
                                      vp, vp, vp, vp, vp, vp, vp, vp]
    for name in I8S_ABI_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def check(rc: int, lib=None):
    if rc != 0:
        msg = (lib or load()).nngp_last_error()
        raise NngpError("libnngp_hip: rc=%d: %s" % (rc, (msg or b"").decode("utf-8", "replace")))


def make_arch(w_std, b_std) -> NngpArch:
    w_std = [float(v) for v in w_std]
    b_std = [float(v) for v in b_std]
    if len(w_std) != len(b_std) or not 1 <= len(w_std) <= MAX_DENSE:
        raise ValueError("architecture must have 1..%d Dense layers" % MAX_DENSE)
    arch = NngpArch()
    arch.n_dense = len(w_std)
    for i, (w, b) in enumerate(zip(w_std, b_std)):
        arch.w_std[i] = w
        arch.b_std[i] = b
    return arch


def canonical_activation(spec):
    """One hidden layer's activation as ("relu",), ("abrelu", a, b) or ("erf", a, b, c).  ABRelu(0, 1) is ReLU and becomes
    ("relu",), so that it takes the ReLU kernels and gives their bits."""
    kind = spec[0]
    if kind == "relu":
        return ("relu",)
    if kind == "abrelu" and len(spec) == 3:
        a, b = float(spec[1]), float(spec[2])
        return ("relu",) if (a == 0.0 and b == 1.0) else ("abrelu", a, b)
    if kind == "erf" and len(spec) == 4:
        return ("erf", float(spec[1]), float(spec[2]), float(spec[3]))
    raise ValueError("unknown activation %r" % (spec,))


def all_relu(activations) -> bool:
    return activations is None or all(canonical_activation(a) == ("relu",) for a in activations)


def make_arch_act(w_std, b_std, activations) -> NngpArchAct:
    """nngp_arch_act of Dense layers (w_std, b_std) with activations[l] after Dense layer l (len(w_std) - 1 of them)."""
    arch = NngpArchAct()
    arch.base = make_arch(w_std, b_std)
    activations = list(activations)
    if len(activations) != arch.base.n_dense - 1:
        raise ValueError("%d Dense layers need %d activations, got %d" % (arch.base.n_dense, arch.base.n_dense - 1,
                                                                          len(activations)))
    for l, spec in enumerate(activations):
        spec = canonical_activation(spec)
        arch.act[l] = ACTIVATIONS[spec[0]][0]
        for e, v in enumerate(spec[1:]):
            arch.p[l][e] = v
    return arch


def pair_groups(d: int):
    """The slot pairs of an encoded query: [(0, 2), (2, 4), ..., (d - 2, d)] -- one group per column's (upper, lower)."""
    d = int(d)
    if d < 2 or d % 2 != 0:
        raise ValueError("pair groups need an even number of features >= 2, got d = %d" % d)
    return tuple((i, i + 2) for i in range(0, d, 2))


def check_groups(groups, weights=None, full_weight=1.0, d=None):
    """(groups, weights, full_weight) in canonical form -- tuples of (begin, end) ints and of floats, and a float -- after the
    checks of include/nngp_additive.h: 0 <= begin < end (<= d when d is given), finite weights >= 0, not all of them zero,
    at most MAX_GROUPS groups.  groups = "pairs" needs d.  weights = None: every group has weight 1."""
    if isinstance(groups, str):
        if groups != "pairs":
            raise ValueError("groups must be a list of (begin, end) ranges or 'pairs', got %r" % (groups,))
        if d is None:
            raise ValueError("groups='pairs' needs the number of features")
        groups = pair_groups(d)
    try:
        out = tuple((int(b), int(e)) for b, e in groups)
        if any(float(b) != ib or float(e) != ie for (b, e), (ib, ie) in zip(groups, out)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("groups must be a list of (begin, end) integer ranges, got %r" % (groups,)) from None
    if len(out) > MAX_GROUPS:
        raise ValueError("at most %d groups, got %d" % (MAX_GROUPS, len(out)))
    for b, e in out:
        if not (0 <= b < e) or (d is not None and e > int(d)):
            raise ValueError("group range [%d, %d) is outside 0 <= begin < end%s" % (b, e, "" if d is None else " <= d = %d" % int(d)))
    w = (1.0,) * len(out) if weights is None else tuple(float(v) for v in weights)
    if len(w) != len(out):
        raise ValueError("%d groups need %d weights, got %d" % (len(out), len(out), len(w)))
    w0 = float(full_weight)
    if not all(np.isfinite(v) and v >= 0.0 for v in w + (w0,)):
        raise ValueError("group weights and full_weight must be finite and >= 0")
    if w0 == 0.0 and not any(v > 0.0 for v in w):
        raise ValueError("all weights are zero: the additive kernel has no term")
    return out, w, w0


def make_groups(groups, weights, full_weight) -> NngpGroups:
    """nngp_groups of a checked table (check_groups).  The ctypes arrays stay referenced by the result."""
    g = NngpGroups()
    n = len(groups)
    g.n_groups = n
    g._begin = (ctypes.c_int32 * max(n, 1))(*[b for b, _ in groups])
    g._end = (ctypes.c_int32 * max(n, 1))(*[e for _, e in groups])
    g._weight = (ctypes.c_double * max(n, 1))(*weights)
    g.begin = ctypes.cast(g._begin, ctypes.POINTER(ctypes.c_int32))
    g.end = ctypes.cast(g._end, ctypes.POINTER(ctypes.c_int32))
    g.weight = ctypes.cast(g._weight, ctypes.POINTER(ctypes.c_double))
    g.full_weight = float(full_weight)
    return g


def require_gpu():
    """The torch device used for HBM buffers; raises (never falls back) when no GPU is present."""
    import torch
    if not torch.cuda.is_available():
        raise NngpError("no MI355X/ROCm device visible: the NNGP hot path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def to_device_f64(a, device=None):
    """numpy / torch array -> contiguous float64 device tensor."""
    import torch
    device = device or require_gpu()
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())
