"""``python -m nngp_src_amd.train --kernel_type nngp ...`` -- drop-in for the reference driver
(train.py:153-203 ``NNGP_train_and_test``, train.py:224-246 ``main``, flags train.py:252-287).

Prints the same lines as the reference (number of query, shapes, "Kernel construction in ... seconds.",
"Mean Square Error: ...", "Inference time=... seconds", then the q-error profile) with the GP running on
the MI355X through libnngp_hip.so.  ``--kernel_type gp`` runs the reference's float64 RBF GP instead (gp.py).
"""
from __future__ import annotations

import datetime
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

from . import stax, predict as nt_predict
from .batching import batch
from .encoder import FOREST_COLUMNS, GeneralQueryEncoder, TableEncoder
from .util import PredictionStatistics, train_test_val_split

pred_stat = PredictionStatistics()


ACTIVATIONS = ("relu", "erf", "abs", "leaky_relu")


def activation_layer(name: str = "relu", leaky_alpha: float = 0.1):
    """The hidden-layer activation --activation names (every hidden layer gets the same one)."""
    if name == "relu":
        return stax.Relu()
    if name == "erf":
        return stax.Erf()
    if name == "abs":
        return stax.Abs()
    if name == "leaky_relu":
        return stax.LeakyRelu(leaky_alpha)
    raise ValueError("unknown activation %r (one of %s)" % (name, ", ".join(ACTIVATIONS)))


def build_kernel_fn(n_relu: int = 1, activation: str = "relu", leaky_alpha: float = 0.1):
    layers = [stax.Dense(512)]
    for _ in range(n_relu):
        layers += [activation_layer(activation, leaky_alpha), stax.Dense(512)]
    layers[-1] = stax.Dense(1)
    return stax.serial(*layers)


def kernel_fn_from_args(args):
    return build_kernel_fn(getattr(args, "n_relu", 1), getattr(args, "activation", "relu"), getattr(args, "leaky_alpha", 0.1))


def NNGP_train_and_test(args, X_train, Y_train, X_test, Y_test, query_infos_train=None, query_infos_test=None,
                        kernel_fn=None, diag_reg=1e-3):
    def prediction(pred_fn, X_test, kernel_type="nngp", compute_cov=True):
        pred_mean, pred_cov = pred_fn(x_test=X_test, get=kernel_type, compute_cov=compute_cov)
        return pred_mean, pred_cov

    if kernel_fn is None:
        init_fn, apply_fn, kernel_fn = kernel_fn_from_args(args)
    # slot pairs + the whole input; --tune_additive has tuned the kernel with its groups and brings them along
    if getattr(args, "additive", "none") == "pairs" and kernel_fn.groups is None:
        kernel_fn = kernel_fn.with_groups("pairs", full_weight=getattr(args, "additive_full_weight", 1.0))
    # --matrix_free_groups pairs: the same table for the matrix-free model's additive form (matfree_additive.py)
    mf_groups = getattr(args, "matrix_free_groups", "none") == "pairs"
    if mf_groups and kernel_fn.groups is None:
        kernel_fn = kernel_fn.with_groups("pairs", full_weight=getattr(args, "matrix_free_full_weight", 1.0))
    kernel_fn = batch(kernel_fn, device_count=0, batch_size=0)
    start = datetime.datetime.now()
    if (getattr(args, "matrix_free", 0) or 0) > 0:  # --matrix_free M: the exact posterior by PCG, M inducing rows as preconditioner
        from .matfree import matfree_mse_ensemble
        from .matfree_additive import matfree_additive_mse_ensemble
        if args.kernel_type != "nngp":
            raise ValueError("--matrix_free solves the NNGP posterior: it needs --kernel_type nngp")
        ensemble = matfree_additive_mse_ensemble if mf_groups else matfree_mse_ensemble
        predict_fn = ensemble(kernel_fn, X_train, Y_train, args.matrix_free, diag_reg=diag_reg,
                              tol=getattr(args, "matrix_free_tol", 1e-10), max_iter=getattr(args, "matrix_free_iters", 1000),
                              chunk_rows=getattr(args, "sparse_chunk", 8192), jitter=getattr(args, "sparse_jitter", 1e-8))
    elif (getattr(args, "sparse", 0) or 0) > 0:  # --sparse M: every training row, M inducing rows (sparse.py)
        from .sparse import sparse_mse_ensemble
        if args.kernel_type != "nngp":
            raise ValueError("--sparse serves the NNGP posterior: it needs --kernel_type nngp")
        predict_fn = sparse_mse_ensemble(kernel_fn, X_train, Y_train, args.sparse, diag_reg=diag_reg,
                                         select=getattr(args, "sparse_select", "greedy"),
                                         chunk_rows=getattr(args, "sparse_chunk", 8192), jitter=getattr(args, "sparse_jitter", 1e-8))
    else:
        predict_fn = nt_predict.gradient_descent_mse_ensemble(kernel_fn, X_train, Y_train, diag_reg=diag_reg)
    duration = (datetime.datetime.now() - start).total_seconds()
    print('Kernel construction in %s seconds.' % duration)

    cov_mode = True if getattr(args, "full_cov", False) else "diag"
    if (getattr(args, "matrix_free", 0) or 0) > 0 and cov_mode is True:
        raise ValueError("--matrix_free gives variances only: not with --full_cov")
    pred_mean, pred_cov = prediction(predict_fn, X_test, kernel_type=args.kernel_type, compute_cov=cov_mode)
    pred_std = np.sqrt(np.diag(pred_cov)) if cov_mode is True else np.sqrt(pred_cov)

    mse = np.sum(np.power(pred_mean - Y_test, 2))
    print("Mean Square Error: {}".format(mse))

    print(X_test.shape, Y_test.shape)
    start = datetime.datetime.now()
    pred_mean, pred_cov = prediction(predict_fn, X_test, kernel_type=args.kernel_type, compute_cov=cov_mode)
    duration = (datetime.datetime.now() - start).total_seconds()
    print("Inference time={} seconds".format(duration))

    errors = np.ravel(np.array(pred_mean - Y_test))
    pred_stat.get_prediction_details(errors, query_infos_test, partition_keys='num_table')
    res = {"pred_mean": np.ravel(pred_mean), "pred_std": np.ravel(pred_std), "errors": errors, "mse": float(mse),
           "fit_info": predict_fn.model_for(args.kernel_type).info()}
    if getattr(args, "loo", False):
        res.update(loo_profile(args, kernel_fn, X_train, Y_train, query_infos_train, diag_reg))
    return res


def loo_profile(args, kernel_fn, X_train, Y_train, query_infos_train=None, diag_reg=1e-3):
    """--loo: the leave-one-out residuals of the fit over the training split (loo.py) -- every training query predicted as if
    it had been held out -- as "LOO Mean Square Error: ..." (the mean of their squares) and their q-error profile."""
    from . import loo
    loo_mean, loo_var = loo.loo_predict(kernel_fn, X_train, Y_train, diag_reg=diag_reg, get=args.kernel_type)
    loo_errors = loo_mean - np.ravel(np.asarray(Y_train, dtype=np.float64))
    loo_mse = float(np.mean(np.power(loo_errors, 2)))
    print("LOO Mean Square Error: {}".format(loo_mse))
    pred_stat.get_prediction_details(loo_errors, query_infos_train, partition_keys='num_table')
    return {"loo_mean": loo_mean, "loo_var": loo_var, "loo_errors": loo_errors, "loo_mse": loo_mse}


def load_training_data(args):
    """datasets.load_training_data for the single-table case (datasets.py:301-346)."""
    relation = args.relations.split(',')[0].strip()
    if relation != 'forest':
        raise NotImplementedError("only the forest relation ships with column metadata; others need their CSV")
    csv = os.path.join(args.data_path or "", "forest.csv")
    if args.data_path and os.path.exists(csv):
        import pandas as pd
        names = [c.name for c in FOREST_COLUMNS]
        df = pd.read_csv(csv, header=None, usecols=list(range(10)), names=names)
        cols = TableEncoder.from_dataframe(df, ['numerical'] * 10, args.names, args.chunk_size).columns
        loader = GeneralQueryEncoder(cols, args.names, args.chunk_size)
    else:
        loader = GeneralQueryEncoder(FOREST_COLUMNS, args.names, args.chunk_size)
    print("feature dim={}".format(loader.total_feat_dim))
    all_queries, all_cards, all_query_infos = loader.load_queries(args.query_path)
    X, Y = loader.transform_to_arrays(all_queries, all_cards)
    return X, Y, all_query_infos


TUNE_OBJECTIVES = ("mll", "loo_nlpd", "loo_mse")


def tune_kernel_fn(args, X_train, Y_train):
    """--tune_hyper STEPS: W_std / b_std / diag_reg of the NNGP on the training split, by marginal likelihood (mll.py) or, with
    --tune_objective loo_nlpd / loo_mse, by a leave-one-out objective (loo.py)."""
    from . import loo, mll
    _, _, kernel_fn = kernel_fn_from_args(args)
    objective = getattr(args, "tune_objective", "mll")
    if getattr(args, "tune_additive", False):  # --tune_additive: the evidence of the additive kernel itself, its weights tuned too
        from . import additive_mll
        kernel_fn = kernel_fn.with_groups("pairs", full_weight=getattr(args, "additive_full_weight", 1.0))
        kernel_fn, diag_reg, _ = additive_mll.tune_hyperparameters(kernel_fn, X_train, Y_train, diag_reg=1e-3, steps=args.tune_hyper,
                                                                   lr=args.tune_lr, b_std_init=args.b_std_init)
        print("Tuned W_std={} b_std={} diag_reg={}".format(list(kernel_fn.w_std), list(kernel_fn.b_std), diag_reg))
        print("Tuned weights: full={} groups={}".format(kernel_fn.full_weight, list(kernel_fn.group_weights)))
        return kernel_fn, diag_reg
    ard = {}
    if getattr(args, "tune_ard", False):  # --tune_ard: one relevance per input feature joins the tuned values (nngp_ard.h)
        groups = getattr(args, "ard_groups", "none")
        ard = {"ard": True, "ard_groups": None if groups == "none" else groups}
    if objective == "mll":
        kernel_fn, diag_reg, _ = mll.tune_hyperparameters(kernel_fn, X_train, Y_train, diag_reg=1e-3, steps=args.tune_hyper,
                                                          lr=args.tune_lr, b_std_init=args.b_std_init, **ard)
    else:
        kernel_fn, diag_reg, _ = loo.tune_hyperparameters(kernel_fn, X_train, Y_train, diag_reg=1e-3, steps=args.tune_hyper,
                                                          lr=args.tune_lr, b_std_init=args.b_std_init,
                                                          objective=objective[len("loo_"):], **ard)
    print("Tuned W_std={} b_std={} diag_reg={}".format(list(kernel_fn.w_std), list(kernel_fn.b_std), diag_reg))
    if ard:
        print("Tuned relevances={}".format([float(v) for v in kernel_fn.input_scale ** 2]))
    return kernel_fn, diag_reg


def sparse_tune_kernel_fn(args, X_train, Y_train):
    """--sparse_tune STEPS (with --sparse M): W_std / b_std / diag_reg by the sparse model's own evidence (sparse.py), at the N
    the sparse model is for."""
    from . import sparse
    _, _, kernel_fn = kernel_fn_from_args(args)
    ard = {}
    if getattr(args, "sparse_tune_ard", False):  # --sparse_tune_ard: one relevance per input feature joins (nngp_sparse_ard.h)
        groups = getattr(args, "ard_groups", "none")
        ard = {"ard": True, "ard_groups": None if groups == "none" else groups}
    kernel_fn, diag_reg, _ = sparse.tune_hyperparameters(
        kernel_fn, X_train, Y_train, args.sparse, bound=getattr(args, "sparse_bound", "vfe"),
        select=getattr(args, "sparse_select", "greedy"), steps=args.sparse_tune, lr=args.tune_lr, b_std_init=args.b_std_init,
        chunk_rows=getattr(args, "sparse_chunk", 8192), jitter=getattr(args, "sparse_jitter", 1e-8), **ard)
    print("Tuned W_std={} b_std={} diag_reg={}".format(list(kernel_fn.w_std), list(kernel_fn.b_std), diag_reg))
    if ard:
        print("Tuned relevances={}".format([float(v) for v in kernel_fn.input_scale ** 2]))
    return kernel_fn, diag_reg


def main(args):
    tune = getattr(args, "tune_hyper", 0) or 0
    if tune and args.kernel_type != 'nngp':
        raise ValueError("--tune_hyper tunes the NNGP posterior (marginal likelihood or leave-one-out): it needs --kernel_type nngp")
    if args.join_query:
        raise NotImplementedError("join schemas need their benchmark CSVs; use Estimator(encoder=...)")
    X, Y, all_query_infos = load_training_data(args)
    print("number of query: {}".format(X.shape[0]))
    X_train, Y_train, qi_train, X_test, Y_test, qi_test, _, _, _ = train_test_val_split(
        X, Y, train_frac=0.6, test_frac=0.2, all_query_infos=all_query_infos, max_num_train=args.max_num_train)
    if args.max_num_test is not None:
        X_test, Y_test, qi_test = X_test[:args.max_num_test], Y_test[:args.max_num_test], qi_test[:args.max_num_test]
    print(X_train.shape, X_test.shape)
    print(Y_train.shape, Y_test.shape)
    if args.kernel_type == 'gp':  # reference train.py:243-244 (its GP_train_and_test, train.py:60-150)
        from .gp import GP_train_and_test
        return GP_train_and_test(X_train, Y_train, X_test, Y_test, qi_train, qi_test,
                                 cov="full" if getattr(args, "full_cov", False) else "diag", pred_stat=pred_stat)
    if (getattr(args, "sparse_tune", 0) or 0) > 0:
        kernel_fn, diag_reg = sparse_tune_kernel_fn(args, X_train, Y_train)
        return NNGP_train_and_test(args, X_train, Y_train, X_test, Y_test, qi_train, qi_test, kernel_fn=kernel_fn,
                                   diag_reg=diag_reg)
    if tune:
        kernel_fn, diag_reg = tune_kernel_fn(args, X_train, Y_train)
        return NNGP_train_and_test(args, X_train, Y_train, X_test, Y_test, qi_train, qi_test, kernel_fn=kernel_fn,
                                   diag_reg=diag_reg)
    return NNGP_train_and_test(args, X_train, Y_train, X_test, Y_test, qi_train, qi_test)


def make_parser():
    parser = ArgumentParser("NNGP/NTK estimator", formatter_class=ArgumentDefaultsHelpFormatter, conflict_handler="resolve")
    parser.add_argument("--chunk_size", default=64, type=int, help="dimension of factorized encoding")
    parser.add_argument("--kernel_type", type=str, default='nngp', help='nngp, ntk, gp')
    parser.add_argument("--feat_encode", type=str, default='dnn-encoder', help='dnn-encoder,one-hot')
    parser.add_argument('--no-cuda', action='store_true', default=True, help='kept for flag parity; ignored')
    parser.add_argument("--relations", type=str, default='forest')
    parser.add_argument("--names", type=str, default='forest')
    parser.add_argument("--query_path", type=str, default='Queries/forest_data')
    parser.add_argument("--data_path", type=str, default='')
    parser.add_argument("--schema_name", type=str, default='imdb_simple', help='yelp, tpcds, tpch')
    # additions (config 1 of BASELINE.json is not reachable from the reference CLI)
    parser.add_argument("--max_num_train", type=int, default=None)
    parser.add_argument("--max_num_test", type=int, default=None)
    parser.add_argument("--n_relu", type=int, default=1, help="hidden layers (reference: 1)")
    parser.add_argument("--activation", type=str, default="relu", choices=ACTIVATIONS, help="activation of every hidden layer")
    parser.add_argument("--leaky_alpha", type=float, default=0.1, help="negative slope of --activation leaky_relu")
    parser.add_argument("--full_cov", action='store_true', help="form the full M x M covariance like the reference")
    parser.add_argument("--tune_hyper", type=int, default=0,
                        help="steps of marginal-likelihood tuning of W_std / b_std / diag_reg before the fit (nngp only; 0: off)")
    parser.add_argument("--tune_objective", type=str, default="mll", choices=TUNE_OBJECTIVES,
                        help="what --tune_hyper minimises: the negative log marginal likelihood, or the leave-one-out nlpd / mse")
    parser.add_argument("--loo", action='store_true',
                        help="after the fit, also print the leave-one-out error and q-error profile over the training split (nngp, ntk)")
    parser.add_argument("--tune_ard", action='store_true',
                        help="with --tune_hyper: also tune one relevance per input feature (W_std of the first layer is then fixed)")
    parser.add_argument("--ard_groups", type=str, default="none", choices=("none", "pairs"),
                        help="--tune_ard: 'pairs' ties features 2i and 2i+1, the two ends of a column's range")
    parser.add_argument("--additive", type=str, default="none", choices=("none", "pairs"),
                        help="'pairs': the additive kernel -- one network per column's (upper, lower) slot pair plus the whole input "
                             "(--loo works on the plain kernel only; --tune_hyper tunes the plain kernel and adds the groups "
                             "afterwards unless --tune_additive is given)")
    parser.add_argument("--tune_additive", action='store_true',
                        help="with --tune_hyper STEPS --additive pairs: tune on the evidence of the additive kernel itself, the "
                             "term weights included (W_std of the last layer is then fixed)")
    parser.add_argument("--additive_full_weight", type=float, default=1.0,
                        help="--additive: weight of the whole-input term (0 leaves it out)")
    parser.add_argument("--sparse", type=int, default=0, metavar="M",
                        help="fit the sparse (inducing-point) NNGP on all training rows with M inducing rows (nngp only; 0: off)")
    parser.add_argument("--sparse_select", type=str, default="greedy", choices=("greedy", "random"),
                        help="--sparse: how the inducing rows are chosen")
    parser.add_argument("--sparse_chunk", type=int, default=8192, help="--sparse: training rows per accumulation step (a multiple of 128)")
    parser.add_argument("--sparse_jitter", type=float, default=1e-8,
                        help="--sparse: jitter on the inducing kernel, relative to its mean diagonal")
    parser.add_argument("--sparse_tune", type=int, default=0, metavar="STEPS",
                        help="--sparse: steps of tuning W_std / b_std / diag_reg on the sparse model's evidence before the fit (0: off)")
    parser.add_argument("--sparse_bound", type=str, default="vfe", choices=("vfe", "dtc"),
                        help="--sparse_tune: the objective, Titsias' collapsed bound (vfe) or the DTC evidence")
    parser.add_argument("--sparse_tune_ard", action='store_true',
                        help="with --sparse M --sparse_tune STEPS: also tune one relevance per input feature on the sparse evidence "
                             "(--ard_groups ties them; W_std of the first layer is fixed during the run)")
    parser.add_argument("--matrix_free", type=int, default=0, metavar="M",
                        help="the exact NNGP posterior without the N x N kernel: preconditioned CG over a fused K.V kernel, with the "
                             "sparse model of M inducing rows as preconditioner (nngp only; 0: off)")
    parser.add_argument("--matrix_free_tol", type=float, default=1e-10, metavar="T",
                        help="--matrix_free: relative residual every solve must reach")
    parser.add_argument("--matrix_free_iters", type=int, default=1000, metavar="K", help="--matrix_free: iteration limit of a solve")
    parser.add_argument("--matrix_free_groups", type=str, default="none", choices=("none", "pairs"),
                        help="--matrix_free on the additive kernel: 'pairs' is the table of --additive pairs inside the fused operator "
                             "(one layer map per group and entry in every CG iteration: about G + 1 times the plain model's cost)")
    parser.add_argument("--matrix_free_full_weight", type=float, default=1.0, metavar="W",
                        help="--matrix_free_groups: weight of the whole-input term (0 leaves it out)")
    parser.add_argument("--tune_lr", type=float, default=0.05, help="step size of --tune_hyper")
    parser.add_argument("--b_std_init", type=float, default=None, help="start of b_std for layers with b_std = 0 (--tune_hyper)")
    return parser


def parse_args(argv=None):
    """The command line with its conflicts checked: --matrix_free goes with --kernel_type nngp only, and not with --sparse, --loo,
    --tune_*, --additive or --full_cov (its own additive kernel is --matrix_free_groups, which needs --matrix_free); --sparse goes with --kernel_type nngp only, and not with --loo or --tune_*;
    --sparse_tune needs --sparse, --sparse_tune_ard needs both; --tune_additive needs --tune_hyper, --additive pairs, the NNGP
    and the marginal likelihood."""
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.sparse < 0:
        parser.error("argument --sparse: M must be >= 0")
    if args.sparse_tune < 0:
        parser.error("argument --sparse_tune: STEPS must be >= 0")
    if args.sparse_tune_ard and (args.sparse <= 0 or args.sparse_tune <= 0):
        parser.error("argument --sparse_tune_ard: needs --sparse M and --sparse_tune STEPS (it tunes relevances on the sparse evidence)")
    if args.sparse_tune > 0 and args.sparse <= 0:
        parser.error("argument --sparse_tune: needs --sparse M (it tunes the sparse model's evidence)")
    if args.tune_additive and not (args.tune_hyper > 0 and args.additive == "pairs" and args.kernel_type == "nngp"
                                   and args.tune_objective == "mll" and not args.tune_ard and args.sparse <= 0):
        parser.error("argument --tune_additive: needs --tune_hyper STEPS, --additive pairs, --kernel_type nngp and "
                     "--tune_objective mll (it tunes the additive kernel's marginal likelihood), without --tune_ard or --sparse")
    if args.sparse > 0:
        if args.kernel_type != "nngp":
            parser.error("argument --sparse: not allowed with --kernel_type %s (the sparse model is the NNGP posterior)" % args.kernel_type)
        if args.loo:
            parser.error("argument --sparse: not allowed with argument --loo")
        if args.tune_hyper or args.tune_ard:
            parser.error("argument --sparse: not allowed with argument --tune_hyper / --tune_ard")
        if args.sparse_chunk < 128 or args.sparse_chunk % 128 != 0:
            parser.error("argument --sparse_chunk: must be a positive multiple of 128")
    if args.matrix_free < 0:
        parser.error("argument --matrix_free: M must be >= 0")
    if args.matrix_free_groups != "none" and args.matrix_free <= 0:
        parser.error("argument --matrix_free_groups: needs --matrix_free M (it is the matrix-free model's additive kernel)")
    if args.matrix_free_groups == "none" and args.matrix_free_full_weight != 1.0:
        parser.error("argument --matrix_free_full_weight: needs --matrix_free_groups pairs")
    if not (np.isfinite(args.matrix_free_full_weight) and args.matrix_free_full_weight >= 0.0):
        parser.error("argument --matrix_free_full_weight: W must be finite and >= 0")
    if args.matrix_free > 0:
        if args.sparse > 0:
            parser.error("argument --matrix_free: not allowed with argument --sparse")
        if args.kernel_type != "nngp":
            parser.error("argument --matrix_free: not allowed with --kernel_type %s (it solves the NNGP posterior)" % args.kernel_type)
        if args.loo:
            parser.error("argument --matrix_free: not allowed with argument --loo")
        if args.tune_hyper or args.tune_ard or args.tune_additive:
            parser.error("argument --matrix_free: not allowed with argument --tune_hyper / --tune_ard / --tune_additive")
        if args.additive != "none":
            parser.error("argument --matrix_free: not allowed with argument --additive (the fused operator has the plain kernel only)")
        if args.full_cov:
            parser.error("argument --matrix_free: not allowed with argument --full_cov (variances only)")
        if not (0.0 < args.matrix_free_tol < 1.0) or args.matrix_free_iters < 1:
            parser.error("argument --matrix_free_tol / --matrix_free_iters: need 0 < T < 1 and K >= 1")
    args.cuda = True
    args.join_query = len(args.relations.split(',')) > 1
    return args


if __name__ == "__main__":
    args = parse_args()
    print(args)
    main(args)
