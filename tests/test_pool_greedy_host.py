"""Greedy pool selection by conditional variance, without a GPU: the NumPy reference (pool_greedy_reference.py) against plain linear
algebra, the argument checks of nngp_pool_select_greedy, the bindings of include/nngp_pool.h, the command line and the NumPy
fallback of the active-learning loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import nngp_oracle as o
import pool_greedy_reference as R
from nngp_src_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forest_pool_cov(golden_dir, n_train=300, pool_end=1000):
    """(Sigma, reg): the oracle's posterior covariance of the forest rows [n_train, pool_end) given the first n_train, made exactly
    symmetric, and the noise the posterior was fitted with (diag_reg 1e-3 of the mean kernel diagonal)."""
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    x, y = g["X_train"], g["Y_train"]
    arch = o.make_arch(1)
    _, cov = o.Posterior(x[:n_train], y[:n_train], arch, 1e-3).predict(x[n_train:pool_end], "nngp", True)
    reg = 1e-3 * np.trace(o.kernel_fn(x[:n_train], None, "nngp", arch)) / n_train
    return 0.5 * (cov + cov.T), float(reg)


@pytest.fixture(scope="module")
def forest(golden_dir):
    return forest_pool_cov(golden_dir)


def test_reference_factor_rows_reproduce_the_picked_rows():
    """noise = 0: C^T C restricted to the picked rows is Sigma[S, :] (a pivoted Cholesky interpolates the rows it has pivoted on)."""
    cov = R.synthetic_spd(90, seed=3)
    idx, gains, factor, gaps = R.greedy(cov, 40, 0.0)
    assert len(set(idx.tolist())) == 40 and gaps.min() > 0
    np.testing.assert_allclose(factor[:, idx].T @ factor, cov[idx, :], rtol=0, atol=1e-12 * np.abs(cov).max())
    # pivoted factor: row j vanishes on the earlier picks, and its own pick holds sqrt(gain)
    for j in range(40):
        assert np.abs(factor[j, idx[:j]]).max(initial=0.0) < 1e-12 * np.abs(cov).max()
        np.testing.assert_allclose(factor[j, idx[j]], np.sqrt(gains[j]), rtol=1e-12)


@pytest.mark.parametrize("noise", [0.0, 0.3])
def test_reference_gains_are_schur_complement_diagonals(noise):
    cov = R.synthetic_spd(70, seed=5)
    idx, gains, _, _ = R.greedy(cov, 25, noise)
    got, best = R.replay(cov, idx, noise)
    for j in range(25):
        s = idx[:j]
        schur = np.diag(cov) - (np.sum(cov[s, :] * np.linalg.solve(cov[np.ix_(s, s)] + noise * np.eye(j), cov[s, :]), axis=0) if j else 0.0)
        np.testing.assert_allclose(gains[j], schur[idx[j]], rtol=1e-10)
        rest = np.setdiff1d(np.arange(70), s)
        assert idx[j] == rest[np.argmax(schur[rest])]
        np.testing.assert_allclose(best[j], schur[rest].max(), rtol=1e-10)
    np.testing.assert_allclose(got, gains, rtol=1e-12)
    np.testing.assert_allclose(got, best, rtol=1e-12)  # greedy picks ARE the best available
    # remaining_variance is the trace of the last Schur complement
    s = idx
    full = cov - cov[:, s] @ np.linalg.solve(cov[np.ix_(s, s)] + noise * np.eye(25), cov[s, :])
    np.testing.assert_allclose(R.remaining_variance(cov, idx, noise), np.trace(full), rtol=1e-10)


def test_reference_rules_ties_nan_and_degenerate_pivots():
    idx, gains, factor, _ = R.greedy(np.eye(7), 7, 0.5)
    assert idx.tolist() == list(range(7)) and np.all(gains == 1.0)
    cov = R.synthetic_spd(12, seed=1)
    cov[[2, 5], [2, 5]] = np.nan
    idx, _, _, _ = R.greedy(cov, 12, 0.0)
    assert idx[-2:].tolist() == [2, 5] and sorted(idx.tolist()) == list(range(12))
    idx, gains, factor, _ = R.greedy(np.zeros((4, 4)), 3, 0.0)  # d + noise = 0: zero columns, picks in index order
    assert idx.tolist() == [0, 1, 2] and not factor.any() and not gains.any()


def test_greedy_leaves_less_variance_than_top_k_on_the_forest_fixture(forest):
    """700 pool rows, noise = reg, the sums of the remaining posterior variances."""
    cov, reg = forest
    before = np.trace(cov)
    out = {}
    for count in (150, 300):
        idx, _, _, gaps = R.greedy(cov, count, reg)
        out[count] = (R.remaining_variance(cov, idx, reg), R.remaining_variance(cov, R.top_k(cov, count), reg),
                      len(set(idx.tolist()) & set(R.top_k(cov, count).tolist())), gaps.min())
        print("forest pool 700, %d picks: before %.0f greedy %.0f top-k %.0f common %d min gap %.2e" % ((count, before) + out[count]))
    np.testing.assert_allclose([before, out[150][0], out[150][1]], [685887, 359782, 376835], rtol=2e-5)
    np.testing.assert_allclose([out[300][0], out[300][1]], [218621, 230735], rtol=2e-5)
    assert out[150][0] < 0.96 * out[150][1] and out[150][2] == 119


def test_argument_validation_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: every call below fails its checks before any GPU work
    call = lib.nngp_pool_select_greedy
    for args, word in (((None, 4, 4, 0.0, 2, one, None, None, 0, None), b"NULL"),
                       ((one, 4, 4, 0.0, 2, None, None, None, 0, None), b"NULL"),
                       ((one, 4, 4, 0.0, 5, one, None, None, 0, None), b"count"),
                       ((one, 4, 4, 0.0, -1, one, None, None, 0, None), b"count"),
                       ((one, 0, 4, 0.0, 0, one, None, None, 0, None), b"m >= 1"),
                       ((one, 4, 3, 0.0, 2, one, None, None, 0, None), b"ld < m"),
                       ((one, 4, 4, 0.0, 2, one, None, one, 3, None), b"ldf < m"),
                       ((one, 4, 4, -1e-9, 2, one, None, None, 0, None), b"noise"),
                       ((one, 4, 4, float("nan"), 2, one, None, None, 0, None), b"noise"),
                       ((one, 4, 4, float("inf"), 2, one, None, None, 0, None), b"noise")):
        rc = call(*args)
        assert rc != 0 and word in lib.nngp_last_error(), (args, lib.nngp_last_error())
    with pytest.raises(_lib.NngpError):
        _lib.check(rc)
    assert call(one, 4, 4, 0.0, 0, one, None, None, 0, None) == 0  # count 0: nothing to do, nothing touched


def test_the_pool_prototypes_bind_and_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_pool.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.POOL_ABI_SYMBOLS)
    lib = _lib.load()
    assert len(lib.nngp_pool_select_greedy.argtypes) == 10 and lib.nngp_pool_select_greedy.restype is ctypes.c_int
    with open(os.path.join(ROOT, "include", "nngp_hip.h")) as f:
        assert "nngp_pool_select_greedy" not in f.read()  # that header's symbol set is pinned to ABI_SYMBOLS
    import nngp_src_amd
    from nngp_src_amd import pool
    assert nngp_src_amd.pool_select_greedy is pool.pool_select_greedy
    for bad in (dict(count=5, noise=0.0), dict(count=-1, noise=0.0), dict(count=1, noise=-1.0), dict(count=1, noise=float("nan"))):
        with pytest.raises(ValueError):
            pool.check_greedy_arguments(4, **bad)


def test_cli_greedy_flag_and_its_conflict_with_top_k(capsys):
    from nngp_src_amd import active_train
    from nngp_src_amd.active import ActiveLearner
    args = active_train.parse_args([])
    assert args.greedy is False and args.selection is None and args.biased_sample is True
    assert ActiveLearner(args).selection is None
    args = active_train.parse_args(["--greedy", "--budget", "7"])
    assert args.selection == "greedy" and args.top_k is False
    learner = ActiveLearner(args)
    assert learner.selection == "greedy" and learner.budget == 7
    args = active_train.parse_args(["--top_k"])
    assert args.selection is None and args.biased_sample is False
    with pytest.raises(SystemExit) as e:
        active_train.parse_args(["--greedy", "--top_k"])
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
    with pytest.raises(ValueError):
        ActiveLearner(selection="random")


def test_numpy_fallback_of_the_learner_equals_the_reference(forest):
    """ActiveLearner(selection='greedy').active_test on a predict_fn without a device model: the same picks as the reference."""
    from nngp_src_amd.active import ActiveLearner, greedy_select
    cov, reg = forest
    cov = cov[:333, :333]
    calls = []

    def predict_fn(x_test=None, get=None, compute_cov=False):
        calls.append(compute_cov)
        return np.zeros((cov.shape[0], 1)), cov

    x_pool = np.zeros((cov.shape[0], 3))
    for noise in (0.0, reg):
        predict_fn.noise = noise
        got = ActiveLearner(budget=40, selection="greedy").active_test(predict_fn, x_pool)
        np.testing.assert_array_equal(got, R.greedy(cov, 40, noise)[0])
    assert calls == [True, True]
    del predict_fn.noise  # a predict_fn that states no noise: 0
    np.testing.assert_array_equal(ActiveLearner(budget=9, selection="greedy").active_test(predict_fn, x_pool), R.greedy(cov, 9, 0.0)[0])
    assert ActiveLearner(budget=1000, selection="greedy").active_test(predict_fn, x_pool).shape == (333,)  # budget above the pool
    # the rules at their edges, as in the reference
    tied = np.eye(6)
    tied[[1, 4], [1, 4]] = np.nan
    np.testing.assert_array_equal(greedy_select(tied, 6, 0.5), R.greedy(tied, 6, 0.5)[0])
    np.testing.assert_array_equal(greedy_select(np.zeros((4, 4)), 3), [0, 1, 2])
    # the exclusion of a picked index does not depend on its residual: NaN off the diagonal, a column whose square overflows
    bad = R.synthetic_spd(30, seed=7)
    first = int(R.greedy(bad, 1, 0.25)[0][0])
    bad[first, (first + 5) % 30] = bad[(first + 5) % 30, first] = np.nan
    bad[3, 20] = bad[20, 3] = np.nan
    got = greedy_select(bad, 30, 0.25)
    assert sorted(got.tolist()) == list(range(30))
    np.testing.assert_array_equal(got, R.greedy(bad, 30, 0.25)[0])
    big = R.synthetic_spd(30, seed=7)
    big[first, (first + 5) % 30] = big[(first + 5) % 30, first] = 1e200
    assert sorted(greedy_select(big, 30, 0.25).tolist()) == list(range(30))
