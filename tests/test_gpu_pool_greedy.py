"""Greedy pool selection by conditional variance on the MI355X (include/nngp_pool.h, csrc/pool_greedy.hip) against the NumPy float64
reference (pool_greedy_reference.py): the operator on the oracle's covariance, shapes at the edges, ties / duplicates / NaN, bit
reproducibility, GPModel.select_pool(method="greedy") and the active-learning loop.

Indices are compared exactly and in order wherever the reference says that the best and the second-best conditional variance are
at least GAP apart (asserted from the reference alone): the library and the reference differ only in the order of a float64 sum.
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import nngp_oracle as o
import pool_greedy_reference as R
from nngp_src_amd import _lib, stax
from nngp_src_amd.model import GPModel

pytestmark = pytest.mark.gpu

GAP = 1e-6       # smallest relative distance between best and second best at which equal indices are demanded
TOL = 1e-10      # gains: relative; factor rows: of max |factor|
# select_pool against the oracle's covariance: the gate on the relative shortfall of a pick behind the best available at its step is
# ten times the worst one measured on the MI355X, and never looser than 1e-3.  The measurement is 0 (printed by the test below, recorded
# in DESIGN.md section 15): the device's 150 picks are the reference's picks on the oracle's Sigma, in order.  Ten times 0 is 0, so
# what this gate demands is EQUAL PICKS, index for index.  That is safe to demand of any device: a pick can only change where the
# covariance error reaches the distance between the best and the second-best conditional variance, which is at least 2.5e-5
# (relative) at every step of this case (asserted below from the reference alone), while the level-2 covariance is documented to 4e-7
# and the gains measured here agree with the oracle's to 1.4e-12 -- a margin of 60 on the documented error, 1e7 on the measured one.
TAU = 10 * 0.0


def dev():
    return torch.device("cuda", 0)


def run(cov, count, noise, ld=None, ldf=None, factor=True, gains=True):
    """nngp_pool_select_greedy through the C ABI.  ld / ldf: leading dimensions, the padding filled with NaN.  Returns
    (indices, gains or None, factor [count, m] or None, cov buffer, factor buffer) with the buffers as NumPy arrays, padding included."""
    lib = _lib.load()
    cov = np.asarray(cov, dtype=np.float64)
    m = cov.shape[0]
    ld = m if ld is None else ld
    ldf = m if ldf is None else ldf
    cbuf = torch.full((m, ld), float("nan"), dtype=torch.float64, device=dev())
    cbuf[:, :m] = torch.from_numpy(cov).to(dev())
    idx = torch.full((max(count, 1),), -7, dtype=torch.int64, device=dev())
    gbuf = torch.full((max(count, 1),), float("nan"), dtype=torch.float64, device=dev()) if gains else None
    fbuf = torch.full((max(count, 1), ldf), float("nan"), dtype=torch.float64, device=dev()) if factor else None
    _lib.check(lib.nngp_pool_select_greedy(_lib.ptr(cbuf), m, ld, float(noise), count, _lib.ptr(idx), _lib.ptr(gbuf), _lib.ptr(fbuf),
                                           ldf, _lib.stream_ptr()), lib)
    torch.cuda.synchronize()
    return (idx.cpu().numpy()[:count], None if gbuf is None else gbuf.cpu().numpy()[:count],
            None if fbuf is None else fbuf.cpu().numpy()[:count, :m], cbuf.cpu().numpy(), None if fbuf is None else fbuf.cpu().numpy())


def check_against_reference(cov, count, noise, got, what):
    idx, gains, factor, gaps = R.greedy(cov, count, noise)
    print("%s: m %d count %d noise %.3g min gap %.2e" % (what, cov.shape[0], count, noise, gaps.min() if count else np.inf))
    assert count == 0 or gaps.min() >= GAP, "the reference itself cannot tell the picks apart: choose another input"
    np.testing.assert_array_equal(got[0], idx)
    if got[1] is not None and count:
        print("   gains: max rel err %.2e" % np.max(np.abs(got[1] - gains) / np.abs(gains)))
        np.testing.assert_allclose(got[1], gains, rtol=TOL, atol=0.0)
    if got[2] is not None and count:
        print("   factor: max err / max|factor| %.2e" % (np.abs(got[2] - factor).max() / np.abs(factor).max()))
        assert np.abs(got[2] - factor).max() <= TOL * np.abs(factor).max()


@pytest.fixture(scope="module")
def forest(golden_dir):
    g = np.load(os.path.join(golden_dir, "forest_n1000_m200.npz"))
    return g["X_train"], g["Y_train"]


def oracle_cov(x, y, n_train, pool_end):
    """(Sigma of the pool rows [n_train, pool_end) given the first n_train rows, exactly symmetric; reg of that fit)."""
    arch = o.make_arch(1)
    _, cov = o.Posterior(x[:n_train], y[:n_train], arch, 1e-3).predict(x[n_train:pool_end], "nngp", True)
    reg = 1e-3 * np.trace(o.kernel_fn(x[:n_train], None, "nngp", arch)) / n_train
    return 0.5 * (cov + cov.T), float(reg)


@pytest.fixture(scope="module")
def sigma700(forest):
    return oracle_cov(*forest, 300, 1000)


@pytest.fixture(scope="module")
def sigma333(forest):
    return oracle_cov(*forest, 128, 461)


# ---- 1. the operator on the oracle's own covariance ----
@pytest.mark.parametrize("with_noise", [True, False])
def test_operator_on_the_oracle_covariance(sigma700, with_noise):
    cov, reg = sigma700
    noise = reg if with_noise else 0.0
    check_against_reference(cov, 150, noise, run(cov, 150, noise), "forest 300 + 700")


@pytest.mark.parametrize("with_noise", [True, False])
def test_operator_on_a_pool_that_is_no_multiple_of_the_tile(sigma333, with_noise):
    cov, reg = sigma333
    assert cov.shape[0] == 333
    noise = reg if with_noise else 0.0
    check_against_reference(cov, 96, noise, run(cov, 96, noise), "forest 128 + 333")


# ---- 2. shapes at the edges ----
@pytest.mark.parametrize("m,count", [(1, 1), (65, 65), (257, 64)])
def test_edge_shapes(m, count):
    cov = R.synthetic_spd(m, seed=7)
    got = run(cov, count, 0.25)
    check_against_reference(cov, count, 0.25, got, "synthetic")
    if count == m:
        assert sorted(got[0].tolist()) == list(range(m))  # every index exactly once


def test_leading_dimensions_with_nan_in_the_padding():
    m, count = 257, 64
    cov = R.synthetic_spd(m, seed=7)
    plain = run(cov, count, 0.25)
    padded = run(cov, count, 0.25, ld=m + 7, ldf=m + 5)
    check_against_reference(cov, count, 0.25, padded, "synthetic, ld = m + 7, ldf = m + 5")
    for a, b in zip(plain[:3], padded[:3]):
        np.testing.assert_array_equal(a, b)  # the same bits with and without padding
    assert np.isnan(padded[3][:, m:]).all() and np.array_equal(padded[3][:, :m], cov)  # cov and its padding untouched
    assert np.isnan(padded[4][:, m:]).all()  # the factor's padding untouched


def test_without_factor_and_without_gains():
    m, count = 257, 64
    cov = R.synthetic_spd(m, seed=7)
    full = run(cov, count, 0.25)
    no_factor = run(cov, count, 0.25, factor=False)
    no_gains = run(cov, count, 0.25, gains=False)
    neither = run(cov, count, 0.25, factor=False, gains=False)
    check_against_reference(cov, count, 0.25, no_factor, "synthetic, factor = NULL")
    check_against_reference(cov, count, 0.25, no_gains, "synthetic, gains = NULL")
    check_against_reference(cov, count, 0.25, neither, "synthetic, both NULL")
    np.testing.assert_array_equal(no_factor[1], full[1])
    np.testing.assert_array_equal(no_gains[2], full[2])


def test_count_zero_touches_nothing():
    cov = R.synthetic_spd(65, seed=7)
    idx, gains, factor, _, fbuf = run(cov, 0, 0.25)
    assert idx.shape == (0,) and np.isnan(fbuf).all()
    lib = _lib.load()
    marker = torch.full((3,), -7, dtype=torch.int64, device=dev())
    cbuf = torch.from_numpy(cov).to(dev())
    assert lib.nngp_pool_select_greedy(_lib.ptr(cbuf), 65, 65, 0.25, 0, _lib.ptr(marker), None, None, 0, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert marker.cpu().tolist() == [-7, -7, -7]


def test_python_operator_on_torch_and_numpy_input():
    import nngp_src_amd
    cov = R.synthetic_spd(257, seed=7)
    idx, gains, factor, _ = R.greedy(cov, 64, 0.25)
    got = nngp_src_amd.pool_select_greedy(cov, 64, noise=0.25, return_factor=True)
    assert all(isinstance(a, np.ndarray) for a in got) and len(got) == 3
    np.testing.assert_array_equal(got[0], idx)
    np.testing.assert_allclose(got[1], gains, rtol=TOL)
    assert np.abs(got[2] - factor).max() <= TOL * np.abs(factor).max()
    wide = torch.full((257, 300), float("nan"), dtype=torch.float64, device=dev())
    wide[:, :257] = torch.from_numpy(cov).to(dev())
    got_t = nngp_src_amd.pool_select_greedy(wide[:, :257], 64, noise=0.25)  # a view with a row stride of its own, used in place
    assert len(got_t) == 2 and all(t.is_cuda for t in got_t)
    np.testing.assert_array_equal(got_t[0].cpu().numpy(), got[0])
    np.testing.assert_array_equal(got_t[1].cpu().numpy(), got[1])
    assert len(nngp_src_amd.pool_select_greedy(cov, 0)[0]) == 0
    with pytest.raises(ValueError):
        nngp_src_amd.pool_select_greedy(cov, 300)
    with pytest.raises(ValueError):
        nngp_src_amd.pool_select_greedy(cov, 3, noise=-1.0)
    with pytest.raises(ValueError):
        nngp_src_amd.pool_select_greedy(cov[:, :5], 3)


# ---- 3. ties, duplicates, NaN ----
def test_equal_variances_go_to_the_lowest_index():
    idx, gains, factor, _, _ = run(np.eye(130), 130, 0.5)
    np.testing.assert_array_equal(idx, np.arange(130))
    np.testing.assert_array_equal(gains, np.ones(130))
    np.testing.assert_array_equal(factor, np.eye(130) / np.sqrt(1.5))


def test_no_two_picks_are_copies_of_each_other(sigma700):
    cov70 = sigma700[0][:70, :70]
    twice = np.concatenate([np.arange(70), np.arange(70)])
    cov = cov70[np.ix_(twice, twice)]  # every pool row present twice: index i and i + 70 are the same query
    idx, gains, _, _, _ = run(cov, 70, 0.0)
    assert len(set((idx % 70).tolist())) == 70, "a query and its copy were both picked"
    ref_gains = R.greedy(cov70, 70, 0.0)[1]
    np.testing.assert_allclose(gains, ref_gains, rtol=1e-8)  # ... and the picks are worth what they are without the copies
    assert gains.min() > 1e-6 * gains.max()


def test_nan_variances_are_picked_last():
    m = 67
    cov = R.synthetic_spd(m, seed=7)
    bad = [3, 40, 66]
    cov[bad, bad] = np.nan
    idx, gains, _, _, _ = run(cov, m, 0.25)
    assert sorted(idx.tolist()) == list(range(m))
    assert idx[-3:].tolist() == bad and not set(bad) & set(idx[:m - 3].tolist())
    assert np.isfinite(gains[:m - 3]).all() and np.isnan(gains[m - 3:]).all()
    np.testing.assert_array_equal(idx, R.greedy(cov, m, 0.25)[0])


def test_every_index_is_picked_once_whatever_the_covariance_holds():
    """The mark of a picked index does not depend on its residual: a NaN off the diagonal must not make a picked index pickable
    again, and a column entry whose square overflows must not mark an index that was never picked."""
    from nngp_src_amd.active import greedy_select
    m = 67
    cov = R.synthetic_spd(m, seed=7)
    first = int(R.greedy(cov, 1, 0.25)[0][0])
    other = (first + 5) % m
    nan_cov = cov.copy()
    nan_cov[first, other] = nan_cov[other, first] = np.nan  # met by the very first column; `first` is picked by then
    nan_cov[10, 50] = nan_cov[50, 10] = np.nan
    idx, gains, _, _, _ = run(nan_cov, m, 0.25)
    assert sorted(idx.tolist()) == list(range(m)), "an index was picked twice"
    np.testing.assert_array_equal(idx, R.greedy(nan_cov, m, 0.25)[0])
    np.testing.assert_array_equal(greedy_select(nan_cov, m, 0.25), idx)
    assert idx[0] == first and np.isnan(gains[list(idx).index(other)])
    big = cov.copy()
    big[first, other] = big[other, first] = 1e200  # c = 1e200 / sqrt(pivot): c * c is +inf, d - c * c is -inf
    idx, _, _, _, _ = run(big, m, 0.25)
    assert sorted(idx.tolist()) == list(range(m)), "an index that was never picked was taken for a picked one"
    assert sorted(greedy_select(big, m, 0.25).tolist()) == list(range(m))
    with np.errstate(over="ignore", invalid="ignore"):
        assert sorted(R.greedy(big, m, 0.25)[0].tolist()) == list(range(m))


# ---- 4. bit reproducibility ----
def test_two_calls_give_the_same_bits():
    cov = R.synthetic_spd(1500, seed=11)
    a = run(cov, 200, 0.1)
    b = run(cov, 200, 0.1)
    for u, v in zip(a[:3], b[:3]):
        assert u.tobytes() == v.tobytes()
    idx, gains, _, _ = R.greedy(cov, 200, 0.1)
    agree = int(np.argmax(np.append(a[0] != idx, True)))  # steps before the first one that differs (all 200 if none does)
    print("m 1500: %d of 200 picks agree with the reference before the first difference" % agree)
    assert len(set(a[0].tolist())) == 200
    got, best = R.replay(cov, a[0], 0.1)
    assert np.max((best - got) / best) <= 1e-9  # every pick is the best available up to the rounding of the sum


# ---- 5. the model ----
def test_select_pool_greedy_on_the_model(forest, sigma700):
    x, y = forest
    cov, reg = sigma700
    model = GPModel(300, x.shape[1], [1.0, 1.0], [0.0, 0.0], diag_reg=1e-3).fit(x[:300], y[:300])
    try:
        assert abs(model.info()["reg"] - reg) <= 1e-9 * reg
        picks, gains = model.select_pool(x[300:1000], 150, method="greedy", return_gains=True)
        np.testing.assert_array_equal(model.select_pool(x[300:1000], 150, method="greedy"), picks)
        # (a) 150 distinct indices of the pool
        assert picks.shape == (150,) and picks.dtype == np.int64 and len(set(picks.tolist())) == 150
        assert picks.min() >= 0 and picks.max() < 700
        # (b) replayed on the oracle's covariance, every pick is within TAU of the best available at its step
        got, best = R.replay(cov, picks, reg)
        shortfall = np.max((best - got) / best)
        ref_picks, _, _, ref_gaps = R.greedy(cov, 150, reg)
        assert ref_gaps.min() >= 2.5e-5  # what makes equal picks a fair demand (see TAU)
        print("select_pool greedy: worst shortfall %.3e (gate %.1e), %d of 150 picks equal the reference's, gains rel err %.2e"
              % (shortfall, TAU, int(np.sum(picks == ref_picks)), np.max(np.abs(gains - got) / got)))
        assert TAU <= 1e-3 and shortfall <= TAU
        np.testing.assert_allclose(gains, got, rtol=1e-5)
        # (c) at least half of what the reference's greedy rule gains over top-k in remaining variance
        r_top, r_ref, r_got = (R.remaining_variance(cov, s, reg) for s in (R.top_k(cov, 150), ref_picks, picks))
        margin = (r_top - r_ref) / r_top
        print("remaining variance: top-k %.0f reference greedy %.0f (%.2f %% less) device greedy %.0f (%.2f %% less)"
              % (r_top, r_ref, 100 * margin, r_got, 100 * (r_top - r_got) / r_top))
        assert margin > 0.04 and r_got <= r_top * (1.0 - 0.5 * margin)
        # (d) arguments
        with pytest.raises(ValueError):
            model.select_pool(x[300:1000], 150, method="greedy", biased=True)
        with pytest.raises(ValueError):
            model.select_pool(x[300:1000], 150, method="marginal")
        with pytest.raises(ValueError):
            model.select_pool(x[300:1000], 150, return_gains=True)
        assert model.select_pool(x[300:1000], 0, method="greedy").shape == (0,)
        assert model.select_pool(x[300:310], 150, method="greedy").shape == (10,)  # count above the pool: the whole pool
    finally:
        model.close()


# ---- 6. the loop ----
def test_active_learning_loop_with_greedy_selection(forest, monkeypatch):
    from nngp_src_amd.active import ActiveLearner
    x, y = forest
    xtr, ytr, xpool, ypool, xval, yval = x[:128], y[:128], x[128:461], y[128:461], x[461:600], y[461:600]
    _, _, kernel_fn = stax.serial(stax.Dense(512), stax.Relu(), stax.Dense(1))
    learner = ActiveLearner(budget=40, active_iters=2, kernel_type="nngp", selection="greedy")
    with contextlib.redirect_stdout(io.StringIO()):
        pf = learner.train(kernel_fn, xtr, ytr, n_cap=208)
    direct = learner._model.select_pool(xpool, 40, method="greedy")
    np.testing.assert_array_equal(learner.active_test(pf, xpool), direct)
    assert len(set(direct.tolist())) == 40
    # the default is what it was: selection=None draws what select_pool(biased=True, seed=10) draws
    default = ActiveLearner(budget=40, active_iters=0)
    assert default.selection is None and default.biased_sample is True
    with contextlib.redirect_stdout(io.StringIO()):
        pf0 = default.train(kernel_fn, xtr, ytr)
    np.testing.assert_array_equal(default.active_test(pf0, xpool), default._model.select_pool(xpool, 40, biased=True, seed=10))
    assert set(default.active_test(pf0, xpool).tolist()) != set(direct.tolist())
    default._model.close()

    calls = {"fit": 0, "append": 0}
    fit, append = GPModel.fit, GPModel.append
    monkeypatch.setattr(GPModel, "fit", lambda self, *a, **k: (calls.__setitem__("fit", calls["fit"] + 1), fit(self, *a, **k))[1])
    monkeypatch.setattr(GPModel, "append", lambda self, *a, **k: (calls.__setitem__("append", calls["append"] + 1), append(self, *a, **k))[1])
    first = learner._model
    merged = []
    merge = learner.merge_data
    monkeypatch.setattr(learner, "merge_data", lambda *a: (merged.append(merge(*a)), merged[-1])[1])
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        learner.active_train(kernel_fn, xtr, ytr, xpool, ypool, xval, yval)
    assert "# Training samples: 208" in buf.getvalue() and buf.getvalue().count("Selection 40") == 2
    # the model is the one fitted above, extended twice: no refit after the first fit
    assert learner._model is first and first.n == 208 and first.info()["n"] == 208
    assert calls == {"fit": 1, "append": 2}
    x_final = merged[-1][0]
    assert x_final.shape[0] == 128 + 80 and np.unique(x_final, axis=0).shape[0] == 208
    np.testing.assert_array_equal(x_final[128:168], xpool[direct])  # the first round moved exactly the picks above
    assert len(learner.history) == 3 and np.isfinite(learner.history).all()
    first.close()
