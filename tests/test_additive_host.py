"""Additive kernels over feature groups, without a GPU: the NumPy reference (additive_reference.py), the validation of group
tables, the bindings of include/nngp_additive.h, what mll / loo refuse, the checkpoint fields and the accuracy the feature is for."""
import os
import re

import numpy as np
import pytest

import additive_reference as R
import nngp_oracle as o
from nngp_src_amd import _lib, loo, mll, stax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS, WEIGHTS = [(0, 2), (2, 3), (3, 7), (1, 5)], [1.0, 0.0, 2.5, 0.3]


def test_reference_sum_is_symmetric_and_psd():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 7))
    for get in ("nngp", "ntk"):
        for acts, w, b in ((None, [1.1, 0.9, 1.0], [0.3] * 3), ([("erf", 1.0, 1.0, 0.0)], [1.0, 1.0], [0.1, 0.1])):
            k = R.kernel_fn(x, None, get, w, b, acts, GROUPS, WEIGHTS, 1.0)
            assert np.array_equal(k, k.T)
            assert np.linalg.eigvalsh(k).min() > -1e-10 * np.abs(k).max()
            dn, dt = R.diag_kernel(x, w, b, acts, GROUPS, WEIGHTS, 1.0)
            # the ReLU oracle takes its diagonal through sqrt(q q - k^2) like any entry: rounding noise of the Gram product,
            # sqrt(2^-52) = 1.5e-8 of angle at most, where diag_kernel has theta = 0
            np.testing.assert_allclose(np.diag(k), dn if get == "nngp" else dt, rtol=1e-7)


def test_one_group_over_all_features_is_the_oracle_kernel():
    rng = np.random.default_rng(1)
    x, x2 = rng.standard_normal((40, 6)), rng.standard_normal((23, 6))
    arch = o.make_arch(2, [1.2, 1.0, 0.8], [0.1, 0.0, 0.2])
    for get in ("nngp", "ntk"):
        for other in (None, x2):
            got = R.kernel_fn(x, other, get, list(arch.w_std), list(arch.b_std), None, [(0, 6)], [1.0], 0.0)
            np.testing.assert_array_equal(got, o.kernel_fn(x, other, get, arch))


def test_group_validation_and_the_pairs_helper():
    assert stax.pair_groups(6) == ((0, 2), (2, 4), (4, 6))
    assert _lib.check_groups("pairs", d=4) == (((0, 2), (2, 4)), (1.0, 1.0), 1.0)
    assert _lib.check_groups(GROUPS, WEIGHTS, 0.0, d=7) == (tuple(GROUPS), tuple(WEIGHTS), 0.0)
    assert _lib.check_groups([], None, 2.0, d=7) == ((), (), 2.0)
    for d in (0, 1, 7):
        with pytest.raises(ValueError):
            stax.pair_groups(d)
    bad = [dict(groups=[(0, 0)]), dict(groups=[(3, 2)]), dict(groups=[(-1, 2)]), dict(groups=[(0, 8)]), dict(groups=[(0.5, 2)]),
           dict(groups=[(0, 2)], weights=[-1.0]), dict(groups=[(0, 2)], weights=[float("nan")]),
           dict(groups=[(0, 2)], weights=[float("inf")]), dict(groups=[(0, 2)], weights=[1.0, 1.0]),
           dict(groups=[(0, 2)], weights=[0.0], full_weight=0.0), dict(groups=[], full_weight=0.0),
           dict(groups=[(0, 2)], full_weight=-1.0), dict(groups=[(0, 2)], full_weight=float("nan")),
           dict(groups=[(0, 1)] * (_lib.MAX_GROUPS + 1)), dict(groups="triples"), dict(groups=[(0, 1, 2)])]
    for kw in bad:
        with pytest.raises(ValueError):
            _lib.check_groups(d=7, **kw)
    with pytest.raises(ValueError):
        _lib.check_groups("pairs")  # needs d
    _, _, kf = stax.additive((stax.Dense(8), stax.Relu(), stax.Dense(1)), GROUPS, WEIGHTS, full_weight=0.5)
    assert (kf.groups, kf.group_weights, kf.full_weight) == (tuple(GROUPS), tuple(WEIGHTS), 0.5)
    assert kf.group_table(7) == (tuple(GROUPS), tuple(WEIGHTS), 0.5)
    with pytest.raises(ValueError):
        kf.group_table(6)  # (3, 7) does not fit 6 features
    scaled = kf.with_input_scale(np.ones(7))
    assert scaled.groups == kf.groups and scaled.full_weight == 0.5 and scaled.input_scale is not None
    plain = scaled.with_groups(None)
    assert plain.groups is None and plain.input_scale is not None
    _, _, serial_kf = stax.serial(stax.Dense(8), stax.Relu(), stax.Dense(1))
    assert serial_kf.groups is None and serial_kf.with_groups("pairs").group_table(4)[0] == ((0, 2), (2, 4))
    with pytest.raises(ValueError):
        serial_kf.with_groups("pairs", weights=[1.0, 1.0])
    g = _lib.make_groups(*_lib.check_groups(GROUPS, WEIGHTS, 0.5, d=7))
    assert g.n_groups == 4 and [g.begin[i] for i in range(4)] == [0, 2, 3, 1] and [g.end[i] for i in range(4)] == [2, 3, 7, 5]
    assert [g.weight[i] for i in range(4)] == WEIGHTS and g.full_weight == 0.5


def test_the_additive_prototypes_bind_and_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_additive.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.ADDITIVE_ABI_SYMBOLS)
    assert int(re.search(r"#define NNGP_MAX_GROUPS (\d+)", text).group(1)) == _lib.MAX_GROUPS >= 128

    class Fn:
        argtypes = restype = None

    class Lib:
        pass

    lib = Lib()
    for name in _lib.ADDITIVE_ABI_SYMBOLS:
        setattr(lib, name, Fn())
    _lib.bind_additive_prototypes(lib)
    assert len(lib.nngp_kernel_build_additive.argtypes) == 14
    assert len(lib.nngp_kernel_diag_additive.argtypes) == 8
    assert len(lib.nngp_model_create_additive.argtypes) == 10
    if os.path.exists(_lib.LIB_PATH):
        real = _lib.load()
        for name in _lib.ADDITIVE_ABI_SYMBOLS:
            assert hasattr(real, name), name


def test_mll_and_loo_reject_a_grouped_kernel_fn():
    _, _, kf = stax.additive((stax.Dense(8), stax.Relu(), stax.Dense(1)), "pairs")
    from nngp_src_amd import batch
    for fn in (kf, batch(kf, batch_size=4, device_count=0)):
        with pytest.raises(ValueError, match="additive"):
            mll.check_supported(fn)
        with pytest.raises(ValueError, match="additive"):
            loo.check_supported(fn)
    x, y = np.zeros((4, 4)), np.zeros(4)
    with pytest.raises(ValueError, match="additive"):
        mll.marginal_likelihood(kf, x, y)
    with pytest.raises(ValueError, match="additive"):
        loo.loo_predict(kf, x, y)


def test_checkpoint_fields_round_trip(tmp_path):
    """The fields GPModel.save writes for a group table (KernelSpec.to_fields) through an .npz and back through what
    GPModel.load reads them with (KernelSpec.from_fields); a checkpoint without them gives no group arguments."""
    import inspect
    from nngp_src_amd import model
    from nngp_src_amd.kernel_spec import KernelSpec
    w, b = [1.0, 1.0], [0.0, 0.0]

    def table_of(spec):
        return None if spec.groups is None else _lib.check_groups(spec.groups, spec.group_weights, spec.full_weight, d=7)

    table = _lib.check_groups(GROUPS, WEIGHTS, 0.25, d=7)
    path = str(tmp_path / "m.npz")
    np.savez(path, x=np.zeros((2, 7)), **KernelSpec(w, b, None, None, *table).to_fields())
    assert table_of(KernelSpec.from_fields(np.load(path, allow_pickle=False))) == table
    empty = _lib.check_groups([], None, 2.0, d=7)
    np.savez(path, **KernelSpec(w, b, None, None, *empty).to_fields())
    assert table_of(KernelSpec.from_fields(np.load(path, allow_pickle=False))) == empty
    plain = KernelSpec(w, b, None, None, None, None, 1.0).to_fields()
    assert not {"groups", "group_weights", "full_weight"} & set(plain)
    np.savez(path, x=np.zeros((2, 7)), **plain)
    back = KernelSpec.from_fields(np.load(path, allow_pickle=False))
    assert (back.groups, back.group_weights, back.full_weight) == (None, None, 1.0)
    for fn, helper in ((model.GPModel.save, "to_fields"), (model.GPModel.load, "from_fields")):
        assert helper in inspect.getsource(fn)
    params = inspect.signature(model.GPModel.__init__).parameters
    assert params["groups"].default is None and params["group_weights"].default is None and params["full_weight"].default == 1.0


def test_train_cli_and_estimator_flags():
    from nngp_src_amd import train
    from nngp_src_amd.estimator import Estimator
    import inspect
    a = train.make_parser().parse_args([])
    assert a.additive == "none" and a.additive_full_weight == 1.0
    a = train.make_parser().parse_args(["--additive", "pairs", "--additive_full_weight", "0.5"])
    assert (a.additive, a.additive_full_weight) == ("pairs", 0.5)
    with pytest.raises(SystemExit):
        train.make_parser().parse_args(["--additive", "triples"])
    assert inspect.signature(Estimator.__init__).parameters["groups"].default is None


def _mse(golden_dir, name, groups, full_weight, get="nngp", n_relu=1):
    g = np.load(os.path.join(golden_dir, name))
    w, b = [1.0] * (n_relu + 1), [0.0] * (n_relu + 1)
    mean = R.Posterior(g["X_train"], g["Y_train"], w, b, None, groups, None, full_weight, diag_reg=1e-3).predict(
        g["X_test"], get, False)
    return float(np.mean((mean - g["Y_test"].reshape(mean.shape)) ** 2))


def test_pairs_plus_full_halves_the_error_on_the_forest_fixtures(golden_dir):
    """The table of DESIGN.md section 14 (float64 reference, all weights 1, diag_reg 1e-3 relative)."""
    pairs = R.pair_groups(20)
    big = [_mse(golden_dir, "forest_n1000_m200.npz", *a) for a in (([], 1.0), (pairs, 0.0), (pairs, 1.0))]
    small = [_mse(golden_dir, "forest_n256_m64.npz", *a) for a in (([], 1.0), (pairs, 0.0), (pairs, 1.0))]
    print("forest_n1000_m200 nngp n_relu=1: full %.3f pairs %.3f pairs+full %.3f (ratio %.3f)" % (*big, big[2] / big[0]))
    print("forest_n256_m64   nngp n_relu=1: full %.3f pairs %.3f pairs+full %.3f" % tuple(small))
    np.testing.assert_allclose(big, [8.374, 4.245, 4.134], atol=2e-3)
    np.testing.assert_allclose(small, [9.493, 5.745, 6.258], atol=2e-3)
    assert big[2] < 0.6 * big[0]
