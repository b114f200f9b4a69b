"""The matrix-free model on the additive kernel without a GPU (include/nngp_matfree_additive.h): the header against its
bindings, every -2 that needs no device, the Python refusals, the command line and the Estimator keyword."""
import ctypes
import os
import re

import numpy as np
import pytest

from nngp_src_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arch():
    return _lib.make_arch_act([1.0, 1.0], [0.0, 0.0], [("relu",)])


def test_the_additive_prototypes_bind_and_match_the_header():
    with open(os.path.join(ROOT, "include", "nngp_matfree_additive.h")) as f:
        text = f.read()
    assert set(re.findall(r"\bint (nngp_\w+)\(", text)) == set(_lib.MATFREE_ADDITIVE_ABI_SYMBOLS)
    lib = _lib.load()
    counts = {}
    for name, body in re.findall(r"\bint (nngp_\w+)\(([^;]*)\);", text):
        counts[name] = len([a for a in body.split(",") if a.strip()])
    assert counts == {"nngp_matfree_create_additive": 12, "nngp_kmv_additive_f64": 12}
    for name in _lib.MATFREE_ADDITIVE_ABI_SYMBOLS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == counts[name] and fn.restype is ctypes.c_int, name
    with open(os.path.join(ROOT, "include", "nngp_matfree.h")) as f:
        plain = f.read()
    for name in _lib.MATFREE_ADDITIVE_ABI_SYMBOLS:
        assert name not in plain  # that header's symbol set is pinned
    import nngp_src_amd
    from nngp_src_amd import matfree, matfree_additive
    assert nngp_src_amd.AdditiveMatrixFreeGPModel is matfree_additive.AdditiveMatrixFreeGPModel
    assert nngp_src_amd.matfree_additive_mse_ensemble is matfree_additive.matfree_additive_mse_ensemble
    assert issubclass(matfree_additive.AdditiveMatrixFreeGPModel, matfree.MatrixFreeGPModel)


def _bad_tables():
    """(table, a word of the error) for every refusal of nngp_additive.h's table; d = 8."""
    many = _lib.MAX_GROUPS + 1
    return [(_lib.make_groups(((0, 2), (6, 9)), (1.0, 1.0), 1.0), b"range"), (_lib.make_groups(((3, 3),), (1.0,), 1.0), b"range"),
            (_lib.make_groups(((-1, 2),), (1.0,), 1.0), b"range"), (_lib.make_groups(((0, 2),), (-0.5,), 1.0), b"weight"),
            (_lib.make_groups(((0, 2),), (float("nan"),), 1.0), b"weight"), (_lib.make_groups(((0, 2),), (1.0,), -1.0), b"full_weight"),
            (_lib.make_groups(((0, 2), (2, 4)), (0.0, 0.0), 0.0), b"all weights are zero"),
            (_lib.make_groups(((0, 2),) * many, (1.0,) * many, 1.0), b"n_groups")]


def test_argument_validation_without_gpu():
    """Both calls refuse a missing or bad table, and their plain counterparts' own argument errors, before any GPU work."""
    lib = _lib.load()
    one, other = ctypes.c_void_p(16), ctypes.c_void_p(4096)  # never dereferenced
    arch = _arch()
    a = ctypes.byref(arch)
    h = ctypes.c_void_p()
    table = _lib.make_groups(((0, 2), (2, 4)), (1.0, 0.5), 1.0)
    good = dict(n_cap=1000, m_cap=128, chunk=256, rhs=16, d=8, ny=1, reg=1e-3, absolute=0, jitter=1e-8)

    def create(out=ctypes.byref(h), arch=a, groups=ctypes.byref(table), **kw):
        p = dict(good, **kw)
        return lib.nngp_matfree_create_additive(out, p["n_cap"], p["m_cap"], p["chunk"], p["rhs"], p["d"], p["ny"], arch, groups, p["reg"],
                                                p["absolute"], p["jitter"])

    def kmv(groups=ctypes.byref(table), out=one, ldo=8, v=other, ldv=8, r=1, x=other, n=8, d=8, arch=a, diag_add=0.0):
        return lib.nngp_kmv_additive_f64(out, ldo, v, ldv, r, x, n, d, arch, groups, diag_add, None)

    for kw, word in [(dict(groups=None), b"group table is NULL")] + [(dict(groups=ctypes.byref(t)), w) for t, w in _bad_tables()] + [
            (dict(out=None), b"NULL"), (dict(arch=None), b"NULL"), (dict(n_cap=0), b"n_cap"), (dict(m_cap=-1), b"m_cap"),
            (dict(m_cap=16385), b"m_cap"), (dict(chunk=0), b"chunk_rows"), (dict(chunk=200), b"chunk_rows"), (dict(rhs=0), b"rhs_cap"),
            (dict(rhs=4097), b"rhs_cap"), (dict(d=0), b"d >= 1"), (dict(ny=0), b"ny"), (dict(ny=17), b"ny"), (dict(jitter=-1e-9), b"jitter"),
            (dict(jitter=float("nan")), b"jitter"), (dict(reg=-1.0), b"diag_reg"), (dict(reg=float("inf")), b"diag_reg")]:
        rc = create(**kw)
        assert rc == -2 and word in lib.nngp_last_error(), (kw, rc, lib.nngp_last_error())
        assert not h.value
    for kw, word in [(dict(groups=None), b"group table is NULL")] + [(dict(groups=ctypes.byref(t)), w) for t, w in _bad_tables()] + [
            (dict(out=None), b"NULL"), (dict(v=None), b"NULL"), (dict(x=None), b"NULL"), (dict(v=one), b"aliases"), (dict(arch=None), b"arch"),
            (dict(n=0), b"n"), (dict(r=0), b"r"), (dict(d=0), b"d >= 1"), (dict(ldo=7), b"ldo"), (dict(ldv=7), b"ldv"),
            (dict(diag_add=float("nan")), b"diag_add"), (dict(diag_add=float("inf")), b"diag_add")]:
        rc = kmv(**kw)
        assert rc == -2 and word in lib.nngp_last_error(), (kw, rc, lib.nngp_last_error())
    with pytest.raises(_lib.NngpError):
        _lib.check(rc)


def test_python_refuses_the_ntk_and_the_full_covariance():
    from nngp_src_amd import matfree, matfree_additive, stax
    from nngp_src_amd.kernel_spec import KernelSpec
    spec = KernelSpec([1.0, 1.0], [0.0, 0.0], groups="pairs", input_scale=np.ones(4))
    assert matfree_additive.check_matfree_additive_spec(spec) is spec  # what check_matfree_spec refuses
    with pytest.raises(ValueError, match="NNGP"):
        matfree_additive.check_matfree_additive_spec(spec, get="ntk")
    # the constructor refuses before it looks for a device
    with pytest.raises(ValueError, match="NNGP"):
        matfree_additive.AdditiveMatrixFreeGPModel(100, 4, [1.0, 1.0], [0.0, 0.0], m=8, groups="pairs", get="ntk")
    with pytest.raises(ValueError):
        matfree_additive.AdditiveMatrixFreeGPModel(100, 4, [1.0, 1.0], [0.0, 0.0], m=8, groups=[(0, 2)], group_weights=[-1.0])
    with pytest.raises(ValueError, match="m must be"):
        matfree_additive.AdditiveMatrixFreeGPModel(100, 4, [1.0, 1.0], [0.0, 0.0], m=-1, groups="pairs")
    kernel_fn = stax.serial(stax.Dense(512), stax.Relu(), stax.Dense(1))[2].with_groups("pairs")
    with pytest.raises(ValueError, match="NNGP"):
        matfree_additive.AdditiveMatrixFreeGPModel.from_kernel_fn(kernel_fn, 100, 4, m=8, get="ntk")
    for cov in ("full", True):  # predict's covariance check is the plain model's
        with pytest.raises(ValueError, match="cov"):
            matfree.check_cov(cov)
    assert matfree_additive.AdditiveMatrixFreeGPModel.predict is matfree.MatrixFreeGPModel.predict
    # the plain model's refusals stand
    with pytest.raises(ValueError, match="groups"):
        matfree.MatrixFreeGPModel(100, 4, [1.0, 1.0], [0.0, 0.0], m=8, groups="pairs")


def test_cli_matrix_free_groups_flags_and_their_conflicts(capsys):
    from nngp_src_amd import train
    args = train.parse_args([])
    assert args.matrix_free_groups == "none" and args.matrix_free_full_weight == 1.0
    args = train.parse_args(["--matrix_free", "128", "--matrix_free_groups", "pairs", "--matrix_free_full_weight", "0.5"])
    assert (args.matrix_free, args.matrix_free_groups, args.matrix_free_full_weight) == (128, "pairs", 0.5)
    for bad in (["--matrix_free_groups", "pairs"], ["--matrix_free_full_weight", "0.5"], ["--matrix_free", "64", "--matrix_free_full_weight", "0.5"],
                ["--matrix_free", "64", "--matrix_free_groups", "pairs", "--matrix_free_full_weight", "-1"],
                ["--matrix_free", "64", "--matrix_free_groups", "triples"],
                # every conflict of --matrix_free holds with the groups
                ["--matrix_free", "64", "--matrix_free_groups", "pairs", "--sparse", "64"],
                ["--matrix_free", "64", "--matrix_free_groups", "pairs", "--kernel_type", "ntk"],
                ["--matrix_free", "64", "--matrix_free_groups", "pairs", "--loo"],
                ["--matrix_free", "64", "--matrix_free_groups", "pairs", "--tune_hyper", "5"],
                ["--matrix_free", "64", "--matrix_free_groups", "pairs", "--additive", "pairs"],
                ["--matrix_free", "64", "--matrix_free_groups", "pairs", "--full_cov"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2 and "--matrix_free" in capsys.readouterr().err, bad


def test_estimator_keyword_needs_matrix_free():
    from nngp_src_amd.estimator import Estimator
    with pytest.raises(ValueError, match="matrix_free_groups"):
        Estimator("forest", "", "", encoder=object(), matrix_free_groups="pairs")
    for kw in (dict(sparse=64), dict(kernel_type="ntk"), dict(groups="pairs")):  # the conflicts of matrix_free hold
        with pytest.raises(ValueError, match="matrix_free"):
            Estimator("forest", "", "", encoder=object(), matrix_free=64, matrix_free_groups="pairs", **kw)
