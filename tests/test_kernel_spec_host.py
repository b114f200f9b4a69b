"""KernelSpec without a GPU and without the library: canonical form and equality, the checks it took over from KernelFn / GPModel /
apply_input_scale, KernelSpec.of, which entry point of the C ABI each kind of kernel takes (on a recording stand-in for the
library), the checkpoint fields, and that no other module collects a kernel_fn's attributes by hand."""
import os
import re

import numpy as np
import pytest

from nngp_src_amd import _lib, batch, stax
from nngp_src_amd.kernel_spec import ATTRIBUTES, KernelSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, B = [1.1, 0.9], [0.2, 0.1]
W3, B3 = [1.1, 1.0, 0.9], [0.2, 0.05, 0.1]
D = 6
# name: (w_std, b_std, activations, group keywords)
KINDS = {
    "relu": (W, B, None, {}),
    "abrelu_erf": (W3, B3, [("abrelu", 0.1, 1.0), ("erf", 1.0, 1.0, 0.0)], {}),
    "relu_empty_groups": (W, B, None, dict(groups=[])),
    "erf_pairs": (W, B, [("erf", 1.0, 1.0, 0.0)], dict(groups="pairs", full_weight=0.5)),
}
SUFFIX = {"relu": "", "abrelu_erf": "_act", "relu_empty_groups": "_additive", "erf_pairs": "_additive"}


def test_canonical_form_and_equality():
    pairs = KernelSpec(W, B, groups="pairs").resolve(D)
    assert pairs.groups == stax.pair_groups(D) and pairs.group_weights == (1.0,) * 3 and pairs.full_weight == 1.0
    for weights in (None, [1.0] * 3):
        explicit = KernelSpec(W, B, groups=stax.pair_groups(D), group_weights=weights)
        assert explicit == pairs and explicit.resolve(D) == pairs and hash(explicit) == hash(pairs)
    assert KernelSpec(W, B, groups="pairs") != pairs  # not bound to a number of features yet
    assert KernelSpec(W, B, groups=stax.pair_groups(D), group_weights=[1.0, 1.0, 2.0]) != pairs
    assert KernelSpec(W, B, groups="pairs", full_weight=0.5).resolve(D) != pairs
    assert KernelSpec(W, B, groups=[], full_weight=2.0).groups == () and KernelSpec(W, B, groups=[]) != KernelSpec(W, B)
    assert KernelSpec(W, B, full_weight=3.0).full_weight == 1.0  # without groups there is no full_weight to carry

    relu = KernelSpec(W, B)
    assert relu.activations == (("relu",),) and relu.all_relu and relu.n_dense == 2 and relu.n_relu == 1
    assert KernelSpec(W, B, [("abrelu", 0, 1)]) == relu and hash(KernelSpec(W, B, [("abrelu", 0.0, 1.0)])) == hash(relu)
    assert KernelSpec(W, B, [("abrelu", 0.1, 1.0)]) != relu and not KernelSpec(W, B, [("abrelu", 0.1, 1.0)]).all_relu
    assert KernelSpec(tuple(W), np.array(B)) == relu and KernelSpec([1.1, 0.8], B) != relu
    assert type(relu.w_std) is tuple and type(relu.b_std) is tuple and relu != (W, B)

    s = [1.0, 0.0, 2.5, 0.5, 1.5, 0.7]
    a, b = relu.replace(input_scale=s), relu.replace(input_scale=np.array(s))
    assert a == b and hash(a) == hash(b) and a != relu and relu != a
    assert a.input_scale.dtype == np.float64 and not a.input_scale.flags.writeable
    for k in range(D):
        other = list(s)
        other[k] += 1e-9
        assert relu.replace(input_scale=other) != a
    assert relu.replace(input_scale=s[:5]) != a
    assert a.replace(input_scale=None) == relu
    assert len({relu, KernelSpec(W, B), a, b, pairs}) == 3
    with pytest.raises(Exception):
        relu.w_std = (1.0, 1.0)  # immutable


def test_the_spec_raises_what_kernel_fn_and_the_models_raised():
    with pytest.raises(ValueError, match="even number of features"):
        KernelSpec(W, B, groups="pairs").resolve(5)
    with pytest.raises(ValueError, match=r"group range \[0, 8\) is outside"):
        KernelSpec(W, B, groups=[(0, 8)]).resolve(7)
    with pytest.raises(ValueError, match="all weights are zero"):
        KernelSpec(W, B, groups=[(0, 2)], group_weights=[0.0], full_weight=0.0)
    with pytest.raises(ValueError, match="all weights are zero"):
        KernelSpec(W, B, groups=[], full_weight=0.0)
    with pytest.raises(ValueError, match="must be finite and >= 0"):
        KernelSpec(W, B, groups="pairs", full_weight=-1.0)
    assert KernelSpec(W, B, groups="pairs", full_weight=0.0).resolve(4).full_weight == 0.0  # the pairs alone
    with pytest.raises(ValueError, match="or 'pairs'"):
        KernelSpec(W, B, groups="triples")
    with pytest.raises(ValueError, match="groups='pairs' takes no weights"):
        KernelSpec(W, B, groups="pairs", group_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="2 Dense layers need 1 activations"):
        KernelSpec(W, B, [("relu",), ("relu",)])
    with pytest.raises(ValueError, match="unknown activation"):
        KernelSpec(W, B, [("tanh",)])
    for bad in ([1.0, -0.1], [1.0, float("nan")], [float("inf")], [[1.0, 2.0]], []):
        with pytest.raises(ValueError, match="input_scale must be one finite value >= 0 per input feature"):
            KernelSpec(W, B, input_scale=bad)
    scaled = KernelSpec(W, B, input_scale=[1.0, 2.0, 3.0, 4.0, 5.0])
    with pytest.raises(ValueError, match="input_scale has 5 values, the model has d = 6"):
        scaled.resolve(D)
    import torch
    with pytest.raises(ValueError, match="input_scale has 5 values, x has 6 features"):
        scaled.scale(torch.zeros((3, D), dtype=torch.float64))
    x = torch.arange(10, dtype=torch.float64).reshape(2, 5)
    assert torch.equal(scaled.scale(x), x * torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64))
    assert scaled.scale(None) is None and KernelSpec(W, B).scale(x) is x
    # the same errors through the front end that holds a spec
    _, _, kf = stax.serial(stax.Dense(8), stax.Relu(), stax.Dense(1))
    with pytest.raises(ValueError, match="takes no weights"):
        kf.with_groups("pairs", weights=[1.0])
    with pytest.raises(ValueError, match="even number"):
        kf.with_groups("pairs").group_table(5)
    with pytest.raises(NotImplementedError, match="shard32 does not take an input_scale"):
        scaled.require_plain_relu("shard32")
    with pytest.raises(NotImplementedError, match=r"grid2d supports Dense,\(Relu,Dense\)\* networks only"):
        KernelSpec(W, B, [("erf", 1.0, 1.0, 0.0)]).require_plain_relu("grid2d")
    KernelSpec(W, B, [("abrelu", 0.0, 1.0)]).require_plain_relu("grid2d")


def test_of_gives_the_same_spec_for_every_carrier():
    acts = [("abrelu", 0.1, 1.0)]
    kf = stax.KernelFn(W, B, acts, input_scale=[1.0, 0.0, 2.5, 1.0], groups="pairs", full_weight=0.5)
    spec = KernelSpec.of(kf)
    assert spec is kf.spec and KernelSpec.of(spec) is spec
    batched = batch(kf, batch_size=4, device_count=0)
    assert batched is not kf and batched.spec is spec and KernelSpec.of(batched) is spec
    assert batch(kf, 0, 0) is kf and KernelSpec.of(batch(kf, 0, 0)) is spec
    for name in ATTRIBUTES:  # the names callers read, on the kernel_fn and on the wrapper
        assert np.array_equal(getattr(kf, name), getattr(spec, name)) and np.array_equal(getattr(batched, name), getattr(spec, name))
    assert set(ATTRIBUTES) == {"w_std", "b_std", "activations", "input_scale", "groups", "group_weights", "full_weight", "n_relu",
                               "all_relu"}
    with pytest.raises(AttributeError):
        kf.input_scale = None  # read-only: a copy comes from with_input_scale
    assert KernelSpec.of((W, B)) == KernelSpec(W, B) == KernelSpec.of(stax.KernelFn(W, B))
    assert KernelSpec.of((W, B, acts)) == KernelSpec(W, B, acts) == spec.replace(input_scale=None, groups=None)
    assert KernelSpec.of((W, B, None)) == KernelSpec(W, B)
    assert kf.with_input_scale(None).spec == spec.replace(input_scale=None)
    assert kf.with_groups(None).spec == spec.replace(groups=None) and kf.with_groups(None).full_weight == 1.0
    assert KernelSpec(**spec.as_keywords()) == spec


class _Recorder:
    """Stands in for the loaded library: every attribute is an entry point that records (name, args) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _struct(arg):
    return arg._obj  # what ctypes.byref(...) refers to


def _check_table(arg, groups, weights, full_weight):
    if groups is None:
        assert arg is None  # NULL
        return
    got, want = _struct(arg), _lib.make_groups(*_lib.check_groups(groups, weights, full_weight, d=D))
    assert type(got) is _lib.NngpGroups and got.n_groups == want.n_groups and got.full_weight == want.full_weight
    for field in ("begin", "end", "weight"):
        assert [getattr(got, field)[i] for i in range(want.n_groups)] == [getattr(want, field)[i] for i in range(want.n_groups)]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_abi_dispatch_on_a_recording_library(kind):
    w, b, acts, grouped = KINDS[kind]
    spec = KernelSpec(w, b, acts, **grouped)
    groups, full_weight = grouped.get("groups"), grouped.get("full_weight", 1.0)
    plain = _lib.make_arch(w, b)
    act = _lib.make_arch_act(w, b, acts or [("relu",)] * (len(w) - 1))
    want_arch = plain if SUFFIX[kind] == "" else act
    lib = _Recorder()
    assert spec.kernel_build(lib, "x1", 7, "x2", 5, D, _lib.DTYPE_F64, "nngp", "ntk", 5, 0, 7, "stream") == 0
    assert spec.model_create(lib, "handle", 130, 5, D, 1, _lib.GET_NTK, 1e-3, 0) == 0
    assert spec.sparse_create(lib, "handle", 128, 128, 1024, D, 1, 1e-3, 0, 1e-8) == 0
    (build, a_build), (create, a_create), (sparse, a_sparse) = lib.calls
    assert build == "nngp_kernel_build" + SUFFIX[kind] and create == "nngp_model_create" + SUFFIX[kind]
    assert sparse == "nngp_sparse_create"
    for args, head in ((a_build, ("x1", 7, "x2", 5, D)), (a_create, ("handle", 130, 5, D, 1))):
        assert args[:5] == head
        assert type(_struct(args[5])) is type(want_arch) and bytes(_struct(args[5])) == bytes(want_arch)
        tail = args[6:]
        if groups is not None:
            _check_table(args[6], groups, None, full_weight)
            tail = args[7:]
        assert tail == ((_lib.DTYPE_F64, "nngp", "ntk", 5, 0, 7, "stream") if args is a_build else (_lib.GET_NTK, 1e-3, 0))
    assert a_sparse[:6] == ("handle", 128, 128, 1024, D, 1) and a_sparse[8:] == (1e-3, 0, 1e-8)
    assert type(_struct(a_sparse[6])) is _lib.NngpArchAct and bytes(_struct(a_sparse[6])) == bytes(act)  # always the _act struct
    _check_table(a_sparse[7], groups, None, full_weight)
    # stax.KernelFn and its struct helper follow the same rule
    kf = stax.KernelFn(w, b, acts, **grouped)
    assert type(kf._arch()) is (_lib.NngpArch if kf.all_relu else _lib.NngpArchAct)


def test_dispatch_refuses_what_does_not_fit_the_features():
    lib = _Recorder()
    with pytest.raises(ValueError, match="even number"):
        KernelSpec(W, B, groups="pairs").model_create(lib, "handle", 10, 0, 5, 1, _lib.GET_NNGP, 1e-3, 0)
    with pytest.raises(ValueError, match="the model has d = 6"):
        KernelSpec(W, B, input_scale=[1.0, 2.0]).sparse_create(lib, "handle", 128, 128, 1024, D, 1, 1e-3, 0, 1e-8)
    with pytest.raises(ValueError, match="needs the number of features"):
        KernelSpec(W, B, groups="pairs").group_table()
    assert lib.calls == [] and KernelSpec(W, B).group_table() is None


def test_checkpoint_fields_are_what_save_wrote(tmp_path):
    """Key sets and dtypes as GPModel.save wrote them before the spec existed."""
    plain = KernelSpec(W, B).to_fields()
    assert set(plain) == {"format", "w_std", "b_std"} and str(plain["format"]) == "nngp-src_amd GPModel v1"
    assert plain["w_std"].dtype == np.float64 and plain["w_std"].tolist() == W and plain["b_std"].tolist() == B
    assert plain["format"].dtype.kind == "U" and plain["format"].shape == ()

    acts = [("abrelu", 0.1, 1.0), ("erf", 0.5, 2.0, 0.25)]
    v2 = KernelSpec(W3, B3, acts).to_fields()
    assert set(v2) == {"format", "w_std", "b_std", "activations"} and str(v2["format"]) == "nngp-src_amd GPModel v2"
    assert v2["activations"].dtype == np.float64 and v2["activations"].shape == (2, 4)
    assert v2["activations"].tolist() == [[_lib.ACT_ABRELU, 0.1, 1.0, 0.0], [_lib.ACT_ERF, 0.5, 2.0, 0.25]]
    mixed = KernelSpec(W3, B3, [("relu",), ("erf", 1.0, 1.0, 0.0)]).to_fields()["activations"]
    assert mixed.tolist() == [[_lib.ACT_RELU, 0.0, 0.0, 0.0], [_lib.ACT_ERF, 1.0, 1.0, 0.0]]

    full = KernelSpec(W, B, input_scale=[1.0, 0.0, 2.5, 1.0], groups=[(0, 2), (1, 4)], group_weights=[1.0, 0.3], full_weight=0.25)
    f = full.to_fields()
    assert set(f) == {"format", "w_std", "b_std", "input_scale", "groups", "group_weights", "full_weight"}
    assert str(f["format"]) == "nngp-src_amd GPModel v1"  # the version follows the activations alone
    assert f["groups"].dtype == np.int64 and f["groups"].tolist() == [[0, 2], [1, 4]]
    assert f["group_weights"].dtype == np.float64 and f["group_weights"].tolist() == [1.0, 0.3]
    assert f["full_weight"].dtype == np.float64 and f["full_weight"].shape == () and float(f["full_weight"]) == 0.25
    assert f["input_scale"].dtype == np.float64 and f["input_scale"].tolist() == [1.0, 0.0, 2.5, 1.0]
    empty = KernelSpec(W, B, groups=[], full_weight=2.0).to_fields()
    assert empty["groups"].shape == (0, 2) and empty["groups"].dtype == np.int64 and empty["group_weights"].shape == (0,)

    path = str(tmp_path / "m.npz")
    for spec in (KernelSpec(W, B), KernelSpec(W3, B3, acts), full, KernelSpec(W, B, groups=[], full_weight=2.0),
                 KernelSpec(W, B, [("erf", 1.0, 1.0, 0.0)], groups="pairs", full_weight=0.5).resolve(D)):
        np.savez(path, x=np.zeros((2, 4)), **spec.to_fields())
        assert KernelSpec.from_fields(np.load(path, allow_pickle=False)) == spec
    # a file with the v1 keys only, as the first version of save wrote it
    np.savez(path, format=np.array("nngp-src_amd GPModel v1"), x=np.zeros((2, 4)), y=np.zeros((2, 1)), w_std=np.array(W),
             b_std=np.array(B), get=np.array("nngp"))
    assert KernelSpec.from_fields(np.load(path, allow_pickle=False)) == KernelSpec(W, B)
    np.savez(path, format=np.array("something else"), w_std=np.array(W), b_std=np.array(B))
    with pytest.raises(_lib.NngpError, match="m.npz is not a GPModel checkpoint"):
        KernelSpec.from_fields(np.load(path, allow_pickle=False), "m.npz")
    np.savez(path, format=np.array("nngp-src_amd GPModel v2"), w_std=np.array(W), b_std=np.array(B),
             activations=np.array([[7.0, 0.0, 0.0, 0.0]]))
    with pytest.raises(_lib.NngpError, match="unknown activation code"):
        KernelSpec.from_fields(np.load(path, allow_pickle=False))


def test_make_arch_act_and_the_checkpoint_share_one_code_table():
    assert _lib.ACTIVATIONS == {"relu": (_lib.ACT_RELU, 0), "abrelu": (_lib.ACT_ABRELU, 2), "erf": (_lib.ACT_ERF, 3)}
    arch = _lib.make_arch_act(W3, B3, [("abrelu", 0.1, 1.0), ("erf", 0.5, 2.0, 0.25)])
    assert [arch.act[0], arch.act[1]] == [_lib.ACT_ABRELU, _lib.ACT_ERF]
    assert list(arch.p[0])[:2] == [0.1, 1.0] and list(arch.p[1]) == [0.5, 2.0, 0.25]


def test_only_kernel_spec_collects_a_kernel_fns_attributes():
    """The point of KernelSpec: no consumer picks the attributes off a kernel_fn one by one, and the list of them exists once."""
    src = os.path.join(ROOT, "nngp-src_amd")
    names = ("w_std", "b_std", "activations", "input_scale", "groups", "group_weights", "full_weight")
    modules = sorted(f for f in os.listdir(src) if f.endswith(".py"))
    assert "kernel_spec.py" in modules and len(modules) > 10
    for module in modules:
        with open(os.path.join(src, module)) as f:
            text = f.read()
        if module == "kernel_spec.py":
            continue
        assert not re.search(r"getattr\(\s*kernel_fn", text), module
        # the seven names as quoted strings, as a hand-written list of them would have them
        assert not all(re.search(r"[\"']%s[\"']" % n, text) for n in names), module
