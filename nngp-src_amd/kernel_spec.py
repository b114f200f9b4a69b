"""KernelSpec: what "the kernel" is, as one immutable value.

A kernel is Dense,(act,Dense)* -- ``w_std``, ``b_std``, ``activations`` -- on features multiplied by ``input_scale``
(include/nngp_ard.h), optionally summed over feature ``groups`` with ``group_weights`` and ``full_weight``
(include/nngp_additive.h).  This module is the only place in Python that lists those attributes: ``stax.KernelFn``, the
``batch()`` wrapper, ``GPModel`` and ``SparseGPModel`` carry a ``KernelSpec`` as ``.spec`` and everything else reads it from
there.  It also holds, once, what follows from the list: validation, equality, the ctypes structs, which entry point of the C ABI
a kernel takes, and the checkpoint fields.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from . import _lib

FORMATS = ("nngp-src_amd GPModel v1", "nngp-src_amd GPModel v2")  # v1: all ReLU; v2 adds the activations


def check_input_scale(scale):
    """None, or the scale as a read-only float64 vector of finite values >= 0."""
    if scale is None:
        return None
    s = np.array(scale, dtype=np.float64)
    if s.ndim != 1 or s.shape[0] < 1 or not np.all(np.isfinite(s)) or np.any(s < 0.0):
        raise ValueError("input_scale must be one finite value >= 0 per input feature")
    s.setflags(write=False)
    return s


@dataclasses.dataclass(frozen=True, eq=False)
class KernelSpec:
    """The fields in canonical form: tuples of float, activations as ``_lib.canonical_activation`` gives them (None: all ReLU),
    ``input_scale`` None or a read-only float64 vector, ``groups`` None, "pairs" or (begin, end) ranges (``resolve(d)`` expands
    "pairs"), ``group_weights`` None or floats (None with ranges: all 1)."""
    w_std: tuple
    b_std: tuple
    activations: tuple = None
    input_scale: np.ndarray = None
    groups: tuple = None
    group_weights: tuple = None
    full_weight: float = 1.0

    def __post_init__(self):
        put = lambda name, value: object.__setattr__(self, name, value)  # noqa: E731  (frozen: the one place that writes)
        put("input_scale", check_input_scale(self.input_scale))
        if self.groups is None:
            table = (None, None, 1.0)
        elif isinstance(self.groups, str):  # the name and full_weight; the ranges come with the number of features (resolve)
            if self.groups != "pairs":
                raise ValueError("groups must be a list of (begin, end) ranges or 'pairs', got %r" % (self.groups,))
            table = ("pairs", None, float(self.full_weight))
            if not (np.isfinite(table[2]) and table[2] >= 0.0):
                raise ValueError("group weights and full_weight must be finite and >= 0")
            if self.group_weights is not None:
                raise ValueError("groups='pairs' takes no weights: give the ranges (stax.pair_groups(d)) to weight them")
        else:
            table = _lib.check_groups(self.groups, self.group_weights, self.full_weight)
        for name, value in zip(("groups", "group_weights", "full_weight"), table):
            put(name, value)
        put("w_std", tuple(float(w) for w in self.w_std))
        put("b_std", tuple(float(b) for b in self.b_std))
        acts = [("relu",)] * self.n_relu if self.activations is None else list(self.activations)
        if len(acts) != self.n_relu:
            raise ValueError("%d Dense layers need %d activations" % (self.n_dense, self.n_relu))
        # per hidden layer: ("relu",), ("abrelu", a, b) or ("erf", a, b, c); ABRelu(0, 1) is stored as ("relu",)
        put("activations", tuple(_lib.canonical_activation(a) for a in acts))

    @classmethod
    def of(cls, obj):
        """The spec of a KernelSpec, of anything that carries one as ``.spec`` (a stax.KernelFn, a batch() wrapper, a model) or
        of a (w_std, b_std[, activations]) tuple."""
        if isinstance(obj, cls):
            return obj
        if hasattr(obj, "spec"):
            return obj.spec
        return cls(obj[0], obj[1], obj[2] if len(obj) > 2 else None)

    def replace(self, **changes):
        """A copy with these fields given anew (and checked like the constructor's)."""
        return dataclasses.replace(self, **changes)

    def as_keywords(self) -> dict:
        """The fields by name: the kernel keywords of GPModel / SparseGPModel."""
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}

    def resolve(self, d):
        """This spec bound to d features: "pairs" expanded, the ranges checked against d, the scale's length too."""
        d = int(d)
        if self.input_scale is not None and self.input_scale.shape[0] != d:
            raise ValueError("input_scale has %d values, the model has d = %d" % (self.input_scale.shape[0], d))
        if self.groups is None:
            return self
        groups, weights, full_weight = _lib.check_groups(self.groups, self.group_weights, self.full_weight, d=d)
        return self.replace(groups=groups, group_weights=weights, full_weight=full_weight)

    # ---- value semantics: two specs that reach the device as the same kernel are equal once resolved ----
    def _but_scale(self):
        return (self.w_std, self.b_std, self.activations, self.groups, self.group_weights, self.full_weight)

    def __eq__(self, other):
        if not isinstance(other, KernelSpec):
            return NotImplemented
        a, b = self.input_scale, other.input_scale
        same_scale = (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))
        return same_scale and self._but_scale() == other._but_scale()

    def __hash__(self):
        return hash(self._but_scale() + (None if self.input_scale is None else tuple(self.input_scale.tolist()),))

    # ---- derived values ----
    @property
    def n_dense(self) -> int:
        return len(self.w_std)

    @property
    def n_relu(self) -> int:
        return self.n_dense - 1  # hidden layers (the name is the all-ReLU one)

    @property
    def all_relu(self) -> bool:
        return _lib.all_relu(self.activations)

    def arch(self) -> _lib.NngpArch:
        return _lib.make_arch(self.w_std, self.b_std)

    def arch_act(self) -> _lib.NngpArchAct:
        return _lib.make_arch_act(self.w_std, self.b_std, self.activations)

    def group_table(self):
        """None without groups, else their nngp_groups ("pairs" has none before resolve(d))."""
        if self.groups is None:
            return None
        return _lib.make_groups(*_lib.check_groups(self.groups, self.group_weights, self.full_weight))

    def scale(self, xd):
        """xd [n, d] (device float64, or None) times the input scale, feature by feature, on xd's device."""
        if self.input_scale is None or xd is None:
            return xd
        import torch
        if int(xd.shape[1]) != self.input_scale.shape[0]:
            raise ValueError("input_scale has %d values, x has %d features" % (self.input_scale.shape[0], int(xd.shape[1])))
        return xd * torch.tensor(self.input_scale, dtype=torch.float64, device=xd.device)

    def require_plain_relu(self, who):
        """NotImplementedError from the multi-GPU layouts, which take the plain ReLU architecture only."""
        if self.input_scale is not None:
            raise NotImplementedError("%s does not take an input_scale (per-feature relevances are single-GPU)" % who)
        if not self.all_relu:  # their row / tile operations take the ReLU architecture only
            raise NotImplementedError("%s supports Dense,(Relu,Dense)* networks only, got activations %r" % (who, self.activations))

    # ---- which entry point of the C ABI this kernel takes; ``lib`` is the loaded library (or a stand-in for it) ----
    def _entry(self, lib, stem, d):
        """(entry point, its architecture arguments): groups (an empty table counts) take ``<stem>_additive`` with the
        activation struct and the table, an all-ReLU network the base entry point with nngp_arch -- the only one the host build of
        the ABI has -- and any other ``<stem>_act``."""
        spec = self.resolve(d)
        table = spec.group_table()
        if table is not None:
            return getattr(lib, stem + "_additive"), (ctypes.byref(spec.arch_act()), ctypes.byref(table))
        if spec.all_relu:
            return getattr(lib, stem), (ctypes.byref(spec.arch()),)
        return getattr(lib, stem + "_act"), (ctypes.byref(spec.arch_act()),)

    def kernel_build(self, lib, x1, n1, x2, n2, d, *rest):
        """nngp_kernel_build[_act|_additive](x1, n1, x2, n2, d, <arch>, *rest); returns its status."""
        fn, arch = self._entry(lib, "nngp_kernel_build", d)
        return fn(x1, n1, x2, n2, d, *arch, *rest)

    def model_create(self, lib, handle, n_cap, m_cap, d, ny, *rest):
        """nngp_model_create[_act|_additive](handle, n_cap, m_cap, d, ny, <arch>, *rest); returns its status."""
        fn, arch = self._entry(lib, "nngp_model_create", d)
        return fn(handle, n_cap, m_cap, d, ny, *arch, *rest)

    def sparse_create(self, lib, handle, m_cap, chunk_rows, test_cap, d, ny, *rest):
        """nngp_sparse_create(handle, m_cap, chunk_rows, test_cap, d, ny, <arch_act>, <table or NULL>, *rest); its status."""
        spec = self.resolve(d)
        table = spec.group_table()
        return lib.nngp_sparse_create(handle, m_cap, chunk_rows, test_cap, d, ny, ctypes.byref(spec.arch_act()),
                                      None if table is None else ctypes.byref(table), *rest)

    # ---- checkpoint fields (GPModel.save / load) ----
    def to_fields(self) -> dict:
        """The kernel's fields of a checkpoint.  An all-ReLU kernel writes v1, any other v2 with the activations as
        (code, a, b, c) rows; input_scale and the group table are written only when present."""
        out = {"format": np.array(FORMATS[0] if self.all_relu else FORMATS[1]), "w_std": np.array(self.w_std),
               "b_std": np.array(self.b_std)}
        if not self.all_relu:
            out["activations"] = np.array([[_lib.ACTIVATIONS[a[0]][0]] + list(a[1:]) + [0.0] * (4 - len(a)) for a in self.activations],
                                          dtype=np.float64).reshape(-1, 4)
        if self.input_scale is not None:
            out["input_scale"] = np.array(self.input_scale)
        if self.groups is not None:
            groups, weights, full_weight = _lib.check_groups(self.groups, self.group_weights, self.full_weight)
            out.update(groups=np.array(groups, dtype=np.int64).reshape(-1, 2), group_weights=np.array(weights, dtype=np.float64),
                       full_weight=np.array(full_weight))
        return out

    @classmethod
    def from_fields(cls, z, name="checkpoint"):
        """The spec of a loaded checkpoint ``z`` (numpy's NpzFile); a file without the optional fields is the plain kernel."""
        fmt = str(z["format"])
        if fmt not in FORMATS:
            raise _lib.NngpError("load: %s is not a GPModel checkpoint" % name)
        acts = None
        if fmt == FORMATS[1]:
            kinds = {code: (kind, nparams) for kind, (code, nparams) in _lib.ACTIVATIONS.items()}
            acts = []
            for row in z["activations"]:
                if int(row[0]) not in kinds:
                    raise _lib.NngpError("load: %s: unknown activation code %r" % (name, row[0]))
                kind, nparams = kinds[int(row[0])]
                acts.append((kind,) + tuple(float(v) for v in row[1:1 + nparams]))
        grouped = {}
        if "groups" in z.files:
            grouped = dict(groups=[(int(b), int(e)) for b, e in z["groups"]], group_weights=[float(v) for v in z["group_weights"]],
                           full_weight=float(z["full_weight"]))
        return cls(z["w_std"].tolist(), z["b_std"].tolist(), acts, z["input_scale"] if "input_scale" in z.files else None, **grouped)


# what a kernel_fn, a batch() wrapper and the models expose by name: the fields and the derived values callers read
ATTRIBUTES = tuple(f.name for f in dataclasses.fields(KernelSpec)) + ("n_relu", "all_relu")


class HasSpec:
    """Read-only access to ``self.spec``'s ATTRIBUTES under their own names."""


for _name in ATTRIBUTES:
    setattr(HasSpec, _name, property(lambda self, _name=_name: getattr(self.spec, _name)))
