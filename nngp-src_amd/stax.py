"""``stax``-shaped front end of the closed-form NNGP/NTK kernel (reference call sites:
train.py:161-164, estimator.py:27-30, active/active_train.py:40-43).

    init_fn, apply_fn, kernel_fn = stax.serial(stax.Dense(512), stax.Relu(), stax.Dense(1))
    k = kernel_fn(x1, x2, 'nngp')          # computed by the HIP kernel build (nngp_kernel_build)

Supported topology: Dense, (act, Dense)* with act one of Relu (what the reference builds), Erf, ABRelu,
LeakyRelu and Abs, chosen per hidden layer; widths do not enter the infinite-width kernel.  An all-ReLU
network takes the ReLU entry points of include/nngp_hip.h, any other the ``_act`` entry points of
include/nngp_activations.h.  ``init_fn`` / ``apply_fn`` are the finite-width network in NumPy (NTK
parameterisation); the reference never calls them, the tests use them as a Monte Carlo pin.
"""
from __future__ import annotations

import collections
import ctypes
import math

import numpy as np

from . import _lib

Kernel = collections.namedtuple("Kernel", ["nngp", "ntk"])
_Layer = collections.namedtuple("_Layer", ["kind", "out_dim", "w_std", "b_std", "act"], defaults=(None,))


def Dense(out_dim, W_std=1.0, b_std=None, parameterization="ntk"):
    if parameterization != "ntk":
        raise NotImplementedError("only the NTK parameterisation (the reference's default) is supported")
    return _Layer("dense", int(out_dim), float(W_std), 0.0 if b_std is None else float(b_std))


def _act(spec):
    for v in spec[1:]:
        if not math.isfinite(v):
            raise ValueError("activation parameters must be finite, got %r" % (spec,))
    return _Layer(spec[0], None, None, None, spec)


# do_stabilize (neural-tangents' rescaling for numerical range) is accepted and ignored: the float64 closed forms need none.
def Relu(do_stabilize=False):
    return _act(("relu",))


def ABRelu(a, b, do_stabilize=False):
    """phi(x) = a x for x < 0, b x for x >= 0."""
    return _act(("abrelu", float(a), float(b)))


def LeakyRelu(alpha, do_stabilize=False):
    return _act(("abrelu", float(alpha), 1.0))


def Abs(do_stabilize=False):
    return _act(("abrelu", -1.0, 1.0))


def Erf(a=1.0, b=1.0, c=0.0):
    """phi(x) = a erf(b x) + c."""
    return _act(("erf", float(a), float(b), float(c)))


def _phi(spec, h):
    if spec[0] == "relu":
        return np.maximum(h, 0.0)
    if spec[0] == "abrelu":
        return np.where(h < 0.0, spec[1] * h, spec[2] * h)
    import torch
    return spec[1] * torch.special.erf(torch.from_numpy(spec[2] * h)).numpy() + spec[3]


def check_input_scale(scale):
    """None, or the scale as a float64 vector of finite values >= 0."""
    if scale is None:
        return None
    s = np.array(scale, dtype=np.float64)
    if s.ndim != 1 or s.shape[0] < 1 or not np.all(np.isfinite(s)) or np.any(s < 0.0):
        raise ValueError("input_scale must be one finite value >= 0 per input feature")
    s.setflags(write=False)
    return s


def apply_input_scale(scale, xd):
    """xd [n, d] (device float64, or None) times the scale, feature by feature, on xd's device."""
    if scale is None or xd is None:
        return xd
    import torch
    if int(xd.shape[1]) != scale.shape[0]:
        raise ValueError("input_scale has %d values, x has %d features" % (scale.shape[0], int(xd.shape[1])))
    return xd * torch.tensor(scale, dtype=torch.float64, device=xd.device)


class KernelFn:
    """kernel_fn(x1, x2=None, get=None): closed-form kernel of Dense,(act,Dense)* on the GPU."""

    def __init__(self, w_std, b_std, activations=None, input_scale=None, groups=None, group_weights=None, full_weight=1.0):
        """input_scale: None or d values >= 0 that multiply the features of x1 and x2 on the device before the build --
        sqrt of the relevances of include/nngp_ard.h (with_input_scale returns a copy that carries them).
        groups: None, "pairs" or (begin, end) feature ranges -- the additive kernel of include/nngp_additive.h,
        full_weight K(x, x') + sum_g group_weights[g] K(x_g, x'_g) (with_groups returns a copy that carries them)."""
        self.input_scale = check_input_scale(input_scale)
        if groups is None:
            self.groups, self.group_weights, self.full_weight = None, None, 1.0
        elif isinstance(groups, str):
            _lib.check_groups(groups, None, full_weight, d=2)  # the name and full_weight; the table is made per call, from d
            self.groups, self.group_weights, self.full_weight = groups, None, float(full_weight)
            if group_weights is not None:
                raise ValueError("groups='pairs' takes no weights: give the ranges (stax.pair_groups(d)) to weight them")
        else:
            self.groups, self.group_weights, self.full_weight = _lib.check_groups(groups, group_weights, full_weight)
        self.w_std = tuple(float(w) for w in w_std)
        self.b_std = tuple(float(b) for b in b_std)
        self.n_relu = len(self.w_std) - 1  # hidden layers (the name is the all-ReLU one)
        acts = [("relu",)] * self.n_relu if activations is None else list(activations)
        if len(acts) != self.n_relu:
            raise ValueError("%d Dense layers need %d activations" % (len(self.w_std), self.n_relu))
        # per hidden layer: ("relu",), ("abrelu", a, b) or ("erf", a, b, c); ABRelu(0, 1) is stored as ("relu",)
        self.activations = tuple(_lib.canonical_activation(a) for a in acts)
        self.all_relu = _lib.all_relu(self.activations)

    def with_input_scale(self, scale):
        """A copy of this kernel_fn with ``input_scale = scale`` (None: without one)."""
        return KernelFn(self.w_std, self.b_std, self.activations, scale, self.groups, self.group_weights, self.full_weight)

    def with_groups(self, groups, weights=None, full_weight=1.0):
        """A copy of this kernel_fn with the additive kernel over ``groups`` (None: the plain kernel again)."""
        return KernelFn(self.w_std, self.b_std, self.activations, self.input_scale, groups, weights, full_weight)

    def group_table(self, d):
        """None, or (groups, weights, full_weight) checked against d features."""
        if self.groups is None:
            return None
        return _lib.check_groups(self.groups, self.group_weights, self.full_weight, d=d)

    def _arch(self):
        if self.all_relu:
            return _lib.make_arch(self.w_std, self.b_std)
        return _lib.make_arch_act(self.w_std, self.b_std, self.activations)

    def __call__(self, x1, x2=None, get=None, *, rows=None, as_numpy=True):
        import torch
        lib = _lib.load()
        dev = _lib.require_gpu()
        gets = ("nngp", "ntk") if get is None else ((get,) if isinstance(get, str) else tuple(get))
        for g in gets:
            if g not in ("nngp", "ntk"):
                raise ValueError("get must be 'nngp', 'ntk' or a tuple of them, got %r" % (get,))
        x1d = _lib.to_device_f64(x1, dev)
        if x1d.ndim != 2:
            raise ValueError("x1 must be [N, d]")
        x2d = None if x2 is None else _lib.to_device_f64(x2, dev)
        if x2d is not None and (x2d.ndim != 2 or x2d.shape[1] != x1d.shape[1]):
            raise ValueError("x2 must be [N2, d] with the same d as x1")
        n1, d = int(x1d.shape[0]), int(x1d.shape[1])
        n2 = n1 if x2d is None else int(x2d.shape[0])
        if self.input_scale is not None:
            x1d, x2d = apply_input_scale(self.input_scale, x1d), apply_input_scale(self.input_scale, x2d)
        r0, r1 = (0, n1) if rows is None else (int(rows[0]), int(rows[1]))
        outs = {g: torch.empty((n1, n2), dtype=torch.float64, device=dev) for g in set(gets)}
        if n1 > 0 and n2 > 0 and r1 > r0:
            table = self.group_table(d)
            if table is not None:
                arch = _lib.make_arch_act(self.w_std, self.b_std, self.activations)
                gr = _lib.make_groups(*table)
                _lib.check(lib.nngp_kernel_build_additive(_lib.ptr(x1d), n1, _lib.ptr(x2d), n2, d, ctypes.byref(arch),
                                                          ctypes.byref(gr), _lib.DTYPE_F64, _lib.ptr(outs.get("nngp")),
                                                          _lib.ptr(outs.get("ntk")), n2, r0, r1, _lib.stream_ptr()))
            else:
                arch = self._arch()
                build = lib.nngp_kernel_build if self.all_relu else lib.nngp_kernel_build_act
                _lib.check(build(_lib.ptr(x1d), n1, _lib.ptr(x2d), n2, d, ctypes.byref(arch),
                                                 _lib.DTYPE_F64, _lib.ptr(outs.get("nngp")), _lib.ptr(outs.get("ntk")),
                                                 n2, r0, r1, _lib.stream_ptr()))
        res = {g: (t[r0:r1] if rows is not None else t) for g, t in outs.items()}
        if as_numpy:
            res = {g: t.cpu().numpy() for g, t in res.items()}
        if get is None:
            return Kernel(res["nngp"], res["ntk"])
        if isinstance(get, str):
            return res[get]
        return collections.namedtuple("Kernel", gets)(*[res[g] for g in gets])


pair_groups = _lib.pair_groups


def additive(layers, groups, weights=None, full_weight=1.0):
    """serial(*layers) with the additive kernel over feature groups: (init_fn, apply_fn, kernel_fn), where
    kernel_fn(x, x') = full_weight K(x, x') + sum_g weights[g] K(x[:, b_g:e_g], x'[:, b_g:e_g]) and K is serial(*layers)'s
    kernel (include/nngp_additive.h).  groups: (begin, end) ranges, or "pairs".  init_fn / apply_fn are those of one
    network of the sum."""
    init_fn, apply_fn, kernel_fn = serial(*layers)
    return init_fn, apply_fn, kernel_fn.with_groups(groups, weights, full_weight)


def serial(*layers):
    """Dense,(act,Dense)* -> (init_fn, apply_fn, kernel_fn); act: Relu, Erf, ABRelu, LeakyRelu or Abs."""
    if not layers or any(not isinstance(l, _Layer) for l in layers):
        raise TypeError("serial() takes stax.Dense(...) and activation layers (stax.Relu(), stax.Erf(), ...)")
    kinds = [l.kind for l in layers]
    ok = len(kinds) % 2 == 1 and all((k == "dense") == (i % 2 == 0) for i, k in enumerate(kinds))
    if not ok:
        raise NotImplementedError("supported topology is Dense,(act,Dense)* with act one of Relu, Erf, ABRelu, "
                                  "LeakyRelu, Abs -- got %s" % kinds)
    dense = [l for l in layers if l.kind == "dense"]
    acts = [l.act for l in layers[1::2]]
    kernel_fn = KernelFn([l.w_std for l in dense], [l.b_std for l in dense], acts)

    def init_fn(rng, input_shape):
        gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        fan_in, params = int(input_shape[-1]), []
        for l in dense:
            params.append((gen.standard_normal((fan_in, l.out_dim)), gen.standard_normal((l.out_dim,))))
            fan_in = l.out_dim
        return tuple(input_shape[:-1]) + (fan_in,), params

    def apply_fn(params, x, readout=True):
        """The finite-width network.  readout=False: the last hidden layer's activations instead of the output (the
        features the last Dense layer reads; their Gram matrix w_std^2 phi phi^T / width + b_std^2 is the finite-width NNGP)."""
        h = np.asarray(x, dtype=np.float64)
        for i, (l, (w, b)) in enumerate(zip(dense, params)):
            if i == len(dense) - 1 and not readout:
                break
            h = l.w_std / math.sqrt(h.shape[-1]) * (h @ w) + l.b_std * b
            if i < len(dense) - 1:
                h = _phi(acts[i], h)
        return h

    return init_fn, apply_fn, kernel_fn
