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
import math

import numpy as np

from . import _lib
from .kernel_spec import HasSpec, KernelSpec

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


class KernelFn(HasSpec):
    """kernel_fn(x1, x2=None, get=None): closed-form kernel of Dense,(act,Dense)* on the GPU.  What the kernel is lives in
    ``.spec`` (kernel_spec.KernelSpec); its fields read as attributes of the kernel_fn."""

    def __init__(self, w_std, b_std, activations=None, input_scale=None, groups=None, group_weights=None, full_weight=1.0):
        """input_scale: None or d values >= 0 that multiply the features of x1 and x2 on the device before the build --
        sqrt of the relevances of include/nngp_ard.h (with_input_scale returns a copy that carries them).
        groups: None, "pairs" or (begin, end) feature ranges -- the additive kernel of include/nngp_additive.h,
        full_weight K(x, x') + sum_g group_weights[g] K(x_g, x'_g) (with_groups returns a copy that carries them)."""
        self.spec = KernelSpec(w_std, b_std, activations, input_scale, groups, group_weights, full_weight)

    def _with(self, **changes):
        return KernelFn(**self.spec.replace(**changes).as_keywords())

    def with_input_scale(self, scale):
        """A copy of this kernel_fn with ``input_scale = scale`` (None: without one)."""
        return self._with(input_scale=scale)

    def with_groups(self, groups, weights=None, full_weight=1.0):
        """A copy of this kernel_fn with the additive kernel over ``groups`` (None: the plain kernel again)."""
        return self._with(groups=groups, group_weights=weights, full_weight=full_weight)

    def group_table(self, d):
        """None, or (groups, weights, full_weight) checked against d features."""
        spec = self.spec.resolve(d)
        return None if spec.groups is None else (spec.groups, spec.group_weights, spec.full_weight)

    def _arch(self):
        return self.spec.arch() if self.all_relu else self.spec.arch_act()

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
        x1d, x2d = self.spec.scale(x1d), self.spec.scale(x2d)
        r0, r1 = (0, n1) if rows is None else (int(rows[0]), int(rows[1]))
        outs = {g: torch.empty((n1, n2), dtype=torch.float64, device=dev) for g in set(gets)}
        if n1 > 0 and n2 > 0 and r1 > r0:
            _lib.check(self.spec.kernel_build(lib, _lib.ptr(x1d), n1, _lib.ptr(x2d), n2, d, _lib.DTYPE_F64, _lib.ptr(outs.get("nngp")),
                                              _lib.ptr(outs.get("ntk")), n2, r0, r1, _lib.stream_ptr()))
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
