"""Helpers for the -m gpu parity tests: thin torch <-> C-ABI glue (everything goes through libnngp_hip.so)."""
import ctypes

import numpy as np
import torch

from nngp_src_amd import _lib


def dev():
    return torch.device("cuda", 0)


def kernel_build(x1, x2, w_std, b_std, get=("nngp", "ntk"), rows=None, dtype=torch.float64, ld=None, knobs=False):
    lib = _lib.load(knobs=knobs)
    x1d = _lib.to_device_f64(x1, dev())
    x2d = None if x2 is None else _lib.to_device_f64(x2, dev())
    n1, d = x1d.shape
    n2 = n1 if x2d is None else x2d.shape[0]
    ld = n2 if ld is None else ld
    outs = {g: torch.full((n1, ld), float("nan"), dtype=dtype, device=dev()) for g in get}
    arch = _lib.make_arch(w_std, b_std)
    r0, r1 = (0, n1) if rows is None else rows
    _lib.check(lib.nngp_kernel_build(_lib.ptr(x1d), n1, _lib.ptr(x2d), n2, d, ctypes.byref(arch),
                                     _lib.DTYPE_F64 if dtype == torch.float64 else _lib.DTYPE_F32,
                                     _lib.ptr(outs.get("nngp")), _lib.ptr(outs.get("ntk")), ld, r0, r1, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return {g: t.cpu().numpy() for g, t in outs.items()}


def build_act(x1, x2, w_std, b_std, acts, get=("nngp", "ntk"), rows=None, dtype=torch.float64, ld=None):
    """kernel_build for a network with other activations (nngp_kernel_build_act)."""
    lib = _lib.load()
    x1d = _lib.to_device_f64(x1, dev())
    x2d = None if x2 is None else _lib.to_device_f64(x2, dev())
    n1, d = x1d.shape
    n2 = n1 if x2d is None else x2d.shape[0]
    ld = n2 if ld is None else ld
    outs = {g: torch.full((n1, ld), float("nan"), dtype=dtype, device=dev()) for g in get}
    arch = _lib.make_arch_act(w_std, b_std, acts)
    r0, r1 = (0, n1) if rows is None else rows
    _lib.check(lib.nngp_kernel_build_act(_lib.ptr(x1d), n1, _lib.ptr(x2d), n2, d, ctypes.byref(arch),
                                         _lib.DTYPE_F64 if dtype == torch.float64 else _lib.DTYPE_F32,
                                         _lib.ptr(outs.get("nngp")), _lib.ptr(outs.get("ntk")), ld, r0, r1, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return {g: t.cpu().numpy() for g, t in outs.items()}


def diag_act(x, w_std, b_std, acts):
    """(K(x, x), Theta(x, x)) per row through nngp_kernel_diag_act."""
    lib = _lib.load()
    xd = _lib.to_device_f64(x, dev())
    dn = torch.empty(xd.shape[0], dtype=torch.float64, device=dev())
    dt = torch.empty_like(dn)
    arch = _lib.make_arch_act(w_std, b_std, acts)
    _lib.check(lib.nngp_kernel_diag_act(_lib.ptr(xd), xd.shape[0], xd.shape[1], ctypes.byref(arch), _lib.ptr(dn), _lib.ptr(dt),
                                        _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dn.cpu().numpy(), dt.cpu().numpy()


def kernel_diag(x, w_std, b_std):
    """(K(x, x), Theta(x, x)) per row through nngp_kernel_diag (all-ReLU network)."""
    lib = _lib.load()
    xd = _lib.to_device_f64(x, dev())
    dn = torch.empty(xd.shape[0], dtype=torch.float64, device=dev())
    dt = torch.empty_like(dn)
    arch = _lib.make_arch(w_std, b_std)
    _lib.check(lib.nngp_kernel_diag(_lib.ptr(xd), xd.shape[0], xd.shape[1], ctypes.byref(arch), _lib.ptr(dn), _lib.ptr(dt),
                                    _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dn.cpu().numpy(), dt.cpu().numpy()


def gemm_nt(c, a, b, alpha, beta, lower_only=False):
    lib = _lib.load()
    m, k = a.shape
    n = b.shape[0]
    _lib.check(lib.nngp_gemm_nt_f32(_lib.ptr(c), c.stride(0), _lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0),
                                    m, n, k, alpha, beta, int(lower_only), _lib.stream_ptr()))
    torch.cuda.synchronize()


def gemm_nt_h3(c, a, b, alpha, beta, scale, lower_only=False):
    lib = _lib.load()
    m, k = a.shape
    n = b.shape[0]
    _lib.check(lib.nngp_gemm_nt_h3(_lib.ptr(c), c.stride(0), _lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0),
                                   m, n, k, alpha, beta, scale, int(lower_only), _lib.stream_ptr()))
    torch.cuda.synchronize()


def gemm_nt_f64(c, cin, a, b, alpha, beta):
    lib = _lib.load()
    m, k = a.shape
    n = b.shape[0]
    _lib.check(lib.nngp_gemm_nt_f64(_lib.ptr(c), c.stride(0), _lib.ptr(cin), 0 if cin is None else cin.stride(0), _lib.ptr(a),
                                    a.stride(0), _lib.ptr(b), b.stride(0), m, n, k, alpha, beta, _lib.stream_ptr()))
    torch.cuda.synchronize()


def gemm_nt_i8s(c, cin, a, b, alpha, beta, slices_a=5, slices_b=5, cut=4):
    lib = _lib.load()
    m, k = a.shape
    n = b.shape[0]
    _lib.check(lib.nngp_gemm_nt_i8s(_lib.ptr(c), c.stride(0), _lib.ptr(cin), 0 if cin is None else cin.stride(0), _lib.ptr(a),
                                    a.stride(0), _lib.ptr(b), b.stride(0), m, n, k, alpha, beta, slices_a, slices_b, cut,
                                    _lib.stream_ptr()))
    torch.cuda.synchronize()


def potrf(a):
    """a: [n, n] float32 cuda tensor (lower triangle used); returns (dinv [n/128,128,128], clamped)."""
    lib = _lib.load()
    n = a.shape[0]
    dinv = torch.full((n // 128, 128, 128), float("nan"), dtype=torch.float32, device=a.device)
    clamped = torch.zeros(1, dtype=torch.int32, device=a.device)
    _lib.check(lib.nngp_potrf_f32(_lib.ptr(a), n, a.stride(0), _lib.ptr(dinv), _lib.ptr(clamped), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dinv, int(clamped.item())


def trsm(b, l, dinv):
    lib = _lib.load()
    _lib.check(lib.nngp_trsm_rlt_f32(_lib.ptr(b), b.stride(0), b.shape[0], _lib.ptr(l), l.stride(0), _lib.ptr(dinv),
                                     l.shape[0], _lib.stream_ptr()))
    torch.cuda.synchronize()


def _padded_f64(a, ld, fill=float("nan")):
    """numpy [r, c] -> cuda [r, ld] float64 with the padding columns filled (they are never read)."""
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[0], ld), fill, dtype=torch.float64, device=dev())
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t


def potrf_dinv_f64(a, ld=None):
    """nngp_potrf_dinv_f64 on a copy of a [n, n] with leading dimension ld: (rc, what came back in a's place [n, n] -- L in the
    lower triangle, workspace above the diagonal blocks --, dinv [n / 128, 128, 128]).  rc < 0: lib.nngp_last_error() says why."""
    lib = _lib.load()
    n = a.shape[0]
    ad = _padded_f64(a, n if ld is None else ld)
    dinv = torch.full((n // 128, 128, 128), float("nan"), dtype=torch.float64, device=dev())
    rc = lib.nngp_potrf_dinv_f64(_lib.ptr(ad), n, ad.stride(0), _lib.ptr(dinv), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, ad[:, :n].cpu().numpy(), dinv.cpu().numpy()


def trsm_fwd_f64(bt, l, dinv, tri=False, ldb=None, ldl=None):
    """nngp_trsm_fwd_f64 on a copy of bt [rows, n]: bt L^-T."""
    lib = _lib.load()
    rows, n = bt.shape
    bd = _padded_f64(bt, n if ldb is None else ldb)
    ld_ = _padded_f64(l, n if ldl is None else ldl)
    dd = _lib.to_device_f64(dinv, dev())
    _lib.check(lib.nngp_trsm_fwd_f64(_lib.ptr(bd), bd.stride(0), rows, _lib.ptr(ld_), ld_.stride(0), _lib.ptr(dd), n, int(tri),
                                     _lib.stream_ptr()), lib)
    torch.cuda.synchronize()
    return bd[:, :n].cpu().numpy()


def factor_solve_f64(a, y, mode, want=("l", "w", "zt", "ainv", "alpha", "nrs"), lda=None):
    """nngp_factor_solve_f64: the outputs named in want that the mode produces, as numpy arrays of the padded size."""
    lib = _lib.load()
    n = a.shape[0]
    np_ = -(-n // 128) * 128
    made = {0: ("l", "w"), 1: ("l", "w", "zt", "ainv", "alpha", "nrs"), 2: ("l", "w", "zt", "alpha", "nrs")}[mode]
    ad = _padded_f64(a, n if lda is None else lda)
    yd = _lib.to_device_f64(y, dev())
    out = {k: torch.full((np_, np_) if k in ("l", "zt", "ainv") else (np_,), float("nan"), dtype=torch.float64, device=dev())
           for k in want if k in made}
    _lib.check(lib.nngp_factor_solve_f64(_lib.ptr(ad), ad.stride(0), _lib.ptr(yd), n, mode, *[_lib.ptr(out.get(k)) for k in
                                         ("l", "w", "zt", "ainv", "alpha", "nrs")], _lib.stream_ptr()), lib)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


I8S_SENTINEL = 0x5A  # what the plane buffers of i8s_cut_rows / i8s_cut_sym hold before the call


def i8s_cut_rows(src, ns, ld=None, ldp=None, scale_in=None, writeback=None):
    """nngp_i8s_cut_rows on src [rows, cols] with leading dimension ld (NaN in the padding): (rc, scales [rows] -- scale_in
    when given --, planes [ns, rows, ldp] int8 with the sentinel wherever the call wrote nothing, the ldp bytes behind the last
    plane (one row too many would land there), the source buffer [rows, ld] after the call, the write-back buffer [rows, ld] or
    None).  writeback: None, "inplace" or "other" (a second buffer filled with NaN)."""
    lib = _lib.load()
    rows, cols = src.shape
    ld = cols + (cols & 1) if ld is None else ld
    ldp = -(-cols // 128) * 128 if ldp is None else ldp
    sd = _padded_f64(src, ld)
    flat = torch.full((ns * rows * ldp + ldp,), I8S_SENTINEL, dtype=torch.int8, device=dev())
    sc_in = None if scale_in is None else _lib.to_device_f64(scale_in, dev())
    sc_out = torch.full((rows,), float("nan"), dtype=torch.float64, device=dev())
    wb = {None: None, "inplace": sd, "other": torch.full((rows, ld), float("nan"), dtype=torch.float64, device=dev())}[writeback]
    rc = lib.nngp_i8s_cut_rows(_lib.ptr(sd), ld, rows, cols, ns, _lib.ptr(sc_in), _lib.ptr(sc_out), _lib.ptr(flat), ldp, _lib.ptr(wb),
                               _lib.stream_ptr())
    torch.cuda.synchronize()
    flat = flat.cpu().numpy()
    return (rc, (sc_out if scale_in is None else sc_in).cpu().numpy(), flat[:ns * rows * ldp].reshape(ns, rows, ldp), flat[ns * rows * ldp:],
            sd.cpu().numpy(), None if wb is None else wb.cpu().numpy())


def i8s_cut_sym(kmat, ns, by_rows, ld=None, ldp=None):
    """nngp_i8s_cut_sym on kmat [n, n]: (rc, scales [n], planes [ns, n, ldp] int8 over the sentinel, sum of the squared scales)."""
    lib = _lib.load()
    n = kmat.shape[0]
    ld = n if ld is None else ld
    ldp = n if ldp is None else ldp
    kd = _padded_f64(kmat, ld)
    planes = torch.full((ns, n, ldp), I8S_SENTINEL, dtype=torch.int8, device=dev())
    sc = torch.full((n,), float("nan"), dtype=torch.float64, device=dev())
    sq = torch.full((1,), float("nan"), dtype=torch.float64, device=dev())
    rc = lib.nngp_i8s_cut_sym(_lib.ptr(kd), ld, n, ns, _lib.ptr(sc), _lib.ptr(planes), ldp, int(by_rows), _lib.ptr(sq), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, sc.cpu().numpy(), planes.cpu().numpy(), float(sq.item())


def i8s_residual(z, kmat, cin, alpha, beta, gamma, ns_z, ns_k, cut, round_z=False, sym=False, base=None, inplace=False, ld_pad=0):
    """nngp_i8s_residual: dict(rc, out [mp, n], z [mp, n] after the call, and with base [mp] given the fused outputs out32, var,
    delta, zstat [mp, 2], floor_rows, floor_z).  inplace: cin's buffer is out.  ld_pad: extra (NaN) columns of every operand."""
    lib = _lib.load()
    mp, n = z.shape
    ld = n + ld_pad
    zd, kd = _padded_f64(z, ld), _padded_f64(kmat, ld)
    cd = None if cin is None else _padded_f64(cin, ld)
    od = cd if inplace else torch.full((mp, ld), float("nan"), dtype=torch.float64, device=dev())
    f = {}
    if base is not None:
        f = {"out32": torch.full((mp, n), float("nan"), dtype=torch.float32, device=dev()), "base": _lib.to_device_f64(base, dev()),
             "var": torch.full((mp,), float("nan"), dtype=torch.float64, device=dev()),
             "delta": torch.full((mp,), float("nan"), dtype=torch.float64, device=dev()),
             "zstat": torch.full((mp, 2), float("nan"), dtype=torch.float64, device=dev()),
             "floor_rows": torch.full((1,), float("nan"), dtype=torch.float64, device=dev()),
             "floor_z": torch.full((1,), float("nan"), dtype=torch.float64, device=dev())}
    rc = lib.nngp_i8s_residual(_lib.ptr(od), ld, _lib.ptr(cd), ld, _lib.ptr(zd), ld, _lib.ptr(kd), ld, mp, n, alpha, beta, gamma, ns_z, ns_k,
                               cut, int(round_z), int(sym), *[_lib.ptr(f.get(k)) for k in
                                                              ("out32", "base", "var", "delta", "zstat", "floor_rows", "floor_z")],
                               _lib.stream_ptr())
    torch.cuda.synchronize()
    res = {"rc": rc, "out": od[:, :n].cpu().numpy(), "z": zd[:, :n].cpu().numpy()}
    res.update({k: t.cpu().numpy() for k, t in f.items() if k != "base"})
    return res


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def mean_gate(mean, ref):
    """SURVEY.md 8d parity gate: |d mu|_2/|mu|_2 <= 1e-4 and |d mu_i| <= 1e-4 max(1, |mu_i|)."""
    mean, ref = np.asarray(mean).ravel(), np.asarray(ref).ravel()
    return rel_l2(mean, ref), float(np.max(np.abs(mean - ref) / np.maximum(1.0, np.abs(ref))))
