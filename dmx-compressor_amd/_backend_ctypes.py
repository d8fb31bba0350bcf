"""The ctypes BINDING of the C ABI (include/dmxq.h): the Python twin of csrc/torch_binding.cpp.

One function per dispatcher op of `torch.ops.dmxq.*`, with the SAME raw schema (integer codes for rounding modes and function
kinds, `int[4]` lists for FloatingPoint formats, optional tensors, `out_dtype`) and the same behaviour: make the tensors contiguous,
factor the shape as [outer, L, inner], allocate the outputs, make the tensor's device current, pass torch's current HIP stream,
call ONE extern "C" entry point, raise `NotImplementedError` where the library answers DMXQ_ERR_UNSUPPORTED (what
TORCH_CHECK_NOT_IMPLEMENTED raises in the C++ binding).  No argument spelling, no policy: that lives ONCE in `_front.py`, which
runs on either binding (`DMXQ_BINDING=torch|ctypes`, ops.py).  No autograd registration and no meta kernels here (the ctypes
binding is not traceable by torch.compile); needs no C++ compiler against the torch headers.
"""
import ctypes
import functools

import torch

from . import _lib
from ._lib import check, dtype_code, lib, ptr, require_gpu, split3, stream_of

_U64 = 0xFFFFFFFFFFFFFFFF


def _prep(x: torch.Tensor, what: str) -> torch.Tensor:
    require_gpu(x, what)
    dtype_code(x.dtype)
    return x if x.is_contiguous() else x.contiguous()


def _split(x, dim):
    return split3(x.shape, dim) if x.dim() else (1, 1, 1)


def _unsupported(what):
    raise NotImplementedError(what)


def _fmt_ptrs(*fmts):
    """int[4] lists (man_bits, exp_bits, exp_bias, flush_subnormal; empty = SAME) -> dmxq_float_fmt pointers (+ keep-alive)"""
    structs = [None if not f else _lib.FloatFmt(int(f[0]), int(f[1]), int(f[2]), int(f[3])) for f in fmts]
    return [ctypes.cast(ctypes.pointer(s), ctypes.c_void_p) if s is not None else None for s in structs], structs


def _guarded(fn):
    """HIP launches go to the CURRENT device: a tensor on another GPU of this process needs its device made current around the
    C-ABI call (the C++ binding's device guard).  One integer compare when it already is."""

    @functools.wraps(fn)
    def g(x, *a, **k):
        t = x[0] if isinstance(x, (list, tuple)) and x else x
        if isinstance(t, torch.Tensor) and t.is_cuda and t.device.index != torch.cuda.current_device():
            with torch.cuda.device(t.device):
                return fn(x, *a, **k)
        return fn(x, *a, **k)

    return g


# ------------------------------------------------------------------------------------------------ block formats
@_guarded
def bfp_qdq(x, precision, block_size, block_dim=-1, symmetric=True, rounding=2, out_dtype=None, seed=0):
    xc = _prep(x, "bfp_qdq")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    outer, L, inner = _split(xc, block_dim)
    check(lib().dmxq_bfp_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), outer, L, inner, block_size, precision,
                             rounding, int(symmetric), seed & _U64, stream_of(xc)), "dmxq_bfp_qdq")
    return out


bfp_qdq_nograd = bfp_qdq


@_guarded
def block_quantize(a, wl, symmetric, rounding, seed=0):
    xc = _prep(a, "block_quantize")
    if xc.dim() != 2:
        raise RuntimeError("block_quantize: expects a [rows, L] view")
    out = torch.empty_like(xc)
    check(lib().dmxq_bfp_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), xc.shape[0], xc.shape[1], 1,
                             max(xc.shape[1], 2), wl, rounding, 1 if symmetric else 2, seed & _U64, stream_of(xc)), "dmxq_bfp_qdq")
    return out


@_guarded
def bfp_qdq_multi(xs, precision, block_size, block_dim=-1, symmetric=True, rounding=2, out_dtype=None, seed=0):
    if not xs:
        return []
    ins = [_prep(t, "bfp_qdq_multi") for t in xs]
    dt, dev = ins[0].dtype, ins[0].device
    if any(x.dtype != dt or x.device != dev for x in ins):
        raise RuntimeError("bfp_qdq_multi: all tensors must share one dtype and one device")
    outs = [torch.empty(x.shape, dtype=out_dtype or dt, device=dev) for x in ins]
    descs = (_lib.TensorDesc * len(ins))()
    for d, x, o in zip(descs, ins, outs):
        d.in_, d.out = x.data_ptr(), o.data_ptr()
        d.outer, d.L, d.inner = _split(x, block_dim)
    check(lib().dmxq_bfp_qdq_multi(descs, len(ins), dtype_code(dt), dtype_code(outs[0].dtype), block_size, precision, rounding,
                                   int(symmetric), seed & _U64, stream_of(ins[0])), "dmxq_bfp_qdq_multi")
    return outs


@_guarded
def bfp_pack(x, precision, block_size, symmetric=True):
    xc = _prep(x, "bfp_pack")
    L = xc.shape[-1] if xc.dim() else 1
    rows = xc.numel() // max(L, 1)
    mant = torch.empty(xc.shape, dtype=torch.int8, device=xc.device)
    exps = torch.empty((tuple(xc.shape[:-1]) if xc.dim() else ()) + (-(-L // block_size),), dtype=torch.uint8, device=xc.device)
    check(lib().dmxq_bfp_pack(ptr(xc), dtype_code(xc.dtype), ptr(mant), ptr(exps), rows, L, block_size, precision, int(symmetric),
                              stream_of(xc)), "dmxq_bfp_pack")
    return mant, exps


@_guarded
def bfp_unpack(mant, exps, precision, block_size, out_dtype):
    require_gpu(mant, "bfp_unpack")
    m, e = mant.contiguous(), exps.contiguous()
    L = m.shape[-1] if m.dim() else 1
    out = torch.empty(m.shape, dtype=out_dtype, device=m.device)
    check(lib().dmxq_bfp_unpack(ptr(m), ptr(e), ptr(out), dtype_code(out_dtype), m.numel() // max(L, 1), L, block_size, precision,
                                stream_of(m)), "dmxq_bfp_unpack")
    return out


@_guarded
def weight_hypernet(w, precision, block_size, symmetric, score, K, M, sq_scale, out_dtype=None, block_dim=-1):
    wc = _prep(w, "weight_hypernet")
    masked = score is not None and M != 0
    sc = _prep(score, "weight_hypernet") if masked else None
    if masked and sc.shape != wc.shape:
        _unsupported("weight_hypernet: score and weight shapes differ")
    outer, L, inner = _split(wc, block_dim if wc.dim() else -1)
    rows = wc.numel() // max(L, 1) if L else 0
    sq = sq_scale.detach().to(device=wc.device, dtype=torch.float32).contiguous() if sq_scale is not None else None
    if sq is not None and sq.numel() != L:
        _unsupported("weight_hypernet: scale length differs from the channel count")
    od = out_dtype or (torch.promote_types(wc.dtype, sc.dtype) if masked else wc.dtype)
    out = torch.empty(wc.shape, dtype=od, device=wc.device)
    if inner != 1:
        check(lib().dmxq_weight_hypernet_strided(ptr(wc), dtype_code(wc.dtype), ptr(sc), dtype_code(sc.dtype) if masked else 0, K,
                                                 M if masked else 0, ptr(sq), ptr(out), dtype_code(od), outer, L, inner, block_size,
                                                 precision, int(symmetric), stream_of(wc)), "dmxq_weight_hypernet_strided")
        return out
    check(lib().dmxq_weight_hypernet(ptr(wc), dtype_code(wc.dtype), ptr(sc), dtype_code(sc.dtype) if masked else 0, K, M if masked else 0,
                                     ptr(sq), ptr(out), dtype_code(od), rows, L, block_size, precision, int(symmetric), stream_of(wc)),
          "dmxq_weight_hypernet")
    return out


@_guarded
def weight_hypernet_multi(ws, precision, block_size, symmetric, scores, K, M, sq_scales, out_dtype=None):
    if not ws:
        return []
    masked = bool(scores) and M != 0
    if (masked and len(scores) != len(ws)) or (sq_scales and len(sq_scales) != len(ws)):
        raise RuntimeError("weight_hypernet_multi: one score / scale per weight, or none")
    wcs = [_prep(w, "weight_hypernet_multi") for w in ws]
    dt, dev = wcs[0].dtype, wcs[0].device
    if any(w.dtype != dt or w.device != dev for w in wcs):
        raise RuntimeError("weight_hypernet_multi: all weights must share one dtype and one device")
    scs = [_prep(s, "weight_hypernet_multi") for s in scores] if masked else []
    if masked and any(s.dtype != scs[0].dtype for s in scs):
        raise RuntimeError("weight_hypernet_multi: all scores must share one dtype")
    if masked and any(s.shape != w.shape for s, w in zip(scs, wcs)):
        _unsupported("weight_hypernet_multi: score and weight shapes differ")
    sqs = [q.detach().to(device=dev, dtype=torch.float32).contiguous() for q in sq_scales] if sq_scales else []
    od = out_dtype or (torch.promote_types(dt, scs[0].dtype) if masked else dt)
    outs = [torch.empty(w.shape, dtype=od, device=dev) for w in wcs]
    descs = (_lib.HypernetDesc * len(wcs))()
    for i, (d, w, o) in enumerate(zip(descs, wcs, outs)):
        L = w.shape[-1] if w.dim() else 1
        if sqs and sqs[i].numel() != L:
            _unsupported("weight_hypernet_multi: scale length differs from the channel count")
        d.w, d.score, d.sq_scale, d.out = w.data_ptr(), (scs[i].data_ptr() if masked else None), (sqs[i].data_ptr() if sqs else None), o.data_ptr()
        d.rows, d.L = (w.numel() // L if L else 0), L
    check(lib().dmxq_weight_hypernet_multi(descs, len(wcs), dtype_code(dt), dtype_code(scs[0].dtype) if masked else 0, K, M if masked else 0,
                                           dtype_code(od), block_size, precision, int(symmetric), stream_of(wcs[0])), "dmxq_weight_hypernet_multi")
    return outs


@_guarded
def input_hypernet(x, sq_scale, precision, block_size, symmetric):
    xc = _prep(x, "input_hypernet")
    L = xc.shape[-1] if xc.dim() else 1
    sq = sq_scale.detach().to(device=xc.device, dtype=torch.float32).contiguous()
    if sq.numel() != L:
        _unsupported("input_hypernet: scale length differs from the channel count")
    out = torch.empty(xc.shape, dtype=torch.float32, device=xc.device)
    check(lib().dmxq_input_hypernet(ptr(xc), dtype_code(xc.dtype), ptr(sq), ptr(out), _lib.F32, xc.numel() // max(L, 1), L, block_size,
                                    precision, int(symmetric), stream_of(xc)), "dmxq_input_hypernet")
    return out


@_guarded
def binary_cast(a, b, op, cast_a, cast_b, cast_out, bfp_block=0, bfp_precision=0):
    ac, bc = _prep(a, "binary_cast"), _prep(b, "binary_cast")
    if ac.shape != bc.shape or ac.dtype != bc.dtype or ac.device != bc.device:
        _unsupported("binary_cast: operands of one shape, dtype and device")
    out = torch.empty_like(ac)
    ptrs, _keep = _fmt_ptrs(cast_a, cast_b, cast_out)
    if bfp_block > 0:
        if ac.dim() < 1 or ac.numel() == 0:
            _unsupported("binary_cast: the BFP epilogue needs a last dim")
        check(lib().dmxq_binary_cast_bfp(ptr(ac), ptr(bc), ptr(out), dtype_code(ac.dtype), ac.numel(), op, *ptrs, ac.shape[-1], bfp_block,
                                         bfp_precision, stream_of(ac)), "dmxq_binary_cast_bfp")
    else:
        check(lib().dmxq_binary_cast(ptr(ac), ptr(bc), ptr(out), dtype_code(ac.dtype), ac.numel(), op, *ptrs, stream_of(ac)), "dmxq_binary_cast")
    return out


@_guarded
def relu_cast(x, cast_in, cast_out, bfp_block=0, bfp_precision=0):
    xc = _prep(x, "relu_cast")
    out = torch.empty_like(xc)
    ptrs, _keep = _fmt_ptrs(cast_in, cast_out)
    if bfp_block > 0:
        if xc.dim() < 1 or xc.numel() == 0:
            _unsupported("relu_cast: the BFP epilogue needs a last dim")
        check(lib().dmxq_relu_cast_bfp(ptr(xc), ptr(out), dtype_code(xc.dtype), xc.numel(), *ptrs, xc.shape[-1], bfp_block, bfp_precision,
                                       stream_of(xc)), "dmxq_relu_cast_bfp")
    else:
        check(lib().dmxq_relu_cast(ptr(xc), ptr(out), dtype_code(xc.dtype), xc.numel(), *ptrs, stream_of(xc)), "dmxq_relu_cast")
    return out


@_guarded
def sbfp_qdq(x, precision, block_size, scaler_man, scaler_exp, scaler_bias, scaler_flush, clamp, symmetric, block_dim=-1, out_dtype=None):
    xc = _prep(x, "sbfp_qdq")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    outer, L, inner = _split(xc, block_dim)
    check(lib().dmxq_sbfp_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), outer, L, inner, block_size, precision,
                              int(clamp), int(symmetric), scaler_man, scaler_exp, scaler_bias, int(scaler_flush), stream_of(xc)), "dmxq_sbfp_qdq")
    return out


sbfp_qdq_nograd = sbfp_qdq


@_guarded
def mxfp_qdq(x, man, exp, block_size, block_dim=-1, out_dtype=None):
    xc = _prep(x, "mxfp_qdq")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    outer, L, inner = _split(xc, block_dim)
    check(lib().dmxq_mxfp_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), outer, L, inner, block_size, man, exp,
                              stream_of(xc)), "dmxq_mxfp_qdq")
    return out


mxfp_qdq_nograd = mxfp_qdq


# ------------------------------------------------------------------------------------------------ element formats
@_guarded
def float_qdq(x, man, exp, bias, flush_subnormal, unsigned_abs=False, rounding=2, out_dtype=None, seed=0):
    xc = _prep(x, "float_qdq")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    check(lib().dmxq_float_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), xc.numel(), man, exp, bias,
                               int(flush_subnormal), int(unsigned_abs), rounding, seed & _U64, stream_of(xc)), "dmxq_float_qdq")
    return out


float_qdq_nograd = float_qdq


@_guarded
def float_qdq_multi(xs, man, exp, bias, flush_subnormal, unsigned_abs=False, rounding=2, out_dtype=None, seed=0):
    if not xs:
        return []
    ins = [_prep(t, "float_qdq_multi") for t in xs]
    dt, dev = ins[0].dtype, ins[0].device
    if any(x.dtype != dt or x.device != dev for x in ins):
        raise RuntimeError("float_qdq_multi: all tensors must share one dtype and one device")
    outs = [torch.empty(x.shape, dtype=out_dtype or dt, device=dev) for x in ins]
    descs = (_lib.TensorDesc * len(ins))()
    for d, x, o in zip(descs, ins, outs):
        d.in_, d.out, d.outer, d.L, d.inner = x.data_ptr(), o.data_ptr(), 1, x.numel(), 1
    check(lib().dmxq_float_qdq_multi(descs, len(ins), dtype_code(dt), dtype_code(outs[0].dtype), man, exp, bias, int(flush_subnormal),
                                     int(unsigned_abs), rounding, seed & _U64, stream_of(ins[0])), "dmxq_float_qdq_multi")
    return outs


def _affine_need(C, scale_numel, group_size, has_axis):
    return (-(-C // (group_size or 1))) if has_axis else 1


@_guarded
def fixed_qdq(x, precision, fraction, clamp, symmetric, rounding, scale, zero_point, ch_axis, group_size, out_dtype=None, seed=0):
    xc = _prep(x, "fixed_qdq")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = zp = None
    outer, C, inner, gs = 1, 1, xc.numel(), 1
    if scale is not None:
        if zero_point is None:
            raise RuntimeError("fixed_qdq: scale without zero_point")
        sc = scale.detach().to(device=xc.device, dtype=torch.float32).contiguous()
        zp = zero_point.detach().to(device=xc.device, dtype=torch.int64).contiguous()
        need = 1
        if ch_axis is not None and xc.dim() > 0:
            outer, C, inner = split3(xc.shape, ch_axis)
            gs = group_size or 1
            need = -(-C // gs)
        if sc.numel() < need or zp.numel() < need:
            raise ValueError(f"fixed_qdq: need {need} scale/zero_point entries, got {sc.numel()}/{zp.numel()}")
    check(lib().dmxq_fixed_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), outer, C, inner, precision, fraction,
                               int(clamp), int(symmetric), rounding, ptr(sc), ptr(zp), gs, seed & _U64, stream_of(xc)), "dmxq_fixed_qdq")
    return out


fixed_qdq_nograd = fixed_qdq


@_guarded
def fixed_qdq_multi(xs, precision, fraction, clamp, symmetric, rounding, scales, zero_points, group_size, out_dtype=None, seed=0):
    if not xs:
        return []
    ins = [_prep(t, "fixed_qdq_multi") for t in xs]
    dt, dev = ins[0].dtype, ins[0].device
    if any(x.dtype != dt or x.device != dev for x in ins):
        raise RuntimeError("fixed_qdq_multi: all tensors must share one dtype and one device")
    if len(scales) != len(ins) or len(zero_points) != len(ins):
        raise RuntimeError("fixed_qdq_multi: one scale and one zero_point tensor per weight")
    outs = [torch.empty(x.shape, dtype=out_dtype or dt, device=dev) for x in ins]
    scs = [s.detach().to(device=dev, dtype=torch.float32).contiguous() for s in scales]
    zps = [z.detach().to(device=dev, dtype=torch.int64).contiguous() for z in zero_points]
    gs = group_size or 1
    descs = (_lib.AffineDesc * len(ins))()
    for i, (d, x, o, s, z) in enumerate(zip(descs, ins, outs, scs, zps)):
        # a one-entry scale means per-tensor ONLY when no group_size was asked for; with group_size set a weight needs
        # ceil(C / group_size) entries like fixed_qdq(ch_axis=0, group_size=...) (an uncalibrated cast, scale = [1.0], must raise here
        # too, not be folded with a per-tensor scale of 1)
        outer, C, inner = split3(x.shape, 0) if x.dim() > 0 else (1, 1, 1)
        need = -(-C // gs) if (group_size or s.numel() != 1) else 1
        if s.numel() < need or z.numel() < need:
            raise ValueError(f"fixed_qdq_multi: tensor {i} needs {need} scale/zero_point entries, got {s.numel()}/{z.numel()}")
        if need == 1:
            outer, C, inner = 1, 1, x.numel()
        d.in_, d.out, d.scale, d.zero_point, d.outer, d.C, d.inner = x.data_ptr(), o.data_ptr(), s.data_ptr(), z.data_ptr(), outer, C, inner
    check(lib().dmxq_fixed_qdq_multi(descs, len(ins), dtype_code(dt), dtype_code(outs[0].dtype), precision, fraction, int(clamp),
                                     int(symmetric), rounding, gs, seed & _U64, stream_of(ins[0])), "dmxq_fixed_qdq_multi")
    return outs


@_guarded
def fixed_float_qdq_multi(xs, precision, fraction, clamp, symmetric, rounding, scales, zero_points, group_size,
                          fs, man, exp, bias, flush_subnormal, unsigned_abs, rounding_float, seed=0):
    """(fixed results, float results): `fixed_qdq_multi(xs, ...)` and `float_qdq_multi(fs, ...)` in one launch where the set allows it"""
    if not xs or not fs:
        return (fixed_qdq_multi(xs, precision, fraction, clamp, symmetric, rounding, scales, zero_points, group_size, None, seed),
                float_qdq_multi(fs, man, exp, bias, flush_subnormal, unsigned_abs, rounding_float, None, seed))
    ins = [_prep(t, "fixed_float_qdq_multi") for t in xs]
    fins = [_prep(t, "fixed_float_qdq_multi") for t in fs]
    dt, dev = ins[0].dtype, ins[0].device
    if any(x.dtype != dt or x.device != dev for x in ins + fins):
        raise RuntimeError("fixed_float_qdq_multi: all tensors must share one dtype and one device")
    if len(scales) != len(ins) or len(zero_points) != len(ins):
        raise RuntimeError("fixed_float_qdq_multi: one scale and one zero_point tensor per weight")
    outs = [torch.empty_like(x) for x in ins]
    fouts = [torch.empty_like(x) for x in fins]
    scs = [s.detach().to(device=dev, dtype=torch.float32).contiguous() for s in scales]
    zps = [z.detach().to(device=dev, dtype=torch.int64).contiguous() for z in zero_points]
    gs = group_size or 1
    descs = (_lib.AffineDesc * len(ins))()
    for i, (d, x, o, s, z) in enumerate(zip(descs, ins, outs, scs, zps)):
        outer, C, inner = split3(x.shape, 0) if x.dim() > 0 else (1, 1, 1)
        need = -(-C // gs) if (group_size or s.numel() != 1) else 1
        if s.numel() < need or z.numel() < need:
            raise ValueError(f"fixed_float_qdq_multi: tensor {i} needs {need} scale/zero_point entries, got {s.numel()}/{z.numel()}")
        if need == 1:
            outer, C, inner = 1, 1, x.numel()
        d.in_, d.out, d.scale, d.zero_point, d.outer, d.C, d.inner = x.data_ptr(), o.data_ptr(), s.data_ptr(), z.data_ptr(), outer, C, inner
    fdescs = (_lib.TensorDesc * len(fins))()
    for d, x, o in zip(fdescs, fins, fouts):
        d.in_, d.out, d.outer, d.L, d.inner = x.data_ptr(), o.data_ptr(), 1, x.numel(), 1
    check(lib().dmxq_fixed_float_qdq_multi(descs, len(ins), precision, fraction, int(clamp), int(symmetric), rounding, gs, fdescs, len(fins), man, exp,
                                           bias, int(flush_subnormal), int(unsigned_abs), rounding_float, dtype_code(dt), seed & _U64,
                                           stream_of(ins[0])), "dmxq_fixed_float_qdq_multi")
    return outs, fouts


# ------------------------------------------------------------------------------------------------ sparsity
def _maybe(t, want, shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device) if want else None


@_guarded
def nm_mask(score, x, K, M, block_dim, want_mask, want_y, mask_dtype=None, y_dtype=None):
    sc = _prep(score, "nm_mask")
    outer, L, inner = _split(sc, block_dim)
    xc = None
    if want_y:
        xc = _prep(x, "nm_sparsify")
        if xc.shape != sc.shape:
            xc = xc.expand(sc.shape).contiguous()
        y_dtype = y_dtype or torch.promote_types(xc.dtype, sc.dtype)
    mask = _maybe(None, want_mask, sc.shape, mask_dtype or sc.dtype, sc.device)
    y = _maybe(None, want_y, sc.shape, y_dtype, sc.device)
    check(lib().dmxq_nm_mask(ptr(sc), dtype_code(sc.dtype), ptr(xc), dtype_code(xc.dtype) if want_y else 0, ptr(mask),
                             dtype_code(mask.dtype) if want_mask else 0, ptr(y), dtype_code(y.dtype) if want_y else 0, outer, L, inner, K, M,
                             stream_of(sc)), "dmxq_nm_mask")
    return mask, y


@_guarded
def topk_mask(score, x, n_zero, want_mask, want_y, mask_dtype=None, y_dtype=None):
    sc = _prep(score, "topk_mask")
    n = sc.numel()
    xc = None
    if want_y:
        xc = _prep(x, "topk_sparsify")
        if xc.shape != sc.shape:
            xc = xc.expand(sc.shape).contiguous()
        y_dtype = y_dtype or torch.promote_types(xc.dtype, sc.dtype)
    mask = _maybe(None, want_mask, sc.shape, mask_dtype or sc.dtype, sc.device)
    y = _maybe(None, want_y, sc.shape, y_dtype, sc.device)
    ws = torch.empty(max(1, (lib().dmxq_topk_workspace_bytes(n) + 7) // 8), dtype=torch.int64, device=sc.device)
    check(lib().dmxq_topk_mask(ptr(sc), dtype_code(sc.dtype), ptr(xc), dtype_code(xc.dtype) if want_y else 0, ptr(mask),
                               dtype_code(mask.dtype) if want_mask else 0, ptr(y), dtype_code(y.dtype) if want_y else 0, n, n_zero, ptr(ws),
                               stream_of(sc)), "dmxq_topk_mask")
    return mask, y


@_guarded
def bernoulli_mask(score, seed, mask_dtype=None):
    sc = _prep(score, "bernoulli_mask")
    mask = torch.empty(sc.shape, dtype=mask_dtype or sc.dtype, device=sc.device)
    check(lib().dmxq_bernoulli_mask(ptr(sc), ptr(mask), dtype_code(sc.dtype), dtype_code(mask.dtype), sc.numel(), seed & _U64,
                                    stream_of(sc)), "dmxq_bernoulli_mask")
    return mask


# ------------------------------------------------------------------------------------------------ calibration
@_guarded
def group_minmax(x, ch_axis, group_size):
    xc = _prep(x, "group_minmax")
    outer, C, inner = _split(xc, ch_axis)
    G = -(-C // group_size)
    mn = torch.empty(G, dtype=torch.float32, device=xc.device)
    mx = torch.empty(G, dtype=torch.float32, device=xc.device)
    check(lib().dmxq_group_minmax(ptr(xc), dtype_code(xc.dtype), outer, C, inner, group_size, ptr(mn), ptr(mx), stream_of(xc)),
          "dmxq_group_minmax")
    return mn, mx


@_guarded
def group_minmax_accumulate(x, ch_axis, group_size, mn, mx):
    xc = _prep(x, "group_minmax_accumulate")
    outer, C, inner = _split(xc, ch_axis)
    gs = max(int(group_size), 1)
    G = -(-C // gs)
    for t in (mn, mx):
        if not (t.is_cuda and t.device == xc.device and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == G):
            raise RuntimeError(f"group_minmax_accumulate: running min / max must be contiguous float32 tensors of {G} entries on the input's device")
    check(lib().dmxq_group_minmax_accumulate(ptr(xc), dtype_code(xc.dtype), outer, C, inner, gs, ptr(mn), ptr(mx), stream_of(xc)),
          "dmxq_group_minmax_accumulate")


@_guarded
def qparams(mn, mx, qmin, qmax, symmetric_qscheme):
    require_gpu(mn, "qparams")
    a = mn.to(torch.float32).contiguous()
    b = mx.to(device=a.device, dtype=torch.float32).contiguous()
    scale = torch.empty_like(a)
    zp = torch.empty(a.shape, dtype=torch.int64, device=a.device)
    check(lib().dmxq_qparams(ptr(a), ptr(b), a.numel(), qmin, qmax, int(symmetric_qscheme), ptr(scale), ptr(zp), stream_of(a)), "dmxq_qparams")
    return scale, zp


@_guarded
def histc(x, bins, lo, hi):
    xc = _prep(x, "histc").reshape(-1)
    out = torch.empty(int(bins), dtype=torch.float32, device=xc.device)
    check(lib().dmxq_histc(ptr(xc), dtype_code(xc.dtype), xc.numel(), int(bins), float(lo), float(hi), ptr(out), stream_of(xc)), "dmxq_histc")
    return out


@_guarded
def channel_maxabs(x, ch_axis):
    xc = _prep(x, "channel_maxabs")
    outer, C, inner = _split(xc, ch_axis)
    out = torch.empty(C, dtype=torch.float32, device=xc.device)
    check(lib().dmxq_channel_maxabs(ptr(xc), dtype_code(xc.dtype), outer, C, inner, ptr(out), stream_of(xc)), "dmxq_channel_maxabs")
    return out


@_guarded
def smoothquant_scale(a_maxabs, b_maxabs, alpha, scale_min):
    require_gpu(a_maxabs, "smoothquant_scale")
    a = a_maxabs.to(torch.float32).contiguous()
    b = b_maxabs.to(device=a.device, dtype=torch.float32).contiguous()
    if b.numel() != a.numel():
        raise RuntimeError("smoothquant_scale: the two maxima must have one entry per channel")
    out = torch.empty_like(a)
    check(lib().dmxq_smoothquant_scale(ptr(a), ptr(b), a.numel(), float(alpha), float(scale_min), ptr(out), stream_of(a)), "dmxq_smoothquant_scale")
    return out


@_guarded
def scale_channels(x, scale, ch_axis, divide, out_dtype=None):
    xc = _prep(x, "scale_channels")
    outer, C, inner = _split(xc, ch_axis)
    sc = scale.detach().to(device=xc.device, dtype=torch.float32).contiguous()
    if sc.numel() != C:
        raise ValueError(f"scale_channels: scale has {sc.numel()} entries for {C} channels")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    check(lib().dmxq_scale_channels(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), outer, C, inner, ptr(sc), int(divide),
                                    stream_of(xc)), "dmxq_scale_channels")
    return out


# ------------------------------------------------------------------------------------------------ approximator slot
@_guarded
def unary(x, kind, param=0.0, out_dtype=None):
    xc = _prep(x, "unary")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    check(lib().dmxq_unary(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), xc.numel(), kind, float(param), stream_of(xc)),
          "dmxq_unary")
    return out


def _rope_args(x, cos, sin, unsqueeze_dim, what):
    xc = _prep(x, what)
    if xc.dim() != 4 or cos.dim() != 3 or sin.dim() != 3 or unsqueeze_dim not in (1, 2) or cos.dtype != xc.dtype or sin.dtype != xc.dtype:
        _unsupported(f"{what}: x [B, n1, n2, D] and cos / sin [B, S, D] of one dtype")
    c, s = _prep(cos, what), _prep(sin, what)
    B, n1, n2, D = xc.shape
    if tuple(c.shape) != (B, n2 if unsqueeze_dim == 1 else n1, D) or s.shape != c.shape:
        _unsupported(f"{what}: cos / sin shape does not match x")
    return xc, c, s, (B, n1, n2, D)


@_guarded
def rope(x, cos, sin, unsqueeze_dim=1):
    xc, c, s, (B, n1, n2, D) = _rope_args(x, cos, sin, unsqueeze_dim, "rope")
    out = torch.empty_like(xc)
    check(lib().dmxq_rope(ptr(xc), ptr(c), ptr(s), ptr(out), dtype_code(xc.dtype), B, n1, n2, D, int(unsqueeze_dim == 1), stream_of(xc)), "dmxq_rope")
    return out


@_guarded
def rope_cast(x, cos, sin, unsqueeze_dim, cast_x, cast_cos, cast_sin, cast_out):
    xc, c, s, (B, n1, n2, D) = _rope_args(x, cos, sin, unsqueeze_dim, "rope_cast")
    ptrs, _keep = _fmt_ptrs(cast_x, cast_cos, cast_sin, cast_out)
    out = torch.empty_like(xc)
    check(lib().dmxq_rope_cast(ptr(xc), ptr(c), ptr(s), ptr(out), dtype_code(xc.dtype), B, n1, n2, D, int(unsqueeze_dim == 1), *ptrs,
                               stream_of(xc)), "dmxq_rope_cast")
    return out


@_guarded
def softmax(x, clamp_min, out_dtype=None):   # over the contiguous last dim
    xc = _prep(x, "softmax")
    cols = xc.shape[-1] if xc.dim() else 1
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    check(lib().dmxq_softmax(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), xc.numel() // max(cols, 1), cols, float(clamp_min),
                             stream_of(xc)), "dmxq_softmax")
    return out


def _wb(x, weight, bias, what, same_dtype):
    w = weight.detach().contiguous() if weight is not None else None
    b = bias.detach().contiguous() if bias is not None else None
    if same_dtype:
        for t in (w, b):
            if t is not None and (t.dtype != x.dtype or t.device != x.device):
                _unsupported(f"{what}: weight / bias must be in the row dtype, on the row's device")
    elif w is not None and b is not None and w.dtype != b.dtype:
        b = b.to(w.dtype)
    return w, b


@_guarded
def norm(x, cols, weight, bias, eps, kind, out_dtype=None):   # kind 0: layer_norm, 1: rms_norm (no bias)
    xc = _prep(x, "norm")
    rows = xc.numel() // max(cols, 1)
    w, b = _wb(xc, weight, bias, "norm", False)
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    if kind == 1:
        check(lib().dmxq_rmsnorm(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), rows, cols, ptr(w),
                                 dtype_code(w.dtype) if w is not None else 0, float(eps), stream_of(xc)), "dmxq_rmsnorm")
    else:
        wb = dtype_code((w if w is not None else b).dtype) if (w is not None or b is not None) else 0
        check(lib().dmxq_layernorm(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), rows, cols, ptr(w), ptr(b), wb, float(eps),
                                   stream_of(xc)), "dmxq_layernorm")
    return out


@_guarded
def unary_cast(x, kind, param, cast_in, cast_out):
    xc = _prep(x, "unary_cast")
    ptrs, _keep = _fmt_ptrs(cast_in, cast_out)
    out = torch.empty_like(xc)
    check(lib().dmxq_unary_cast(ptr(xc), ptr(out), dtype_code(xc.dtype), xc.numel(), kind, float(param), *ptrs, stream_of(xc)), "dmxq_unary_cast")
    return out


@_guarded
def unary_cast_table(like, kind, param, cast_in, cast_out):
    require_gpu(like, "unary_cast_table")
    if like.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError("unary_cast_table: a bfloat16 / float16 GPU tensor names the dtype and the device")
    ptrs, _keep = _fmt_ptrs(cast_in, cast_out)
    table = torch.empty(65536, dtype=torch.int16, device=like.device)
    check(lib().dmxq_unary_cast_table(dtype_code(like.dtype), kind, float(param), *ptrs, ptr(table), stream_of(like)), "dmxq_unary_cast_table")
    return table


@_guarded
def lut16_apply(x, table):
    xc = _prep(x, "lut16_apply")
    if xc.element_size() != 2 or table.numel() != 65536 or table.element_size() != 2 or table.device != xc.device or not table.is_contiguous():
        raise RuntimeError("lut16_apply: a 16-bit tensor and a 65536-entry 16-bit table on its device")
    out = torch.empty_like(xc)
    check(lib().dmxq_lut16_apply(ptr(xc), ptr(out), xc.numel(), ptr(table), stream_of(xc)), "dmxq_lut16_apply")
    return out


@_guarded
def softmax_cast(x, clamp_min, cast_in, cast_out, bfp_block=0, bfp_precision=0):
    xc = _prep(x, "softmax_cast")
    cols = xc.shape[-1] if xc.dim() else 1
    rows = xc.numel() // max(cols, 1)
    ptrs, _keep = _fmt_ptrs(cast_in, cast_out)
    out = torch.empty_like(xc)
    if bfp_block > 0:
        check(lib().dmxq_softmax_cast_bfp(ptr(xc), ptr(out), dtype_code(xc.dtype), rows, cols, float(clamp_min), *ptrs, bfp_block, bfp_precision,
                                          stream_of(xc)), "dmxq_softmax_cast_bfp")
    else:
        check(lib().dmxq_softmax_cast(ptr(xc), ptr(out), dtype_code(xc.dtype), rows, cols, float(clamp_min), *ptrs, stream_of(xc)), "dmxq_softmax_cast")
    return out


@_guarded
def norm_cast(x, cols, weight, bias, eps, kind, cast_in, cast_out, bfp_block=0, bfp_precision=0):
    xc = _prep(x, "norm_cast")
    rows = xc.numel() // max(cols, 1)
    w, b = _wb(xc, weight, bias, "norm_cast", True)
    for t in (w, b):
        if t is not None and t.numel() != cols:
            _unsupported("norm_cast: one weight / bias entry per column")
    ptrs, _keep = _fmt_ptrs(cast_in, cast_out)
    out = torch.empty_like(xc)
    L = lib()
    if kind == 1:
        if bfp_block > 0:
            check(L.dmxq_rmsnorm_cast_bfp(ptr(xc), ptr(out), dtype_code(xc.dtype), rows, cols, ptr(w), float(eps), *ptrs, bfp_block, bfp_precision,
                                          stream_of(xc)), "dmxq_rmsnorm_cast_bfp")
        else:
            check(L.dmxq_rmsnorm_cast(ptr(xc), ptr(out), dtype_code(xc.dtype), rows, cols, ptr(w), float(eps), *ptrs, stream_of(xc)), "dmxq_rmsnorm_cast")
    elif bfp_block > 0:
        check(L.dmxq_layernorm_cast_bfp(ptr(xc), ptr(out), dtype_code(xc.dtype), rows, cols, ptr(w), ptr(b), float(eps), *ptrs, bfp_block,
                                        bfp_precision, stream_of(xc)), "dmxq_layernorm_cast_bfp")
    else:
        check(L.dmxq_layernorm_cast(ptr(xc), ptr(out), dtype_code(xc.dtype), rows, cols, ptr(w), ptr(b), float(eps), *ptrs, stream_of(xc)),
              "dmxq_layernorm_cast")
    return out


# ------------------------------------------------------------------------------------------------ GPTQ
def _gptq_format(fmt, what):
    """the 12 fields of a dmxq_gptq_format in the struct's order: one format, or one format's slice of a list"""
    if len(fmt) != 12:
        raise RuntimeError(f"{what}: fmt is the 12 fields of dmxq_gptq_format")
    return _lib.GptqFormat(*[int(v) for v in fmt])


def _gptq_matrix(t, w, name):
    if not (t.is_cuda and t.device == w.device and t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)):
        raise RuntimeError(f"gptq_block: {name} must be a float32 matrix with unit column stride on w's GPU")


@_guarded
def gptq_block(w, hinv, inv_d, microblock, fmt, scale, zero_point, q, err):
    require_gpu(w, "gptq_block")
    for t, name in ((w, "w"), (hinv, "hinv"), (q, "q"), (err, "err")):
        _gptq_matrix(t, w, name)
    f = _gptq_format(fmt, "gptq_block")
    if microblock < 1:
        raise RuntimeError("gptq_block: microblock must be positive")
    rows, count = w.shape
    nmb = -(-count // microblock)
    if tuple(q.shape) != (rows, count) or tuple(err.shape) != (rows, count) or tuple(hinv.shape) != (count, count):
        raise RuntimeError("gptq_block: w, q, err must be [rows, count] and hinv [count, count]")
    if not (inv_d.is_cuda and inv_d.device == w.device and inv_d.dtype == torch.float32 and inv_d.is_contiguous()
            and inv_d.numel() == nmb * microblock * microblock):
        raise RuntimeError(f"gptq_block: inv_d must be a contiguous float32 [{nmb}, {microblock}, {microblock}] tensor on w's GPU")
    if scale is not None and not (scale.is_cuda and scale.device == w.device and scale.dtype == torch.float32 and scale.is_contiguous()):
        raise RuntimeError("gptq_block: scale must be a contiguous float32 tensor on w's GPU")
    if zero_point is not None and not (zero_point.is_cuda and zero_point.device == w.device and zero_point.dtype == torch.int64
                                       and zero_point.is_contiguous()):
        raise RuntimeError("gptq_block: zero_point must be a contiguous int64 tensor on w's GPU")
    if f.kind == _lib.GPTQ_FIXED:
        need = rows if f.per_row else 1
        if scale is None or zero_point is None or scale.numel() < need or zero_point.numel() < need:
            raise RuntimeError("gptq_block: a fixed point cast needs its scale and zero point (one per row when per_row)")

    def ld(t):
        return max(t.stride(0), count) if t.shape[0] <= 1 else t.stride(0)

    check(lib().dmxq_gptq_block(ptr(w), ld(w), ptr(q), ld(q), ptr(err), ld(err), rows, count, ptr(hinv), ld(hinv), ptr(inv_d), microblock,
                                ctypes.byref(f), ptr(scale), ptr(zero_point), stream_of(w)), "dmxq_gptq_block")


@_guarded
def gptq_block_dynamic(w, hinv, inv_d, microblock, fmt, rounding, group, qmin, qmax, symmetric_qscheme, q, err, scale_out, zp_out):
    what = "gptq_block_dynamic"
    require_gpu(w, what)
    for t, name in ((w, "w"), (hinv, "hinv"), (q, "q"), (err, "err"), (scale_out, "scale_out")):
        if not (t.is_cuda and t.device == w.device and t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)):
            raise RuntimeError(f"{what}: {name} must be a float32 matrix with unit column stride on w's GPU")
    f = _gptq_format(fmt, what)
    if microblock < 1 or group < 1:
        raise RuntimeError(f"{what}: microblock and group must be positive")
    rows, count = w.shape
    nmb, ng = -(-count // microblock), count // group
    if tuple(q.shape) != (rows, count) or tuple(err.shape) != (rows, count) or tuple(hinv.shape) != (count, count):
        raise RuntimeError(f"{what}: w, q, err must be [rows, count] and hinv [count, count]")
    if not (inv_d.is_cuda and inv_d.device == w.device and inv_d.dtype == torch.float32 and inv_d.is_contiguous()
            and inv_d.numel() == nmb * microblock * microblock):
        raise RuntimeError(f"{what}: inv_d must be a contiguous float32 [{nmb}, {microblock}, {microblock}] tensor on w's GPU")
    if not (zp_out.is_cuda and zp_out.device == w.device and zp_out.dtype == torch.int64 and zp_out.dim() == 2
            and (zp_out.shape[1] <= 1 or zp_out.stride(1) == 1)):
        raise RuntimeError(f"{what}: zp_out must be an int64 matrix with unit column stride on w's GPU")
    if tuple(scale_out.shape) != (rows, ng) or tuple(zp_out.shape) != (rows, ng):
        raise RuntimeError(f"{what}: scale_out and zp_out must be [rows, count / group] = [{rows}, {ng}]")

    def ld(t, n):
        return max(t.stride(0), n) if t.shape[0] <= 1 else t.stride(0)

    check(lib().dmxq_gptq_block_dynamic(ptr(w), ld(w, count), ptr(q), ld(q, count), ptr(err), ld(err, count), rows, count, ptr(hinv),
                                        ld(hinv, count), ptr(inv_d), microblock, ctypes.byref(f), int(rounding), int(group), int(qmin), int(qmax),
                                        int(bool(symmetric_qscheme)), ptr(scale_out), ld(scale_out, ng), ptr(zp_out), ld(zp_out, ng),
                                        stream_of(w)), "dmxq_gptq_block_dynamic")


# ------------------------------------------------------------------------------------------------ HistogramObserver
def _hist_state(t, like, dtype, numel, what, op):
    if not (t.is_cuda and t.device == like.device and t.dtype == dtype and t.is_contiguous() and t.numel() == numel):
        raise RuntimeError(f"{op}: {what} must be a contiguous {dtype} tensor of {numel} entries on the input's device")


@_guarded
def hist_observe(x, ch_axis, group_size, upsample_rate, hist, min_val, max_val, status, scratch):
    xc = _prep(x, "hist_observe")
    if group_size < 1 or upsample_rate < 1:
        raise RuntimeError("hist_observe: group_size and upsample_rate must be positive")
    outer, C, inner = _split(xc, ch_axis)
    G = -(-C // group_size)
    if not (G >= 1 and hist.numel() >= G and hist.numel() % G == 0):
        raise RuntimeError(f"hist_observe: the histogram must hold {G} groups of bins")
    _hist_state(hist, xc, torch.float32, hist.numel(), "hist", "hist_observe")
    _hist_state(min_val, xc, torch.float32, G, "min_val", "hist_observe")
    _hist_state(max_val, xc, torch.float32, G, "max_val", "hist_observe")
    _hist_state(status, xc, torch.int32, 1, "status", "hist_observe")
    if not (scratch.is_cuda and scratch.device == xc.device and scratch.is_contiguous()):
        raise RuntimeError("hist_observe: scratch must be a contiguous tensor on the input's device")
    check(lib().dmxq_hist_observe(ptr(xc), dtype_code(xc.dtype), outer, C, inner, group_size, hist.numel() // G, upsample_rate, ptr(hist),
                                  ptr(min_val), ptr(max_val), ptr(status), ptr(scratch), scratch.numel() * scratch.element_size(),
                                  stream_of(xc)), "dmxq_hist_observe")


@_guarded
def hist_qparams(hist, min_val, max_val, precision, qmin, qmax, symmetric_qscheme):
    require_gpu(hist, "hist_qparams")
    G = min_val.numel()
    if not (G >= 1 and hist.numel() >= G and hist.numel() % G == 0):
        raise RuntimeError(f"hist_qparams: the histogram must hold {G} groups of bins")
    _hist_state(hist, hist, torch.float32, hist.numel(), "hist", "hist_qparams")
    _hist_state(min_val, hist, torch.float32, G, "min_val", "hist_qparams")
    _hist_state(max_val, hist, torch.float32, G, "max_val", "hist_qparams")
    scale = torch.empty(G, dtype=torch.float32, device=hist.device)
    zp = torch.empty(G, dtype=torch.int64, device=hist.device)
    check(lib().dmxq_hist_qparams(ptr(hist), ptr(min_val), ptr(max_val), G, hist.numel() // G, precision, qmin, qmax, int(symmetric_qscheme),
                                  ptr(scale), ptr(zp), stream_of(hist)), "dmxq_hist_qparams")
    return scale, zp


# ------------------------------------------------------------------------------------------------ error statistics
def _error_rows(stats, scratch, like, rows, op):
    if not (stats.is_cuda and stats.device == like.device and stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == 4 * rows):
        raise RuntimeError(f"{op}: stats must be a contiguous float64 tensor of {rows} x 4 entries on the input's device")
    if not (scratch.is_cuda and scratch.device == like.device and scratch.is_contiguous()):
        raise RuntimeError(f"{op}: scratch must be a contiguous tensor on the input's device")


@_guarded
def error_stats(ref, test, accumulate, stats, scratch):
    rc, tc = _prep(ref, "error_stats"), _prep(test, "error_stats")
    if rc.device != tc.device or rc.numel() != tc.numel():
        raise RuntimeError("error_stats: ref and test must hold the same number of elements on one device")
    _error_rows(stats, scratch, rc, 1, "error_stats")
    check(lib().dmxq_error_stats(ptr(rc), dtype_code(rc.dtype), ptr(tc), dtype_code(tc.dtype), rc.numel(), int(bool(accumulate)), ptr(stats),
                                 ptr(scratch), scratch.numel() * scratch.element_size(), stream_of(rc)), "dmxq_error_stats")


@_guarded
def cast_error(x, fmts, scale, zero_point, accumulate, stats, scratch):
    xc = _prep(x, "cast_error")
    if not fmts or len(fmts) % 12:
        raise RuntimeError("cast_error: fmts is the 12 fields of dmxq_gptq_format per format")
    K = len(fmts) // 12
    _error_rows(stats, scratch, xc, K, "cast_error")
    if scale is not None and not (scale.is_cuda and scale.device == xc.device and scale.dtype == torch.float32 and scale.is_contiguous()
                                  and scale.numel() >= K):
        raise RuntimeError("cast_error: scale must be a contiguous float32 tensor with an entry per format on x's GPU")
    if zero_point is not None and not (zero_point.is_cuda and zero_point.device == xc.device and zero_point.dtype == torch.int64
                                       and zero_point.is_contiguous() and zero_point.numel() >= K):
        raise RuntimeError("cast_error: zero_point must be a contiguous int64 tensor with an entry per format on x's GPU")
    f = (_lib.GptqFormat * K)(*[_gptq_format(fmts[12 * k:12 * k + 12], "cast_error") for k in range(K)])
    L = xc.shape[-1] if xc.dim() else 1
    rows = xc.numel() // L if L else 0
    check(lib().dmxq_cast_error(ptr(xc), dtype_code(xc.dtype), rows, L, ctypes.cast(f, ctypes.c_void_p), K, ptr(scale), ptr(zero_point),
                                int(bool(accumulate)), ptr(stats), ptr(scratch), scratch.numel() * scratch.element_size(), stream_of(xc)),
          "dmxq_cast_error")


# ------------------------------------------------------------------------------------------------ Hadamard rotation
@_guarded
def hadamard_qdq(x, size, inverse, fmt, scale, zero_point, out_dtype=None):
    xc = _prep(x, "hadamard_qdq")
    if fmt and len(fmt) != 12:
        raise RuntimeError("hadamard_qdq: fmt is empty (rotation only) or the 12 fields of dmxq_gptq_format")
    if xc.dim() < 1:
        raise RuntimeError("hadamard_qdq: expects a tensor with at least one dimension")
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    L = xc.shape[-1]
    rows = xc.numel() // L if L else 0
    f = _gptq_format(fmt, "hadamard_qdq") if fmt else None
    if scale is not None and not (scale.is_cuda and scale.device == xc.device and scale.dtype == torch.float32 and scale.is_contiguous()):
        raise RuntimeError("hadamard_qdq: scale must be a contiguous float32 tensor on x's GPU")
    if zero_point is not None and not (zero_point.is_cuda and zero_point.device == xc.device and zero_point.dtype == torch.int64
                                       and zero_point.is_contiguous()):
        raise RuntimeError("hadamard_qdq: zero_point must be a contiguous int64 tensor on x's GPU")
    if f is not None and f.kind == _lib.GPTQ_FIXED:
        need = rows if f.per_row else 1
        if scale is None or zero_point is None or scale.numel() < need or zero_point.numel() < need:
            raise RuntimeError("hadamard_qdq: a fixed point cast needs its scale and zero point (one per row when per_row)")
    check(lib().dmxq_hadamard_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), rows, L, size, int(bool(inverse)),
                                  ctypes.byref(f) if f is not None else None, ptr(scale), ptr(zero_point), stream_of(xc)), "dmxq_hadamard_qdq")
    return out


# ------------------------------------------------------------------------------------------------ dynamic integer cast
@_guarded
def dynamic_fixed_qdq(x, segment, whole_rows, precision, fraction, clamp, symmetric, rounding, qmin, qmax, symmetric_qscheme, want_qparams,
                      out_dtype=None):
    xc = _prep(x, "dynamic_fixed_qdq")
    if segment < 1 or xc.numel() % segment != 0:
        raise RuntimeError("dynamic_fixed_qdq: the segment must divide the number of elements")
    n = xc.numel() // segment
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = torch.empty(n if want_qparams else 0, dtype=torch.float32, device=xc.device)
    zp = torch.empty(n if want_qparams else 0, dtype=torch.int64, device=xc.device)
    check(lib().dmxq_dynamic_fixed_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), n, segment, int(bool(whole_rows)),
                                       precision, fraction, int(bool(clamp)), int(bool(symmetric)), rounding, qmin, qmax,
                                       int(bool(symmetric_qscheme)), ptr(sc) if want_qparams else None, ptr(zp) if want_qparams else None,
                                       stream_of(xc)), "dmxq_dynamic_fixed_qdq")
    return out, sc, zp


# ------------------------------------------------------------------------------------------------ learned step size (backward)
@_guarded
def lsq_backward(x, g, scale, zero_point, segment, whole_rows, precision, rounding, qmin, qmax, grad_factor, want_dz, want_dx):
    """-> (dx, empty unless want_dx; ds float32 [n_segments]; dz float32 [n_segments], empty unless want_dz)"""
    xc, gc = _prep(x, "lsq_backward"), _prep(g, "lsq_backward")
    if gc.device != xc.device or gc.numel() != xc.numel():
        raise RuntimeError("lsq_backward: x and g must hold the same number of elements on one device")
    if segment < 1 or xc.numel() % segment != 0:
        raise RuntimeError("lsq_backward: the segment must divide the number of elements")
    n = xc.numel() // segment
    for t in (scale, zero_point):
        if not (t.is_cuda and t.device == xc.device and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
            raise RuntimeError(f"lsq_backward: scale and zero_point must be contiguous float32 tensors of {n} entries on x's GPU")
    dx = torch.empty(xc.shape if want_dx else 0, dtype=xc.dtype, device=xc.device)
    ds = torch.empty(n, dtype=torch.float32, device=xc.device)
    dz = torch.empty(n if want_dz else 0, dtype=torch.float32, device=xc.device)
    sb = int(lib().dmxq_lsq_scratch_bytes(segment)) if whole_rows == 2 else 0
    scratch = torch.empty(sb // 8, dtype=torch.float64, device=xc.device)
    check(lib().dmxq_lsq_backward(ptr(xc), ptr(gc), ptr(dx) if want_dx else None, dtype_code(xc.dtype), dtype_code(gc.dtype), dtype_code(dx.dtype), n, segment,
                                  int(whole_rows), precision, rounding, qmin, qmax, ptr(scale), ptr(zero_point), float(grad_factor),
                                  int(bool(want_dz)), ptr(ds), ptr(dz) if want_dz else None, ptr(scratch) if sb else None, sb, stream_of(xc)),
          "dmxq_lsq_backward")
    return dx, ds, dz


# ------------------------------------------------------------------------------------------------ dynamic scaled float cast
DYNF_GROUP, DYNF_ROWS, DYNF_TILE = 0, 1, 2   # dmxq_dynamic_float_mode (include/dmxq.h)


@_guarded
def dynamic_float_qdq(x, mode, segment, man, exp, bias, flush_subnormal, rounding, pow2_scale, want_scale, out_dtype=None):
    """-> (out, scale): scale float32 [n_segments] ([..., R / g, C / g] for tiles), empty unless want_scale"""
    xc = _prep(x, "dynamic_float_qdq")
    if segment < 1:
        raise RuntimeError("dynamic_float_qdq: the segment must be positive")
    rows = cols = 0
    if mode == DYNF_TILE:
        if xc.dim() < 2 or xc.shape[-2] % segment or xc.shape[-1] % segment:
            raise RuntimeError("dynamic_float_qdq: the tile size must divide the last two dimensions")
        cols = xc.shape[-1]
        rows = xc.numel() // cols
        sc_shape = tuple(xc.shape[:-2]) + (xc.shape[-2] // segment, cols // segment)
        n = (rows // segment) * (cols // segment)
    else:
        if xc.numel() % segment != 0:
            raise RuntimeError("dynamic_float_qdq: the segment must divide the number of elements")
        n = xc.numel() // segment
        sc_shape = (n,)
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = torch.empty(sc_shape if want_scale else 0, dtype=torch.float32, device=xc.device)
    check(lib().dmxq_dynamic_float_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), mode, n, segment, rows, cols, man, exp,
                                       bias, int(bool(flush_subnormal)), rounding, int(bool(pow2_scale)), ptr(sc) if want_scale else None,
                                       stream_of(xc)), "dmxq_dynamic_float_qdq")
    return out, sc


# ------------------------------------------------------------------------------------------------ codebook casts
def _codebook_args(xc, segment, levels, what):
    if segment < 1 or xc.numel() % segment != 0:
        raise RuntimeError(f"{what}: the segment must divide the number of elements")
    if not (levels.is_cuda and levels.device == xc.device and levels.dtype == torch.float32 and levels.is_contiguous() and levels.dim() == 1):
        raise RuntimeError(f"{what}: the levels must be a contiguous 1-d float32 tensor on x's GPU")


@_guarded
def codebook_qdq(x, mode, segment, levels, norm, want_scale, want_index, out_dtype=None):
    """-> (out, scale float32 [n_segments], index uint8 in x's shape): the last two empty unless wanted"""
    xc = _prep(x, "codebook_qdq")
    _codebook_args(xc, segment, levels, "codebook_qdq")
    n = xc.numel() // segment
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = torch.empty(n if want_scale else 0, dtype=torch.float32, device=xc.device)
    idx = torch.empty(xc.shape if want_index else 0, dtype=torch.uint8, device=xc.device)
    check(lib().dmxq_codebook_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), mode, n, segment, ptr(levels), levels.numel(),
                                  float(norm), ptr(sc) if want_scale else None, ptr(idx) if want_index else None, stream_of(xc)),
          "dmxq_codebook_qdq")
    return out, sc, idx


@_guarded
def codebook_accumulate(x, mode, segment, levels, norm, acc, accumulate):
    """acc (float64 [K, 3]) (+)= the Lloyd statistics of x under the table; the partial rows' workspace is allocated here"""
    xc = _prep(x, "codebook_accumulate")
    _codebook_args(xc, segment, levels, "codebook_accumulate")
    if not (acc.is_cuda and acc.device == xc.device and acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == levels.numel() * 3):
        raise RuntimeError("codebook_accumulate: acc must be a contiguous float64 [K, 3] tensor on x's GPU")
    n = xc.numel() // segment
    wb = int(lib().dmxq_codebook_workspace_bytes(dtype_code(xc.dtype), mode, n, segment))
    ws = torch.empty(wb // 8 + 1, dtype=torch.float64, device=xc.device)
    check(lib().dmxq_codebook_accumulate(ptr(xc), dtype_code(xc.dtype), mode, n, segment, ptr(levels), levels.numel(), float(norm), ptr(acc),
                                         int(bool(accumulate)), ptr(ws), stream_of(xc)), "dmxq_codebook_accumulate")


# ------------------------------------------------------------------------------------------------ vector codebook casts
def _vq_args(xc, segment, table, what):
    if segment < 1 or xc.numel() % segment != 0:
        raise RuntimeError(f"{what}: the segment must divide the number of elements")
    if not (table.is_cuda and table.device == xc.device and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2
            and table.shape[1] >= 1):
        raise RuntimeError(f"{what}: the table must be a contiguous float32 [K, d] tensor on x's GPU")
    if xc.dim() < 1 or xc.shape[-1] % table.shape[1] != 0:
        raise RuntimeError(f"{what}: the last dimension must be a multiple of the table's d")


@_guarded
def vq_qdq(x, mode, segment, table, norm, want_scale, want_index, out_dtype=None):
    """-> (out, scale float32 [n_segments], index uint8 x.shape[:-1] + (L / d,)): the last two empty unless wanted"""
    xc = _prep(x, "vq_qdq")
    _vq_args(xc, segment, table, "vq_qdq")
    K, d = table.shape
    n = xc.numel() // segment
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = torch.empty(n if want_scale else 0, dtype=torch.float32, device=xc.device)
    idx = torch.empty(tuple(xc.shape[:-1]) + (xc.shape[-1] // d,) if want_index else 0, dtype=torch.uint8, device=xc.device)
    check(lib().dmxq_vq_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), mode, n, segment, ptr(table), d, K, float(norm),
                            ptr(sc) if want_scale else None, ptr(idx) if want_index else None, stream_of(xc)), "dmxq_vq_qdq")
    return out, sc, idx


@_guarded
def vq_accumulate(x, mode, segment, table, norm, acc, accumulate):
    """acc (float64 [K, d + 2]) (+)= the k-means statistics of x under the table; the partial blocks' workspace is allocated here"""
    xc = _prep(x, "vq_accumulate")
    _vq_args(xc, segment, table, "vq_accumulate")
    K, d = table.shape
    if not (acc.is_cuda and acc.device == xc.device and acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == K * (d + 2)):
        raise RuntimeError("vq_accumulate: acc must be a contiguous float64 [K, d + 2] tensor on x's GPU")
    n = xc.numel() // segment
    wb = int(lib().dmxq_vq_workspace_bytes(dtype_code(xc.dtype), mode, n, segment, d, K))
    ws = torch.empty(wb // 8 + 1, dtype=torch.float64, device=xc.device)
    check(lib().dmxq_vq_accumulate(ptr(xc), dtype_code(xc.dtype), mode, n, segment, ptr(table), d, K, float(norm), ptr(acc),
                                   int(bool(accumulate)), ptr(ws), stream_of(xc)), "dmxq_vq_accumulate")


# ------------------------------------------------------------------------------------------------ HQQ
@_guarded
def hqq_qdq(x, segment, rounding, qmin, qmax, lp_norm, beta, kappa, iters, want_qparams, want_codes, out_dtype=None):
    """-> (out, scale float32 [n_segments], zero float32 [n_segments], codes uint8 in x's shape): empty unless wanted"""
    xc = _prep(x, "hqq_qdq")
    if segment < 1 or xc.numel() % segment != 0:
        raise RuntimeError("hqq_qdq: the group size must divide the number of elements")
    n = xc.numel() // segment
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = torch.empty(n if want_qparams else 0, dtype=torch.float32, device=xc.device)
    zero = torch.empty(n if want_qparams else 0, dtype=torch.float32, device=xc.device)
    codes = torch.empty(xc.shape if want_codes else 0, dtype=torch.uint8, device=xc.device)
    check(lib().dmxq_hqq_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), n, segment, rounding, qmin, qmax, float(lp_norm),
                             float(beta), float(kappa), int(iters), ptr(sc) if want_qparams else None, ptr(zero) if want_qparams else None,
                             ptr(codes) if want_codes else None, stream_of(xc)), "dmxq_hqq_qdq")
    return out, sc, zero, codes


# ------------------------------------------------------------------------------------------------ outlier-aware dynamic cast
@_guarded
def outlier_fixed_qdq(x, segment, k, precision, fraction, clamp, symmetric, rounding, qmin, qmax, symmetric_qscheme, outlier_fmt, want_qparams,
                      want_outliers, out_dtype=None):
    """-> (out, scale float32 [n_segments], zero_point int64 [n_segments], idx int32 [n_segments, k], val [n_segments, k]): empty unless wanted"""
    xc = _prep(x, "outlier_fixed_qdq")
    if segment < 1 or xc.numel() % segment != 0:
        raise RuntimeError("outlier_fixed_qdq: the segment must divide the number of elements")
    if k < 0:
        raise RuntimeError("outlier_fixed_qdq: k must not be negative")
    n = xc.numel() // segment
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = torch.empty(n if want_qparams else 0, dtype=torch.float32, device=xc.device)
    zp = torch.empty(n if want_qparams else 0, dtype=torch.int64, device=xc.device)
    idx = torch.empty((n, k) if want_outliers else (0, k), dtype=torch.int32, device=xc.device)
    val = torch.empty((n, k) if want_outliers else (0, k), dtype=out.dtype, device=xc.device)
    (fo,), _keep = _fmt_ptrs(outlier_fmt)
    check(lib().dmxq_outlier_fixed_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), n, segment, int(k), precision, fraction,
                                       int(clamp), int(symmetric), rounding, qmin, qmax, int(symmetric_qscheme), fo,
                                       ptr(sc) if want_qparams else None, ptr(zp) if want_qparams else None,
                                       ptr(idx) if want_outliers else None, ptr(val) if want_outliers else None, stream_of(xc)),
          "dmxq_outlier_fixed_qdq")
    return out, sc, zp, idx, val


# ------------------------------------------------------------------------------------------------ Wanda
def _channel_sum(x, acc, scratch, entry, what):
    xc = _prep(x, what)
    C = xc.shape[-1] if xc.dim() else 1
    rows = xc.numel() // C if C else 0
    if not (acc.is_cuda and acc.device == xc.device and acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == C):
        raise RuntimeError(f"{what}: acc must be a contiguous float64 tensor of {C} entries on the input's device")
    need = lib().dmxq_channel_sumsq_workspace_bytes(rows, C)
    if not (scratch.is_cuda and scratch.device == xc.device and scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= need
            and scratch.data_ptr() % 8 == 0):
        raise RuntimeError(f"{what}: scratch must be a contiguous 8-byte aligned tensor of at least {need} bytes on the input's device")
    check(getattr(lib(), entry)(ptr(xc), dtype_code(xc.dtype), rows, C, ptr(acc), ptr(scratch), stream_of(xc)), entry)


@_guarded
def channel_sumsq(x, acc, scratch):
    """acc (float64 [C], C = x's last dim) += the sum of squares over every other dim; scratch: dmxq_channel_sumsq_workspace_bytes bytes of
    any contiguous device tensor"""
    _channel_sum(x, acc, scratch, "dmxq_channel_sumsq_accumulate", "channel_sumsq")


@_guarded
def channel_sumabs(x, acc, scratch):
    """the |x| twin of channel_sumsq (AWQ): same checks, same scratch"""
    _channel_sum(x, acc, scratch, "dmxq_channel_sumabs_accumulate", "channel_sumabs")


def _wanda_shapes(w, act_norm):
    if w.dim() != 2:
        raise RuntimeError("wanda_nm: the weight must be a [rows, L] matrix")
    if not (act_norm.is_cuda and act_norm.device == w.device and act_norm.dtype == torch.float32 and act_norm.is_contiguous()
            and act_norm.numel() == w.shape[1]):
        raise RuntimeError(f"wanda_nm: act_norm must be a contiguous float32 tensor of {w.shape[1]} entries on the weight's device")


@_guarded
def wanda_nm(w, act_norm, K, M, want_score, want_mask, want_y, mask_dtype=None, y_dtype=None):
    """-> (score float32, mask, y): an output that was not requested comes back as an empty 1-d tensor"""
    wc = _prep(w, "wanda_nm")
    _wanda_shapes(wc, act_norm)
    none = torch.empty(0, dtype=wc.dtype, device=wc.device)
    score = torch.empty(wc.shape, dtype=torch.float32, device=wc.device) if want_score else None
    mask = torch.empty(wc.shape, dtype=mask_dtype or torch.float32, device=wc.device) if want_mask else None
    y = torch.empty(wc.shape, dtype=y_dtype or torch.promote_types(wc.dtype, torch.float32), device=wc.device) if want_y else None
    check(lib().dmxq_wanda_nm(ptr(wc), dtype_code(wc.dtype), ptr(act_norm), ptr(score), ptr(mask), dtype_code(mask.dtype) if want_mask else 0,
                              ptr(y), dtype_code(y.dtype) if want_y else 0, wc.shape[0], wc.shape[1], K, M, stream_of(wc)), "dmxq_wanda_nm")
    return (score if want_score else none.float()), (mask if want_mask else none), (y if want_y else none)


# ------------------------------------------------------------------------------------------------ AWQ
@_guarded
def awq_group_error(w, s, group, precision, fraction, clamp, symmetric, qmin, qmax, symmetric_qscheme, want_wq):
    """-> (d float32, wq in w's dtype): wq comes back as an empty 1-d tensor when it was not requested"""
    wc = _prep(w, "awq_group_error")
    if wc.dim() != 2:
        raise RuntimeError("awq_group_error: the weight must be a [rows, L] matrix")
    if not (s.is_cuda and s.device == wc.device and s.dtype == torch.float32 and s.is_contiguous() and s.numel() == wc.shape[1]):
        raise RuntimeError(f"awq_group_error: s must be a contiguous float32 tensor of {wc.shape[1]} entries on the weight's device")
    d = torch.empty(wc.shape, dtype=torch.float32, device=wc.device)
    wq = torch.empty(wc.shape if want_wq else 0, dtype=wc.dtype, device=wc.device)
    check(lib().dmxq_awq_group_error(ptr(wc), dtype_code(wc.dtype), ptr(s), ptr(d), ptr(wq) if want_wq else None, wc.shape[0], wc.shape[1], group,
                                     precision, fraction, int(bool(clamp)), int(bool(symmetric)), qmin, qmax, int(bool(symmetric_qscheme)),
                                     stream_of(wc)), "dmxq_awq_group_error")
    return d, wq


@_guarded
def awq_clip(w, blocks, ratios, y, group, precision, fraction, clamp, symmetric, qmin, qmax, symmetric_qscheme, want_best, want_clip, want_losses):
    """y (w's dtype and shape, may be w) is written -> (best uint8 [rows, G], clip float32 [rows, G], losses float32 [rows, G, n]): empty
    unless wanted"""
    wc = _prep(w, "awq_clip")
    if wc.dim() != 2 or group < 1 or wc.shape[1] % group != 0:
        raise RuntimeError("awq_clip: the weight must be a [rows, L] matrix with the group size dividing L")
    rows, G, n = wc.shape[0], wc.shape[1] // group, ratios.numel()
    for t, shape, what in ((blocks, (G, group, group), "blocks"), (ratios, (n,), "ratios")):
        if not (t.is_cuda and t.device == wc.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError(f"awq_clip: {what} must be a contiguous float32 {list(shape)} tensor on the weight's device")
    if not (y.is_cuda and y.device == wc.device and y.dtype == wc.dtype and y.is_contiguous() and y.shape == wc.shape):
        raise RuntimeError("awq_clip: y must be a contiguous tensor of the weight's dtype and shape on its device")
    best = torch.empty((rows, G) if want_best else 0, dtype=torch.uint8, device=wc.device)
    clip = torch.empty((rows, G) if want_clip else 0, dtype=torch.float32, device=wc.device)
    losses = torch.empty((rows, G, n) if want_losses else 0, dtype=torch.float32, device=wc.device)
    check(lib().dmxq_awq_clip(ptr(wc), dtype_code(wc.dtype), ptr(blocks), ptr(ratios), n, ptr(y), ptr(best) if want_best else None,
                              ptr(clip) if want_clip else None, ptr(losses) if want_losses else None, rows, wc.shape[1], group, precision,
                              fraction, int(bool(clamp)), int(bool(symmetric)), qmin, qmax, int(bool(symmetric_qscheme)), stream_of(wc)),
          "dmxq_awq_clip")
    return best, clip, losses


# ------------------------------------------------------------------------------------------------ AdaRound
def _adaround_args(wc, V, scale, zero_point, segment, what):
    if segment < 1 or wc.numel() % segment != 0:
        raise RuntimeError(f"{what}: the segment must divide the number of elements")
    n = wc.numel() // segment
    if not (V.is_cuda and V.device == wc.device and V.dtype == torch.float32 and V.is_contiguous() and V.numel() == wc.numel()):
        raise RuntimeError(f"{what}: V must be a contiguous float32 tensor of the weight's element count on its GPU")
    for t in (scale, zero_point):
        if not (t.is_cuda and t.device == wc.device and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
            raise RuntimeError(f"{what}: scale and zero_point must be contiguous float32 tensors of {n} entries on the weight's GPU")
    return n


@_guarded
def adaround_forward(w, V, scale, zero_point, segment, qmin, qmax, hard, out_dtype=None):
    """-> y in out_dtype (the weight's dtype by default) and w's shape"""
    wc = _prep(w, "adaround_forward")
    n = _adaround_args(wc, V, scale, zero_point, segment, "adaround_forward")
    y = torch.empty(wc.shape, dtype=out_dtype or wc.dtype, device=wc.device)
    check(lib().dmxq_adaround_forward(ptr(wc), ptr(V), ptr(y), dtype_code(wc.dtype), dtype_code(y.dtype), n, segment, qmin, qmax, ptr(scale),
                                      ptr(zero_point), int(bool(hard)), stream_of(wc)), "dmxq_adaround_forward")
    return y


@_guarded
def adaround_backward(w, V, g, scale, zero_point, segment, qmin, qmax, beta, reg_weight, want_reg):
    """-> (dV float32 in w's shape; reg float64 [1], empty unless want_reg)"""
    wc, gc = _prep(w, "adaround_backward"), _prep(g, "adaround_backward")
    if gc.device != wc.device or gc.numel() != wc.numel():
        raise RuntimeError("adaround_backward: w and g must hold the same number of elements on one device")
    n = _adaround_args(wc, V, scale, zero_point, segment, "adaround_backward")
    dV = torch.empty(wc.shape, dtype=torch.float32, device=wc.device)
    reg = torch.empty(1 if want_reg else 0, dtype=torch.float64, device=wc.device)
    sb = int(lib().dmxq_adaround_scratch_bytes(wc.numel())) if want_reg else 0
    scratch = torch.empty(sb // 8, dtype=torch.float64, device=wc.device)
    check(lib().dmxq_adaround_backward(ptr(wc), ptr(V), ptr(gc), ptr(dV), dtype_code(wc.dtype), dtype_code(gc.dtype), n, segment, qmin, qmax,
                                       ptr(scale), ptr(zero_point), float(beta), float(reg_weight), ptr(reg) if want_reg else None,
                                       ptr(scratch) if sb else None, sb, stream_of(wc)), "dmxq_adaround_backward")
    return dV, reg


# ------------------------------------------------------------------------------------------------ block-scaled float cast
@_guarded
def block_scaled_float_qdq(x, group, fmt, scale_fmt, scale_max, tensor_scale, want_scale, want_code, out_dtype=None):
    """-> (out, scale, scale_code_value): float32 [n_groups] each, empty unless wanted; fmt / scale_fmt: (man, exp, bias, flush, rounding);
    tensor_scale: None or ONE float32 on x's device (read by the kernel only)"""
    xc = _prep(x, "block_scaled_float_qdq")
    if len(fmt) != 5 or len(scale_fmt) != 5:
        raise RuntimeError("block_scaled_float_qdq: a format is (man, exp, bias, flush, rounding)")
    if group < 1 or xc.numel() % group != 0:
        raise RuntimeError("block_scaled_float_qdq: the group must divide the number of elements")
    if tensor_scale is not None and not (tensor_scale.is_cuda and tensor_scale.device == xc.device and tensor_scale.dtype == torch.float32
                                         and tensor_scale.numel() == 1):
        raise RuntimeError("block_scaled_float_qdq: tensor_scale must be ONE float32 on the input's device")
    n = xc.numel() // group
    out = torch.empty(xc.shape, dtype=out_dtype or xc.dtype, device=xc.device)
    sc = torch.empty(n if want_scale else 0, dtype=torch.float32, device=xc.device)
    sq = torch.empty(n if want_code else 0, dtype=torch.float32, device=xc.device)
    check(lib().dmxq_block_scaled_float_qdq(ptr(xc), ptr(out), dtype_code(xc.dtype), dtype_code(out.dtype), n, group, *[int(v) for v in fmt],
                                            *[int(v) for v in scale_fmt], float(scale_max), ptr(tensor_scale) if tensor_scale is not None else None,
                                            ptr(sc) if want_scale else None, ptr(sq) if want_code else None, stream_of(xc)),
          "dmxq_block_scaled_float_qdq")
    return out, sc, sq


@_guarded
def block_scaled_tensor_scale(x, fmax, scale_max):
    """-> float32 [1]: (max |x| / fmax) / scale_max over the whole contiguous tensor, 1 where not finite or below 2^-126"""
    xc = _prep(x, "block_scaled_tensor_scale")
    t = torch.empty(1, dtype=torch.float32, device=xc.device)
    check(lib().dmxq_block_scaled_tensor_scale(ptr(xc), dtype_code(xc.dtype), xc.numel(), float(fmax), float(scale_max), ptr(t), stream_of(xc)),
          "dmxq_block_scaled_tensor_scale")
    return t
