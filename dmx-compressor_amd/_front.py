"""The tensor-level front ends of the library, written ONCE for both bindings of the C ABI (include/dmxq.h).

Every function here is the Python spelling of one (or two) dispatcher ops -- rounding names, torch dtypes, Format objects, the
`DmxqError` for non-GPU tensors, seeds for stochastic rounding, "None when not fusable" -- over a RAW namespace `_ops` whose
functions carry the schema of `torch.ops.dmxq.*` (csrc/torch_binding.cpp):
  * `_backend_torch.RAW`   the TORCH_LIBRARY extension `lib/dmxq_torch.so` (meta kernels, registered straight-through backward);
  * `_backend_ctypes`      the same schema in Python over plain ctypes (no compiler against the torch headers needed).
`ops.py` binds one of them (`DMXQ_BINDING=torch|ctypes`).  A new entry point is therefore written in the C ABI, in the two bindings
(which only allocate and call) and HERE -- not, as until round 3, as two complete front ends.

No CPU path: a non-GPU tensor or a missing library raises `DmxqError`.
"""
import math
from typing import Optional

import torch

from ._lib import DmxqError, ROUNDING_CODE, require_gpu

__all__ = [
    "bfp_qdq", "block_quantize", "bfp_qdq_multi", "bfp_pack", "bfp_unpack", "weight_hypernet", "weight_hypernet_multi", "input_hypernet", "binary_cast", "rope_cast", "relu_cast", "unary_cast", "unary_cast_table", "lut16_apply", "softmax_cast", "layernorm_cast", "rmsnorm_cast", "sbfp_qdq", "mxfp_qdq", "float_qdq", "float_qdq_multi", "fixed_qdq", "fixed_qdq_multi", "fixed_float_qdq_multi", "nm_mask", "nm_sparsify", "nm_mask_class", "topk_mask", "topk_sparsify", "bernoulli_mask", "group_minmax", "group_minmax_accumulate", "qparams", "channel_maxabs",
    "smoothquant_scale", "scale_channels", "gelu", "silu", "quick_gelu", "exp", "silu_experimental", "rope", "softmax", "layernorm",
    "rmsnorm", "histc", "gptq_fields", "gptq_block", "gptq_block_dynamic", "hist_observe", "hist_scratch_words", "hist_qparams", "error_stats", "cast_error",
    "error_scratch_bytes", "cast_error_entry", "hadamard", "hadamard_qdq", "hadamard_check_size", "HADAMARD_SIZES",
    "dynamic_fixed_qdq", "dynamic_check", "dynamic_class", "DYNAMIC_GRANULARITIES", "DYNAMIC_CHAIN_BY_DEFAULT",
    "dynamic_float_qdq", "dynamic_float_check", "dynamic_float_class", "dynamic_float_fmax", "DYNAMIC_FLOAT_GRANULARITIES",
    "DYNAMIC_FLOAT_CHAIN_BY_DEFAULT",
    "codebook_qdq", "codebook_check", "codebook_class", "codebook_accumulate", "codebook_fit", "CODEBOOKS", "NF4", "CODEBOOK_GRANULARITIES",
    "CODEBOOK_KERNEL_LEVELS", "CODEBOOK_CHAIN_BY_DEFAULT",
    "vq_qdq", "vq_check", "vq_grid", "vq_class", "vq_accumulate", "vq_fit", "VQ_DIMS", "VQ_CHAIN_BY_DEFAULT", "VQ_CHAIN_PIECE_ENTRIES",
    "hqq_qdq", "hqq_check", "hqq_class", "HQQ_CHAIN_BY_DEFAULT", "HQQ_KERNEL_NORMS",
    "outlier_fixed_qdq", "outlier_check", "outlier_class", "outlier_bits_per_element", "OUTLIER_CHAIN_BY_DEFAULT", "OUTLIER_KERNEL_MAX_K",
    "lsq_backward", "lsq_fixed_qdq", "lsq_class", "lsq_scratch_bytes", "lsq_grad_factor", "LSQ_CHAIN_BY_DEFAULT",
    "block_scaled_float_qdq", "block_scaled_tensor_scale", "block_scaled_float_class", "block_scaled_check", "NVFP4",
    "BLOCK_SCALED_CHAIN_BY_DEFAULT",
    "channel_sumsq", "channel_sumsq_workspace_bytes", "wanda_score", "wanda_nm_sparsify", "wanda_class", "WANDA_CHAIN_BY_DEFAULT",
    "channel_sumabs", "awq_candidate_scales", "awq_scaled_error", "awq_class", "awq_search", "AWQ_CHAIN_BY_DEFAULT",
    "awq_clip", "awq_clip_check", "awq_clip_class", "awq_clip_ratios", "awq_gram_blocks", "AWQ_CLIP_CHAIN_BY_DEFAULT", "AWQ_CLIP_MAX_RATIOS",
    "adaround_check", "adaround_class", "adaround_scratch_bytes", "adaround_init", "adaround_qdq", "adaround_backward",
    "ADAROUND_CHAIN_BY_DEFAULT",
]

_ops = None   # the raw namespace: set by bind()


def bind(raw) -> None:
    """ops.py hands over the binding's raw namespace (torch.ops.dmxq overloads, or the _backend_ctypes module)"""
    global _ops
    _ops = raw


_SEED_COUNTER = [0x5EED]


def _next_seed() -> int:
    """Stochastic rounding draws from a counter-based stream keyed by (seed, element index); a fresh seed per call,
    derived from `torch.initial_seed()` (the DEFAULT generator's seed: `torch.manual_seed` makes runs reproducible; a
    non-default `torch.Generator` is not consulted -- pass `seed=` explicitly for that).

    The seed is a kernel ARGUMENT, so a hipGraph capture would freeze it and every replay would repeat the same draws
    (accumulated rounding would no longer be unbiased): implicit seeding is refused while the current stream is
    capturing.  An explicit `seed=` is the caller's statement that frozen draws are intended."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise DmxqError("stochastic rounding with an implicit seed inside a hipGraph capture: the seed would be frozen "
                        "into the graph and every replay would reuse the same random draws; pass seed= explicitly or "
                        "keep stochastic casts outside the captured region")
    _SEED_COUNTER[0] += 1
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + _SEED_COUNTER[0]) & 0xFFFFFFFFFFFFFFFF


def _seed_arg(seed, rounding):
    s = _next_seed() if (seed is None and rounding == "stochastic") else (seed or 0)
    return s - (1 << 64) if s >= (1 << 63) else s  # the schema's int is int64: same 64 bits


# ---------------------------------------------------------------------------------------------------- block formats
def bfp_qdq(x, precision: int, block_size: int, block_dim: int = -1, symmetric: bool = True,
            rounding: str = "nearest", out_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None):
    """BlockFloatingPoint Q->DQ of a whole tensor in one launch (numerical/format.py:304-343 semantics).
    Blocks run along `block_dim`; output has x's shape, contiguous, dtype `out_dtype` (default x.dtype)."""
    require_gpu(x, "bfp_qdq")
    op = _ops.bfp_qdq if (x.requires_grad and torch.is_grad_enabled()) else _ops.bfp_qdq_nograd   # (the STE wrapper costs ~2.5 us per call)
    return op(x, precision, block_size, block_dim, symmetric, ROUNDING_CODE[rounding], out_dtype, _seed_arg(seed, rounding))


def block_quantize(a2d, wl: int, symmetric: bool = True, rounding: str = "nearest", seed: Optional[int] = None):
    """The pybind seam on a [rows, L] float32 view, one block per row (quant_cpu.cpp:299-311).  symmetric False is the
    NATIVE asymmetric branch (:247-253), which is not the asymmetric FORMAT of bfp_qdq(symmetric=False)."""
    require_gpu(a2d, "block_quantize")
    return _ops.block_quantize(a2d, wl, symmetric, ROUNDING_CODE[rounding], _seed_arg(seed, rounding))


def bfp_qdq_multi(tensors, precision: int, block_size: int, block_dim: int = -1, symmetric: bool = True,
                  rounding: str = "nearest", out_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None):
    """BFP Q->DQ of MANY tensors of one dtype on one device in as few launches as possible (`dmxq_bfp_qdq_multi`): the
    same results as `[bfp_qdq(t, ...) for t in tensors]`."""
    tensors = list(tensors)
    if not tensors:
        return []   # (an empty Tensor[] carries no dispatch key)
    for t in tensors:
        require_gpu(t, "bfp_qdq_multi")
    if tensors and any(t.dtype != tensors[0].dtype or t.device != tensors[0].device for t in tensors):
        raise ValueError("bfp_qdq_multi: all tensors must share one dtype and one device")
    return list(_ops.bfp_qdq_multi(tensors, precision, block_size, block_dim, symmetric, ROUNDING_CODE[rounding], out_dtype,
                                   _seed_arg(seed, rounding)))


def bfp_pack(x, precision: int, block_size: int, symmetric: bool = True):
    """Packed on-wire BFP of a tensor blocked along its last dim: (int8 mantissa codes, same shape; uint8 shared
    exponents, [..., ceil(L / block_size)]).  bfp_unpack(*bfp_pack(x)) == bfp_qdq(x)."""
    require_gpu(x, "bfp_pack")
    return _ops.bfp_pack(x, precision, block_size, symmetric)


def bfp_unpack(mant, exps, precision: int, block_size: int, out_dtype: torch.dtype = torch.float32):
    require_gpu(mant, "bfp_unpack")
    return _ops.bfp_unpack(mant, exps, precision, block_size, out_dtype)


def weight_hypernet(w, precision: int, block_size: int, symmetric: bool = True, score=None, K: int = 0, M: int = 0,
                    sq_scale=None, out_dtype: Optional[torch.dtype] = None, block_dim: int = -1):
    """Fused N:M mask -> SmoothQuant scale -> BFP Q->DQ over a weight (one launch), everything along `block_dim`: the last dim
    (Linear) or any other (conv weights along in-channels: dmxq_weight_hypernet_strided).
    Returns None when the geometry / dtype combination is not fusable (the caller runs the unfused chain)."""
    require_gpu(w, "weight_hypernet")
    try:
        return _ops.weight_hypernet(w, precision, block_size, symmetric, score if M else None, K, M if score is not None else 0,
                                    sq_scale, out_dtype, block_dim)
    except NotImplementedError:
        return None


def weight_hypernet_multi(ws, precision: int, block_size: int, symmetric: bool = True, scores=None, K: int = 0, M: int = 0,
                          sq_scales=None, out_dtype: Optional[torch.dtype] = None):
    """The weight chain of MANY Linear weights (one dtype, one device, one N:M pattern, one BFP format) in as few launches as
    possible (`dmxq_weight_hypernet_multi`): the same results as `[weight_hypernet(w, ...) for w in ws]`.  scores / sq_scales: one
    per weight, or None.  Returns None -- nothing launched -- when any of them is not fusable (the caller goes one by one)."""
    ws = list(ws)
    if not ws:
        return []   # (an empty Tensor[] carries no dispatch key)
    for w in ws:
        require_gpu(w, "weight_hypernet_multi")
    try:
        return list(_ops.weight_hypernet_multi(ws, precision, block_size, symmetric, list(scores) if (scores is not None and M) else [],
                                               K, M if scores is not None else 0, list(sq_scales) if sq_scales is not None else [], out_dtype))
    except NotImplementedError:
        return None


def input_hypernet(x, sq_scale, precision: int, block_size: int, symmetric: bool = True):
    """Fused SmoothQuant input scaling -> BFP input cast along the last dim (one launch): BFP_QDQ(x / sq_scale) in float32, the
    dtype `a / scale` has in the reference (smoothquant.py:255-268).  None when the geometry is not fusable."""
    require_gpu(x, "input_hypernet")
    try:
        return _ops.input_hypernet(x, sq_scale, precision, block_size, symmetric)
    except NotImplementedError:
        return None


def _fmt4(f):
    return [] if f is None else [int(f.mantissa), int(f.exponent), int(f.bias), int(bool(f.flush_subnormal))]


def binary_cast(a, b, op: str, cast_a=None, cast_b=None, cast_out=None, then_bfp=None):
    """A binary DmxModule in one launch: cast_out(cast_a(a) op cast_b(b)), op in {"add", "mul"}; each cast is a FloatingPoint
    format (nearest, signed) or None = SAME.  then_bfp = (precision, block_size): the consumer's BFP input cast along the last dim in the
    same launch (dmxq_binary_cast_bfp).  None when not fusable (the caller runs the casts and the op one by one)."""
    require_gpu(a, "binary_cast")
    for f in (cast_a, cast_b, cast_out):
        if f is not None and (f.rounding != "nearest" or f.unsigned):
            return None
    try:
        return _ops.binary_cast(a, b, {"add": 0, "mul": 1}[op], _fmt4(cast_a), _fmt4(cast_b), _fmt4(cast_out),
                                int(then_bfp[1]) if then_bfp else 0, int(then_bfp[0]) if then_bfp else 0)
    except NotImplementedError:
        return None


def sbfp_qdq(x, precision: int, block_size: int, scaler_man: int, scaler_exp: int, scaler_bias: int,
             scaler_flush: bool = True, clamp: bool = True, symmetric: bool = True, block_dim: int = -1,
             out_dtype: Optional[torch.dtype] = None):
    """ScaledBlockFloatingPoint Q->DQ (numerical/format.py:453-479), one launch."""
    require_gpu(x, "sbfp_qdq")
    op = _ops.sbfp_qdq if (x.requires_grad and torch.is_grad_enabled()) else _ops.sbfp_qdq_nograd
    return op(x, precision, block_size, scaler_man, scaler_exp, scaler_bias, scaler_flush, clamp, symmetric, block_dim, out_dtype)


def mxfp_qdq(x, man: int, exp: int, block_size: int, block_dim: int = -1, out_dtype: Optional[torch.dtype] = None):
    """MXFP Q->DQ (numerical/format.py:545-564), one launch."""
    require_gpu(x, "mxfp_qdq")
    op = _ops.mxfp_qdq if (x.requires_grad and torch.is_grad_enabled()) else _ops.mxfp_qdq_nograd
    return op(x, man, exp, block_size, block_dim, out_dtype)


# ---------------------------------------------------------------------------------------------------- element formats
def float_qdq(x, man: int, exp: int, bias: int, flush_subnormal: bool, unsigned: bool = False,
              rounding: str = "nearest", out_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None):
    """Low-bit float Q->DQ (quant/quant_function.py:120-152 semantics), one launch."""
    require_gpu(x, "float_qdq")
    op = _ops.float_qdq if (x.requires_grad and torch.is_grad_enabled()) else _ops.float_qdq_nograd
    return op(x, man, exp, bias, flush_subnormal, unsigned, ROUNDING_CODE[rounding], out_dtype, _seed_arg(seed, rounding))


def fixed_qdq(x, precision: int, fraction: int, clamp: bool = True, symmetric: bool = True, rounding: str = "nearest",
              scale: Optional[torch.Tensor] = None, zero_point: Optional[torch.Tensor] = None,
              ch_axis: Optional[int] = None, group_size: Optional[int] = None,
              out_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None):
    """Fixed-point Q->DQ with the affine wrapper of numerical/cast.py:278-296 fused in, one launch.
    scale None: bare FixedPoint.cast.  ch_axis None: per-tensor scale; else per-channel (group_size None) or
    per-group slabs of `group_size` channels."""
    require_gpu(x, "fixed_qdq")
    op = _ops.fixed_qdq if (x.requires_grad and torch.is_grad_enabled()) else _ops.fixed_qdq_nograd
    return op(x, precision, fraction, clamp, symmetric, ROUNDING_CODE[rounding], scale, zero_point, ch_axis,
                          group_size or None, out_dtype, _seed_arg(seed, rounding))


def float_qdq_multi(tensors, mantissa: int, exponent: int, bias: Optional[int] = None, flush_subnormal: bool = True,
                    unsigned: bool = False, rounding: str = "nearest", out_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None):
    """Low-bit floating point Q->DQ (format.py:208-233) of MANY tensors of one dtype on one device in as few launches as possible
    (`dmxq_float_qdq_multi`): the same results as `[float_qdq(t, mantissa, exponent, bias, ...) for t in tensors]` -- the bias casts
    of a layer's modules (modeling/nn/core.py:191-203), a few hundred elements each, as ONE launch."""
    tensors = list(tensors)
    for t in tensors:
        require_gpu(t, "float_qdq_multi")
    if bias is None:
        bias = (1 << (exponent - 1)) - 1
    return list(_ops.float_qdq_multi(tensors, mantissa, exponent, bias, bool(flush_subnormal), bool(unsigned), ROUNDING_CODE[rounding],
                                     out_dtype, _seed_arg(seed, rounding)))


def fixed_qdq_multi(tensors, precision: int, fraction: int, clamp: bool, symmetric: bool, scales, zero_points,
                    group_size: Optional[int] = None, rounding: str = "nearest", out_dtype: Optional[torch.dtype] = None,
                    seed: Optional[int] = None):
    """Affine integer Q->DQ (numerical/cast.py:278-296) of MANY weights of one dtype on one device in as few launches as
    possible (`dmxq_fixed_qdq_multi`): the same results as `[fixed_qdq(t, ..., scale=s, zero_point=z, ch_axis=0 (or None when
    s has one entry), group_size=group_size) for t, s, z in zip(tensors, scales, zero_points)]`."""
    tensors = list(tensors)
    for t in tensors:
        require_gpu(t, "fixed_qdq_multi")
    return list(_ops.fixed_qdq_multi(tensors, precision, fraction, clamp, symmetric, ROUNDING_CODE[rounding], list(scales),
                                     list(zero_points), group_size or 0, out_dtype, _seed_arg(seed, rounding)))


def fixed_float_qdq_multi(tensors, precision: int, fraction: int, clamp: bool, symmetric: bool, scales, zero_points, group_size: Optional[int],
                          float_tensors, mantissa: int, exponent: int, bias: Optional[int] = None, flush_subnormal: bool = True,
                          unsigned: bool = False):
    """`fixed_qdq_multi(tensors, ...)` AND `float_qdq_multi(float_tensors, ...)` (nearest rounding both) in ONE launch where the set allows
    it (`dmxq_fixed_float_qdq_multi`: a layer's INT8 weight casts and its bias casts); -> (fixed results, float results), bit-identical to
    the two calls."""
    tensors, float_tensors = list(tensors), list(float_tensors)
    for t in tensors + float_tensors:
        require_gpu(t, "fixed_float_qdq_multi")
    if bias is None:
        bias = (1 << (exponent - 1)) - 1
    if not tensors or not float_tensors:
        # one of the sets is empty: exactly the two calls (decided HERE so that both bindings behave alike -- ADVICE r5: the torch
        # binding refused an empty list where the ctypes one fell back)
        return (fixed_qdq_multi(tensors, precision, fraction, clamp, symmetric, scales, zero_points, group_size=group_size) if tensors else [],
                float_qdq_multi(float_tensors, mantissa, exponent, bias, flush_subnormal, unsigned) if float_tensors else [])
    a, b = _ops.fixed_float_qdq_multi(tensors, precision, fraction, clamp, symmetric, ROUNDING_CODE["nearest"], list(scales), list(zero_points),
                                      group_size or 0, float_tensors, mantissa, exponent, bias, bool(flush_subnormal), bool(unsigned),
                                      ROUNDING_CODE["nearest"], 0)
    return list(a), list(b)


# ---------------------------------------------------------------------------------------------------- sparsity
def _nm(score, x, K, M, block_dim, want_mask, want_y, mask_dtype, y_dtype):
    require_gpu(score, "nm_mask")
    if score.dim() == 0 or score.shape[block_dim] % M != 0:
        # sparse.py:166-168
        raise AssertionError(
            f"score has size {tuple(score.shape)} at dimension {block_dim}, not a multiple of block size {M}")
    mask, y = _ops.nm_mask(score, x, K, M, block_dim, want_mask, want_y, mask_dtype, y_dtype)
    return (mask if want_mask else None), (y if want_y else None)


def nm_mask(score, K: int, M: int, block_dim: int = -1, mask_dtype: Optional[torch.dtype] = None):
    """N:M mask (sparse.py:163-180): float mask in the score's dtype."""
    return _nm(score, None, K, M, block_dim, True, False, mask_dtype, None)[0]


def nm_sparsify(x, score, K: int, M: int, block_dim: int = -1, out_dtype: Optional[torch.dtype] = None,
                return_mask: bool = False):
    """Fused mask + apply: y = x * mask(score) (sparse.py:287-301); out dtype defaults to torch's promotion of
    (x.dtype, score.dtype), i.e. what `x * mask` yields in the reference."""
    require_gpu(x, "nm_sparsify")
    mask, y = _nm(score, x, K, M, block_dim, return_mask, True, None, out_dtype)
    return (y, mask) if return_mask else y


def nm_mask_class(score, K: int, M: int, block_dim: int = -1, x=None, mask_dtype: Optional[torch.dtype] = None,
                  out_dtype: Optional[torch.dtype] = None, return_mask: Optional[bool] = None) -> str:
    """The kernel `nm_mask(score, K, M, block_dim, mask_dtype)` -- or, with `x`, `nm_sparsify(x, score, K, M, block_dim, out_dtype,
    return_mask)` -- launches: "typed", "f32_mask", "vector", "group_m", "any_m", or "none" for an empty tensor; asked of the library
    itself (dmxq_nm_mask_class, the function dmxq_nm_mask decides with; no GPU involved, tensors on any device: only dtypes, sizes and the
    alignment of the bases count).  The outputs are fresh allocations, so their bases are taken as 16-byte aligned, and so is the
    contiguous copy of an input that is not contiguous."""
    import ctypes

    from ._lib import NM_ROUTE_NAMES, check, dtype_code, lib, split3
    want_y = x is not None
    want_mask = (not want_y) if return_mask is None else bool(return_mask)
    outer, L, inner = split3(score.shape, block_dim) if score.dim() else (1, 1, 1)
    fresh = 0x100000    # (any 16-byte aligned address: never dereferenced)

    def base(t):
        return t.data_ptr() if t.is_contiguous() and t.numel() else fresh

    y_dtype = (out_dtype or torch.promote_types(x.dtype, score.dtype)) if want_y else score.dtype
    route = ctypes.c_int(0)
    check(lib().dmxq_nm_mask_class(dtype_code(score.dtype), dtype_code(x.dtype) if want_y else 0, dtype_code(mask_dtype or score.dtype),
                                   dtype_code(y_dtype), outer, L, inner, int(K), int(M), base(score),
                                   (base(x) if x.shape == score.shape else fresh) if want_y else None, fresh if want_mask else None,
                                   fresh if want_y else None, ctypes.byref(route)), "dmxq_nm_mask_class")
    return NM_ROUTE_NAMES[route.value]


def _topk(score, x, density, want_mask, want_y, mask_dtype, y_dtype):
    require_gpu(score, "topk_mask")
    n_zero = int(score.numel() * (1.0 - density))  # sparse.py:116
    mask, y = _ops.topk_mask(score, x, n_zero, want_mask, want_y, mask_dtype, y_dtype)
    return (mask if want_mask else None), (y if want_y else None)


def topk_mask(score, density: float, mask_dtype: Optional[torch.dtype] = None):
    """Global top-k mask (sparse.py:109-123): the int(n * (1 - density)) lowest scores are zeroed; float mask in the
    score's dtype.  No sort: a radix select + one masking pass (csrc/topk.hip)."""
    return _topk(score, None, density, True, False, mask_dtype, None)[0]


def topk_sparsify(x, score, density: float, return_mask: bool = False):
    """x * topk_mask(score) in the same final pass (sparse.py:300), torch's type promotion for the product."""
    require_gpu(x, "topk_sparsify")
    mask, y = _topk(score, x, density, return_mask, True, None, None)
    return (y, mask) if return_mask else y


def bernoulli_mask(score, seed: Optional[int] = None, mask_dtype: Optional[torch.dtype] = None):
    """Bernoulli supermask (sparse.py:201-221): 1 with probability score."""
    require_gpu(score, "bernoulli_mask")
    return _ops.bernoulli_mask(score, _seed_arg(seed, "stochastic"), mask_dtype)


# ---------------------------------------------------------------------------------------------------- calibration
def group_minmax(x, ch_axis: int, group_size: int):
    """Per-group (slabs of `group_size` channels along ch_axis) min and max: two float32 [G] tensors."""
    require_gpu(x, "group_minmax")
    return _ops.group_minmax(x, ch_axis, group_size)


def group_minmax_accumulate(x, ch_axis: int, group_size: int, mn, mx):
    """running min / max of slabs of `group_size` channels updated IN PLACE by one launch: mn = min(mn, min(x)), mx = max(mx, max(x))
    (MinMaxObserver.forward as a whole, observer.py:173-193).  mn / mx: contiguous float32 GPU tensors of ceil(C / group_size) entries."""
    require_gpu(x, "group_minmax_accumulate")
    _ops.group_minmax_accumulate(x, ch_axis, group_size, mn, mx)


def qparams(mn, mx, qmin: int, qmax: int, symmetric_qscheme: bool):
    """(min,max) -> (scale fp32, zero_point int64), numerical/observer.py:59-115."""
    require_gpu(mn, "qparams")
    return _ops.qparams(mn, mx, qmin, qmax, symmetric_qscheme)


def histc(x, bins: int, lo: float = 0.0, hi: float = 0.0):
    """torch.histc(x, bins, min=lo, max=hi) as the HistogramObserver uses it (numerical/observer.py:470-472,
    489-491): float32 [bins] counts.  lo == hi selects the data's own range, widened by one either side when the
    data is constant (torch.histc's convention)."""
    require_gpu(x, "histc")
    lo, hi = float(lo), float(hi)
    if lo == hi and x.numel():
        mn, mx = group_minmax(x.reshape(1, -1), 0, 1)
        lo, hi = float(mn), float(mx)
        if lo == hi:
            lo, hi = lo - 1.0, hi + 1.0
    if x.numel() == 0 and not lo < hi:
        return torch.zeros(int(bins), dtype=torch.float32, device=x.device)
    if not (lo < hi and math.isfinite(lo) and math.isfinite(hi)):
        raise DmxqError(f"histc: needs a finite range with min < max, got [{lo}, {hi}]")
    return _ops.histc(x, int(bins), lo, hi)


def hist_observe(x, ch_axis: int, group_size: int, upsample_rate: int, hist, min_val, max_val, status, scratch):
    """One HistogramObserver observation of every group (slabs of `group_size` channels along ch_axis; per tensor: x.reshape(1, -1),
    0, 1) in four launches, no host synchronisation (dmxq_hist_observe).  The state is updated IN PLACE: hist float32 [G, bins],
    min_val / max_val float32 [G] (+inf / -inf before the first observation), status int32 [1] (0; 1 after an infinite extremum, 2
    after a NaN: the observation the host code refuses with OverflowError / ValueError).  scratch: >= (2 + bins) * G words of device
    memory (hist_scratch_words)."""
    require_gpu(x, "hist_observe")
    _ops.hist_observe(x, int(ch_axis), int(group_size), int(upsample_rate), hist, min_val, max_val, status, scratch)


def hist_scratch_words(n_groups: int, bins: int) -> int:
    return (2 + int(bins)) * int(n_groups)


def hist_qparams(hist, min_val, max_val, precision: int, qmin: int, qmax: int, symmetric_qscheme: bool):
    """HistogramObserver.calculate_qparams of every group in one launch (dmxq_hist_qparams): the L2 range search over the histogram,
    then (scale float32 [G], zero_point int64 [G]); a group that observed nothing gets (1, 0)."""
    require_gpu(hist, "hist_qparams")
    return _ops.hist_qparams(hist, min_val, max_val, int(precision), int(qmin), int(qmax), bool(symmetric_qscheme))


def channel_maxabs(x, ch_axis: int):
    """max|x| per channel along ch_axis (numerical/smoothquant.py:285-299): float32 [C]."""
    require_gpu(x, "channel_maxabs")
    return _ops.channel_maxabs(x, ch_axis)


def smoothquant_scale(a_maxabs, b_maxabs, alpha: float, scale_min: float = 1e-5):
    require_gpu(a_maxabs, "smoothquant_scale")
    return _ops.smoothquant_scale(a_maxabs, b_maxabs, float(alpha), float(scale_min))


def scale_channels(x, scale, ch_axis: int, divide: bool, out_dtype: Optional[torch.dtype] = None):
    require_gpu(x, "scale_channels")
    return _ops.scale_channels(x, scale, ch_axis, divide, out_dtype)


# ---------------------------------------------------------------------------------------------------- approximator slot
UNARY_GELU, UNARY_GELU_TANH, UNARY_SILU, UNARY_QUICK_GELU, UNARY_EXP, UNARY_SILU_EXPERIMENTAL = range(6)


def gelu(x, approximate: str = "none", out_dtype: Optional[torch.dtype] = None):
    require_gpu(x, "gelu")
    return _ops.unary(x, UNARY_GELU_TANH if approximate == "tanh" else UNARY_GELU, 0.0, out_dtype)


def silu(x, out_dtype: Optional[torch.dtype] = None):
    """torch.nn.functional.silu (modeling/nn/torch_modules.py:1559-1576), exact function."""
    require_gpu(x, "silu")
    return _ops.unary(x, UNARY_SILU, 0.0, out_dtype)


def quick_gelu(x, out_dtype: Optional[torch.dtype] = None):
    """transformers' QuickGELUActivation `x * sigmoid(1.702 * x)` in the input dtype (custom_modules.py:112-117)."""
    require_gpu(x, "quick_gelu")
    return _ops.unary(x, UNARY_QUICK_GELU, 0.0, out_dtype)


def exp(x, out_dtype: Optional[torch.dtype] = None):
    """torch.exp (modeling/nn/torch_modules.py:236-242 Exp)."""
    require_gpu(x, "exp")
    return _ops.unary(x, UNARY_EXP, 0.0, out_dtype)


def silu_experimental(x, scale: float):
    """the reference's `experimental.silu` (functional/functions.py:7-21): relu(x.to(float16)) * scale -> float16"""
    require_gpu(x, "silu_experimental")
    return _ops.unary(x, UNARY_SILU_EXPERIMENTAL, float(scale), torch.float16)


def rope(x, cos, sin, unsqueeze_dim: int = 1):
    """APPLY_LLAMA_ROPE for ONE of q / k: (x * cos) + (rotate_half(x) * sin) in the tensor dtype (custom_modules.py:142-172);
    x [B, n1, n2, D], cos / sin [B, S, D].  Returns None when the HIP kernel does not take this shape / dtype mix (the
    caller keeps torch's own ops)."""
    require_gpu(x, "rope")
    try:
        return _ops.rope(x, cos, sin, unsqueeze_dim)
    except NotImplementedError:
        return None


def relu_cast(x, cast_in=None, cast_out=None, then_bfp=None):
    """A ReLU DmxModule in one launch: cast_out(relu(cast_in(x))); casts are FloatingPoint formats (nearest, signed) or None = SAME;
    then_bfp as binary_cast (dmxq_relu_cast_bfp).  None when not fusable."""
    require_gpu(x, "relu_cast")
    for f in (cast_in, cast_out):
        if f is not None and (f.rounding != "nearest" or f.unsigned):
            return None
    try:
        return _ops.relu_cast(x, _fmt4(cast_in), _fmt4(cast_out), int(then_bfp[1]) if then_bfp else 0, int(then_bfp[0]) if then_bfp else 0)
    except NotImplementedError:
        return None


def rope_cast(x, cos, sin, unsqueeze_dim: int = 1, cast_x=None, cast_cos=None, cast_sin=None, cast_out=None):
    """One operand of an ApplyRotaryPosEmb module with its casts in one launch: cast_out(rope(cast_x(x), cast_cos(cos), cast_sin(sin)));
    casts are FloatingPoint formats (nearest, signed) or None = SAME.  None when not fusable."""
    require_gpu(x, "rope_cast")
    for f in (cast_x, cast_cos, cast_sin, cast_out):
        if f is not None and (f.rounding != "nearest" or f.unsigned):
            return None
    try:
        return _ops.rope_cast(x, cos, sin, unsqueeze_dim, _fmt4(cast_x), _fmt4(cast_cos), _fmt4(cast_sin), _fmt4(cast_out))
    except NotImplementedError:
        return None


def softmax(x, dim: int = -1, input_clamp: Optional[float] = None, out_dtype: Optional[torch.dtype] = None):
    require_gpu(x, "softmax")
    d = dim % x.dim()
    xt = x if d == x.dim() - 1 else x.transpose(d, -1)
    out = _ops.softmax(xt, float(input_clamp) if input_clamp is not None else -math.inf, out_dtype)
    return out if d == x.dim() - 1 else out.transpose(d, -1)


def _cols(normalized_shape):
    cols = 1
    for s in (normalized_shape if not isinstance(normalized_shape, int) else (normalized_shape,)):
        cols *= s
    return cols


def layernorm(x, normalized_shape, weight=None, bias=None, eps: float = 1e-5,
              out_dtype: Optional[torch.dtype] = None):
    require_gpu(x, "layernorm")
    return _ops.norm(x, _cols(normalized_shape), weight, bias, float(eps), 0, out_dtype)


def rmsnorm(x, normalized_shape, weight=None, eps: Optional[float] = None, out_dtype: Optional[torch.dtype] = None):
    """torch.nn.functional.rms_norm over the trailing `normalized_shape` (modeling/nn/torch_modules.py:1144-1170);
    eps None = torch.finfo(x.dtype).eps, as torch."""
    require_gpu(x, "rmsnorm")
    eps = torch.finfo(x.dtype).eps if eps is None else eps
    return _ops.norm(x, _cols(normalized_shape), weight, None, float(eps), 1, out_dtype)


# ---- an activation / normalisation DmxModule in one launch (include/dmxq.h dmxq_unary_cast ...): cast_out(f(cast_in(x)))
_UNARY_KIND = {"gelu": UNARY_GELU, "gelu_tanh": UNARY_GELU_TANH, "silu": UNARY_SILU, "quick_gelu": UNARY_QUICK_GELU, "exp": UNARY_EXP}


def _casts_ok(*fmts):
    return all(f is None or (f.rounding == "nearest" and not f.unsigned) for f in fmts)


def unary_cast(x, func: str, cast_in=None, cast_out=None):
    """A GELU / SiLU / QuickGELU / Exp DmxModule in one launch; func in {"gelu", "gelu_tanh", "silu", "quick_gelu", "exp"};
    casts are FloatingPoint formats (nearest, signed) or None = SAME.  None when not fusable (the caller runs the three steps)."""
    require_gpu(x, "unary_cast")
    if not _casts_ok(cast_in, cast_out):
        return None
    try:
        return _ops.unary_cast(x, _UNARY_KIND[func], 0.0, _fmt4(cast_in), _fmt4(cast_out))
    except NotImplementedError:
        return None


def unary_cast_table(like, func: str, cast_in=None, cast_out=None, param: float = 0.0):
    """The 65,536-entry table of a unary DmxModule on `like`'s 16-bit dtype and device: table[p] = cast_out(f(cast_in(x_p))) for input
    pattern p, f in float64 rounded once (dmxq_unary_cast_table).  func as unary_cast, plus "silu_experimental" (param = scale).
    Casts: FloatingPoint formats (nearest, signed; rounding casts allowed) or None.  None when a cast is not tabulable."""
    require_gpu(like, "unary_cast_table")
    if like.dtype not in (torch.bfloat16, torch.float16) or not _casts_ok(cast_in, cast_out):
        return None
    kind = 5 if func == "silu_experimental" else _UNARY_KIND[func]
    try:
        return _ops.unary_cast_table(like, kind, float(param), _fmt4(cast_in), _fmt4(cast_out))
    except NotImplementedError:
        return None


def lut16_apply(x, table):
    """out[i] = table[x[i] as a 16-bit pattern] (dmxq_lut16_apply): the application of unary_cast_table's result.  None when x is not
    a whole number of aligned 16-byte vectors."""
    require_gpu(x, "lut16_apply")
    try:
        return _ops.lut16_apply(x, table)
    except NotImplementedError:
        return None


def softmax_cast(x, dim: int = -1, cast_in=None, cast_out=None, input_clamp: Optional[float] = None, then_bfp=None):
    """A Softmax DmxModule in one launch (softmax over the LAST dim only).  then_bfp = (precision, block_size): the consumer's BFP input
    cast (symmetric, nearest, along the same dim) applied to the result in the same launch.  None when not fusable."""
    require_gpu(x, "softmax_cast")
    if x.dim() == 0 or dim % x.dim() != x.dim() - 1 or not _casts_ok(cast_in, cast_out):
        return None
    try:
        return _ops.softmax_cast(x, float(input_clamp) if input_clamp is not None else -math.inf, _fmt4(cast_in), _fmt4(cast_out),
                                 int(then_bfp[1]) if then_bfp else 0, int(then_bfp[0]) if then_bfp else 0)
    except NotImplementedError:
        return None


def layernorm_cast(x, normalized_shape, weight=None, bias=None, eps: float = 1e-5, cast_in=None, cast_out=None, then_bfp=None):
    """A LayerNorm DmxModule in one launch (weight / bias in x's dtype); then_bfp = (precision, block_size): the consumers' BFP input
    cast (symmetric, nearest, along the rows) applied in the same launch.  None when not fusable."""
    require_gpu(x, "layernorm_cast")
    if not _casts_ok(cast_in, cast_out):
        return None
    try:
        return _ops.norm_cast(x, _cols(normalized_shape), weight, bias, float(eps), 0, _fmt4(cast_in), _fmt4(cast_out),
                              int(then_bfp[1]) if then_bfp else 0, int(then_bfp[0]) if then_bfp else 0)
    except NotImplementedError:
        return None


def rmsnorm_cast(x, normalized_shape, weight=None, eps: Optional[float] = None, cast_in=None, cast_out=None, then_bfp=None):
    """An RMSNorm DmxModule in one launch (eps None = torch.finfo(x.dtype).eps, as torch); then_bfp as layernorm_cast.  None when not
    fusable."""
    require_gpu(x, "rmsnorm_cast")
    if not _casts_ok(cast_in, cast_out):
        return None
    eps = torch.finfo(x.dtype).eps if eps is None else eps
    try:
        return _ops.norm_cast(x, _cols(normalized_shape), weight, None, float(eps), 1, _fmt4(cast_in), _fmt4(cast_out),
                              int(then_bfp[1]) if then_bfp else 0, int(then_bfp[0]) if then_bfp else 0)
    except NotImplementedError:
        return None


# ---------------------------------------------------------------------------------------------------- GPTQ
def gptq_fields(fmt, per_row: bool = False):
    """The dmxq_gptq_format fields (include/dmxq.h) of a weight format the fused GPTQ column kernel covers, or None: BFP (MXINT) with
    nearest rounding and blocks of >= 2, FloatingPoint with nearest rounding and <= 22 mantissa bits, FixedPoint with nearest rounding
    (per_row: one affine scale / zero point per output row, else one for the tensor)."""
    from .format import BlockFloatingPoint, FixedPoint, FloatingPoint
    if getattr(fmt, "rounding", None) != "nearest":
        return None
    if isinstance(fmt, BlockFloatingPoint):
        if fmt.block_size < 2 or not 2 <= fmt.precision <= 22:
            return None
        return [0, fmt.precision, fmt.block_size, int(bool(fmt.symmetric)), 0, 0, 0, 0, 0, 0, 0, 0]
    if isinstance(fmt, FloatingPoint):
        if fmt.mantissa > 22:
            return None
        return [1, 0, 0, 0, fmt.mantissa, fmt.exponent, fmt.bias, int(bool(fmt.flush_subnormal)), int(bool(fmt.unsigned)), 0, 0, 0]
    if isinstance(fmt, FixedPoint):
        return [2, fmt.precision, 0, int(bool(fmt.symmetric)), 0, 0, 0, 0, 0, fmt.fraction, int(bool(fmt.clamp)), int(bool(per_row))]
    return None


def gptq_block(w, hinv, inv_d, q, err, microblock: int, fields, scale=None, zero_point=None):
    """GPTQ's in-block column loop for one block of <= 128 columns in one launch (dmxq_gptq_block; layer_reconstruction.py:300-318):
    w = W[:, i1:i2] (read only), hinv = Hinv[i1:i2, i1:i2], inv_d = the inverses of its diagonal microblocks [ceil(count / mb), mb, mb];
    writes Q[:, i1:i2] into `q` and the error block into `err` (float32 views with unit column stride).  `fields`: gptq_fields(...).
    NotImplementedError where the kernel does not take the format / microblock (the caller runs its own loop)."""
    require_gpu(w, "gptq_block")
    _ops.gptq_block(w, hinv, inv_d, int(microblock), [int(v) for v in fields], scale, zero_point, q, err)


def gptq_block_dynamic(w, hinv, inv_d, q, err, scale_out, zp_out, microblock: int, group: int, fmt, symmetric_qscheme: bool = False):
    """gptq_block for an integer format with DYNAMIC per-group scales (dmxq_gptq_block_dynamic): at every column j of the
    block with j % group == 0 each row takes (scale, zero point) = qparams(group_minmax(w[:, j:j + group])) of its values as the loop
    has updated them, casts the group's columns with it as gptq_block casts with a per-row scale, and records it in
    scale_out / zp_out (float32 / int64 [rows, count // group] views with unit column stride).  fmt: a clamped XP[p,0] format (or its
    shorthand); symmetric_qscheme as ops.qparams takes it.  ValueError for a format without an integer range; NotImplementedError
    where the kernel does not take the group (16, 32, 64, 128; it divides count and is a multiple of the microblock), the microblock
    or the format (the caller runs its own loop; nothing was launched)."""
    from .observer import get_qmin_qmax
    fmt, _, group = dynamic_check(fmt, "per_group", group, what="gptq_block_dynamic")
    require_gpu(w, "gptq_block_dynamic")
    qmin, qmax = get_qmin_qmax(fmt)
    fields = [2, fmt.precision, 0, int(bool(fmt.symmetric)), 0, 0, 0, 0, 0, fmt.fraction, int(bool(fmt.clamp)), 1]
    _ops.gptq_block_dynamic(w, hinv, inv_d, int(microblock), fields, ROUNDING_CODE[fmt.rounding], int(group), qmin, qmax,
                            bool(symmetric_qscheme), q, err, scale_out, zp_out)


# ---------------------------------------------------------------------------------------------------- error statistics
ERR_MAX_FORMATS = 8   # formats per dmxq_cast_error call


def error_scratch_bytes(n: int, n_formats: int = 1) -> int:
    """dmxq_error_scratch_bytes: the scratch one dmxq_error_stats (n_formats = 1) or dmxq_cast_error call over n elements needs.  A host
    query of the library itself, the same for both bindings."""
    from ._lib import lib
    return int(lib().dmxq_error_scratch_bytes(int(n), int(n_formats)))


def _err_scratch(x, n_formats):
    return torch.empty(max(error_scratch_bytes(x.numel(), n_formats), 8), dtype=torch.uint8, device=x.device)


def _err_out(like, rows, out, accumulate, what):
    if out is None:
        if accumulate:
            raise ValueError(f"{what}: accumulate=True merges into an existing row: pass it as out=")
        return torch.empty((rows, 4) if rows is not None else (4,), dtype=torch.float64, device=like.device)
    want = 4 * (rows if rows is not None else 1)
    if not (out.is_cuda and out.device == like.device and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == want):
        raise ValueError(f"{what}: out must be a contiguous float64 tensor of {want} entries on the input's device")
    return out


def error_stats(ref, test, out=None, accumulate: bool = False):
    """[sum_sq_err, sum_sq_ref, max_abs_err, count] between a reference and a test tensor of one shape (float32 / float16 / bfloat16 in any
    combination) as a float64 [4] row ON THE DEVICE: one read of each tensor, no host synchronisation (dmxq_error_stats).
    sum_sq_err = sum (float(ref) - float(test))^2 and sum_sq_ref = sum float(ref)^2 in fp64; max_abs_err is torch's
    (ref - test).float().abs().max(); mse = row[0] / row[3], SQNR in dB = 10 log10(row[1] / row[0]).  accumulate=True merges into `out`
    (sums add, max takes the max, count adds): statistics over many batches.  A non-dense view is copied to a contiguous tensor first."""
    require_gpu(ref, "error_stats")
    require_gpu(test, "error_stats")
    if ref.shape != test.shape:
        raise ValueError(f"error_stats: shapes differ: {tuple(ref.shape)} and {tuple(test.shape)}")
    out = _err_out(ref, None, out, accumulate, "error_stats")
    _ops.error_stats(ref.detach(), test.detach(), bool(accumulate), out, _err_scratch(ref, 1))
    return out


def _cast_error_entry(entry):
    """a `formats` entry of cast_error -> (Format, scale, zero_point); FixedPoint: (format, scale, zero_point), numbers or 1-element tensors"""
    from .format import FixedPoint, Format
    fmt, scale, zp = entry if isinstance(entry, (tuple, list)) else (entry, None, None)
    fmt = Format.from_shorthand(fmt)
    if not isinstance(fmt, Format):
        raise TypeError(f"cast_error: {fmt!r} is not a numerical format")
    parts = [fmt] + [getattr(fmt, a) for a in ("block_format", "scaler_format", "element_format") if hasattr(fmt, a)]
    if any(getattr(p, "rounding", None) == "stochastic" for p in parts):
        raise NotImplementedError(f"cast_error: {fmt!r} rounds stochastically: its error is not a property of the format alone")
    if scale is not None:
        if not isinstance(fmt, FixedPoint):
            raise ValueError(f"cast_error: only a FixedPoint entry takes a (format, scale, zero_point) triple, got {fmt!r}")
        if any(isinstance(t, torch.Tensor) and t.numel() != 1 for t in (scale, zp)):
            raise ValueError("cast_error: a FixedPoint entry takes ONE scale and zero point (per-channel / per-group: CastTo.measure_error)")
    return fmt, scale, zp


cast_error_entry = _cast_error_entry   # (benchmark.format_sweep parses its entries the same way)


def _affine_tensor(v, dtype, like, default):
    if isinstance(v, torch.Tensor):
        return v.detach().to(device=like.device, dtype=dtype).reshape(1)
    return torch.full((1,), default if v is None else v, dtype=dtype, device=like.device)   # (a fill launch: no host copy, capturable)


def _cast_like_library(x, fmt, scale, zp, block_dim):
    """the library's own cast of x to fmt, in x's dtype (what CastTo.forward returns)"""
    from .format import FixedPoint
    if isinstance(fmt, FixedPoint) and scale is not None:
        return fixed_qdq(x, fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding,
                         scale=_affine_tensor(scale, torch.float32, x, 1.0), zero_point=_affine_tensor(zp, torch.int64, x, 0), out_dtype=x.dtype)
    return fmt.cast(x, block_dim, out_dtype=x.dtype)


def cast_error(x, formats, block_dim: int = -1, out=None, accumulate: bool = False):
    """The error_stats row between x and its cast to each of K formats -- float64 [K, 4] on the device -- WITHOUT materialising the casts
    where the fused kernel covers them: x is read once per group of up to 8 formats and every cast is evaluated in registers
    (dmxq_cast_error).  formats: Format objects or shorthands; a FixedPoint entry may be a (format, scale, zero_point)
    triple (numbers or 1-element tensors: the affine wrapper of CastTo), else it is the bare fixed point cast.
    Row k equals error_stats(x, CastTo(formats[k], block_dim=block_dim)(x)): count and max_abs_err bit for bit, the two sums up to the
    order of an fp64 sum.  Fused: BFP / MXINT (nearest, blocks of 8 .. 128 along the last dim, dividing it), FloatingPoint (nearest) and
    FixedPoint (nearest) on a tensor whose last dim is a multiple of 8.  Everything else -- a block dim other than the last, MXFP, SBFP,
    ragged blocks, up / down rounding -- runs as the library's own cast followed by error_stats, under the same contract.  Stochastic
    rounding is refused (NotImplementedError)."""
    from .format import BlockFloatingPoint, FixedPoint, FloatingPoint
    require_gpu(x, "cast_error")
    entries = [_cast_error_entry(e) for e in formats]
    K = len(entries)
    if K == 0:
        raise ValueError("cast_error: no formats")
    out = _err_out(x, K, out, accumulate, "cast_error").view(K, 4)
    xd = x.detach()
    xd = xd if xd.is_contiguous() else xd.contiguous()
    last = xd.dim() >= 1 and -xd.dim() <= block_dim < xd.dim() and block_dim % xd.dim() == xd.dim() - 1
    fields = []
    for fmt, scale, zp in entries:
        f = gptq_fields(fmt) if xd.dim() >= 1 else None
        if f is not None and isinstance(fmt, BlockFloatingPoint) and not last:
            f = None
        if f is not None and isinstance(fmt, FloatingPoint) and fmt.native_of() == xd.dtype:
            f = None   # (Format.cast hands such a tensor through untouched)
        fields.append(f)
    fused = [i for i in range(K) if fields[i] is not None]
    rest = [i for i in range(K) if fields[i] is None]
    for c0 in range(0, len(fused), ERR_MAX_FORMATS):
        idx = fused[c0:c0 + ERR_MAX_FORMATS]
        dense = idx == list(range(idx[0], idx[0] + len(idx)))
        rows = out[idx[0]:idx[0] + len(idx)] if dense else (torch.stack([out[i] for i in idx]) if accumulate else
                                                            torch.empty((len(idx), 4), dtype=torch.float64, device=xd.device))
        scale = zp = None
        if any(isinstance(entries[i][0], FixedPoint) for i in idx):
            scale = torch.cat([_affine_tensor(entries[i][1], torch.float32, xd, 1.0) for i in idx])
            zp = torch.cat([_affine_tensor(entries[i][2], torch.int64, xd, 0) for i in idx])
        try:
            _ops.cast_error(xd, [int(v) for i in idx for v in fields[i]], scale, zp, bool(accumulate), rows, _err_scratch(xd, len(idx)))
        except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched: a last dim that is no multiple of 8 or of a block size, ...)
            rest += idx
            continue
        if not dense:
            for j, i in enumerate(idx):
                out[i].copy_(rows[j])
    for i in sorted(rest):
        fmt, scale, zp = entries[i]
        with torch.no_grad():
            y = _cast_like_library(xd, fmt, scale, zp, block_dim)
        error_stats(xd, y, out=out[i], accumulate=accumulate)
    return out


# ---------------------------------------------------------------------------------------------------- Hadamard rotation
HADAMARD_SIZES = (8, 16, 32, 64, 128, 256)   # block widths of dmxq_hadamard_qdq


def hadamard_check_size(size, what: str = "hadamard") -> int:
    """the rotation width, or ValueError: a power of two from 8 to 256"""
    if isinstance(size, bool) or not isinstance(size, int) or size not in HADAMARD_SIZES:
        raise ValueError(f"{what}: the rotation size must be one of {HADAMARD_SIZES}, got {size!r}")
    return size


def _rot_dim(x, size, dim, what):
    if x.dim() < 1 or not -x.dim() <= dim < x.dim():
        raise ValueError(f"{what}: dimension {dim} of a tensor of shape {tuple(x.shape)}")
    d = dim % x.dim()
    if x.shape[d] % size:
        raise ValueError(f"{what}: dimension {dim} has {x.shape[d]} elements, not a multiple of the rotation size {size}")
    return d


def _to_last(x, d):
    """the rotated dimension as the contiguous last one (d not last: a transposing copy -- the SLOW path)"""
    return x if d == x.dim() - 1 else x.movedim(d, -1).contiguous()


def _from_last(y, d):
    return y if d == y.dim() - 1 else y.movedim(-1, d).contiguous()


def _rotate(x, size, d, out_dtype):
    return _from_last(_ops.hadamard_qdq(_to_last(x.detach(), d), size, False, [], None, None, out_dtype), d)


class _Rotation(torch.autograd.Function):
    """R is symmetric and orthonormal: the gradient of R(x) is R(grad)"""

    @staticmethod
    def forward(ctx, x, size, d, out_dtype):
        ctx.set_materialize_grads(False)
        ctx.rot = (size, d, x.dtype)
        return _rotate(x, size, d, out_dtype)

    @staticmethod
    def backward(ctx, g):
        size, d, dt = ctx.rot
        return (None if g is None else _rotate(g, size, d, dt)), None, None, None


class _RotatedCast(torch.autograd.Function):
    """rotate -> cast (-> rotate back): the cast is a straight-through estimator, so the backward is the identity with the inverse
    rotation and R(grad) without it"""

    @staticmethod
    def forward(ctx, x, run, size, d, inverse):
        ctx.set_materialize_grads(False)
        ctx.rot = (size, d, x.dtype, inverse)
        return run(x.detach())

    @staticmethod
    def backward(ctx, g):
        size, d, dt, inverse = ctx.rot
        if g is not None:
            g = (g if g.dtype == dt else g.to(dt)) if inverse else _rotate(g, size, d, dt)
        return g, None, None, None, None


def hadamard(x, size: int, dim: int = -1, out_dtype: Optional[torch.dtype] = None):
    """The orthonormal block-Hadamard rotation of blocks of `size` consecutive elements along `dim`, one launch (dmxq_hadamard_qdq without
    a format): log2(size) butterfly stages of fp32 adds / subtracts, strides 1, 2, .., size / 2, then one multiply by
    float32(1 / sqrt(size)); rounded once to out_dtype (default x.dtype).  Its own inverse.  size in HADAMARD_SIZES, dividing the
    dimension (ValueError otherwise).  A `dim` other than the last is transposed to the last with a contiguous copy, rotated and
    transposed back: a slow path.  Differentiable: the gradient is hadamard(grad)."""
    hadamard_check_size(size, "hadamard")
    require_gpu(x, "hadamard")
    d = _rot_dim(x, size, dim, "hadamard")
    out_dtype = out_dtype or x.dtype
    if x.requires_grad and torch.is_grad_enabled():
        return _Rotation.apply(x, size, d, out_dtype)
    return _rotate(x, size, d, out_dtype)


# dmxq_gptq_format kinds that fused=None sends to the three-launch chain although the kernel takes them.  The rule: the fused call moves
# 4 B per bf16 element and the chain 20 B, so a format is routed to the kernel only when its fused call has been MEASURED under 5 x its
# plain cast on [4096, 4096] and [14336, 4096] (tools/bench_hadamard.py).  profiles/r11_hadamard.txt: BFP[8|8]{16}, MXFP4[E2M1]{32} and
# per-tensor XP[8,0] at H = 32 / 64 / 128 all between 1.98 x and 2.70 x -- every kind goes to the kernel (FloatingPoint, not in that
# table, is the cheapest cast body of the four in the same kernel).
HADAMARD_CHAIN_BY_DEFAULT = frozenset()


def _hadamard_fields(fmt, per_row):
    """the dmxq_gptq_format fields of a format the fused rotation kernel casts to (gptq_fields plus MXFP, kind 3), or None"""
    from .format import MXFP, FloatingPoint
    if isinstance(fmt, MXFP):
        ef = fmt.element_format   # (MXFP.cast reads the element format's mantissa and exponent widths only)
        if ef.mantissa > 22:
            return None
        return [3, 0, int(fmt.block_size), 0, int(ef.mantissa), int(ef.exponent), 0, 0, 0, 0, 0, 0]
    f = gptq_fields(fmt, per_row)
    if f is not None and isinstance(fmt, FloatingPoint) and fmt.native_of() == torch.float32:
        return None   # (Format.cast hands a float32 tensor through untouched)
    return f


def hadamard_qdq(x, size: int, fmt, block_dim: int = -1, inverse: bool = True, scale=None, zero_point=None, per_row: bool = False,
                 out_dtype: Optional[torch.dtype] = None, fused: Optional[bool] = None, ch_axis: Optional[int] = None,
                 group_size: Optional[int] = None):
    """Rotate, quantize, and rotate back (inverse=True) or stay in the rotated basis (inverse=False):
        y = round_to(out_dtype, R(Q(R(x))))   or   round_to(out_dtype, Q(R(x)))
    with R = hadamard(., size) along block_dim in float32 and Q the library's own cast of the rotated float32 tensor to `fmt` (a Format
    or shorthand), blocks along the same dimension, float32 out; ONE rounding to out_dtype (default x.dtype) at the end.
    ONE launch (dmxq_hadamard_qdq) for BFP / MXINT (nearest, a power-of-two block dividing size), MXFP (a power-of-two block dividing size),
    FloatingPoint (nearest) and FixedPoint (nearest; scale / zero_point: one for the tensor -- numbers or 1-element tensors, default
    scale 1 and zero point 0 through the same affine form on the kernel and on the chain, as ops.cast_error treats a bare FixedPoint
    entry -- or with per_row one per row of the [rows, L] view, the rotated dimension being the last).
    fused=None: the kernel where it applies (every fused format measured 2.0-2.7 x its plain cast, under the 5 x at which the chain
    would be the better default: profiles/r11_hadamard.txt; HADAMARD_CHAIN_BY_DEFAULT would list the exceptions), else the chain hadamard (float32) -> the library's cast (float32) -> hadamard: the same
    bits by construction, three launches.  The chain takes everything Format.cast takes -- SBFP, up / down / stochastic rounding (the usual
    seed rules), blocks that do not divide size, and per-channel / per-group affine scales (ch_axis, group_size as ops.fixed_qdq; on the
    chain only).  fused=True raises NotImplementedError instead of falling back; fused=False forces the chain.
    A block_dim other than the last is transposed to the last with a contiguous copy and back: a slow path.
    Autograd: the cast is a straight-through estimator -- the backward is the identity with inverse, hadamard(grad) without."""
    from .format import FixedPoint, Format, Same
    hadamard_check_size(size, "hadamard_qdq")
    require_gpu(x, "hadamard_qdq")
    fmt = Format.from_shorthand(fmt)
    if not isinstance(fmt, Format):
        raise TypeError(f"hadamard_qdq: {fmt!r} is not a numerical format")
    d = _rot_dim(x, size, block_dim, "hadamard_qdq")
    out_dtype = out_dtype or x.dtype
    fixed = isinstance(fmt, FixedPoint)
    if (scale is not None or zero_point is not None or per_row or ch_axis is not None or group_size) and not fixed:
        raise ValueError(f"hadamard_qdq: only a FixedPoint format takes an affine scale / zero point, got {fmt!r}")
    if per_row and (ch_axis is not None or group_size):
        raise ValueError("hadamard_qdq: per_row or ch_axis / group_size, not both")
    if per_row and d != x.dim() - 1:
        raise ValueError("hadamard_qdq: per_row scales go with a rotation along the last dimension")
    if (per_row or ch_axis is not None) and (scale is None or zero_point is None):
        raise ValueError("hadamard_qdq: per-row / per-channel / per-group casts need their scale and zero_point tensors")
    on_chain_only = ch_axis is not None or bool(group_size) or isinstance(fmt, Same)

    def affine(xl):
        if per_row or ch_axis is not None:
            return (scale.detach().to(device=xl.device, dtype=torch.float32).reshape(-1).contiguous(),
                    zero_point.detach().to(device=xl.device, dtype=torch.int64).reshape(-1).contiguous())
        return _affine_tensor(scale, torch.float32, xl, 1.0), _affine_tensor(zero_point, torch.int64, xl, 0)

    def cast(r, dt):   # the library's cast of the rotated float32 tensor r (rotated dimension last)
        if not fixed:
            y = fmt.cast(r, -1, out_dtype=dt)
            return y if y.dtype == dt else y.to(dt)   # (SAME and FLOAT32 hand a float32 tensor through)
        sc, zp = affine(r)
        if per_row:
            y = fixed_qdq(r.reshape(-1, r.shape[-1]), fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=sc,
                          zero_point=zp, ch_axis=0, out_dtype=dt)
            return y.reshape(r.shape)
        ax = None
        if ch_axis is not None:   # the channel axis after the rotated dimension moved to the end
            a = ch_axis % x.dim()
            ax = a if d == x.dim() - 1 or a < d else (x.dim() - 1 if a == d else a - 1)
        return fixed_qdq(r, fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=sc, zero_point=zp, ch_axis=ax,
                         group_size=group_size, out_dtype=dt)

    def run(xd):
        xl = _to_last(xd, d)
        if fused is not False:
            fields = None if on_chain_only else _hadamard_fields(fmt, per_row)
            if fields is None and fused:
                raise NotImplementedError(f"hadamard_qdq: no fused kernel for {fmt!r}"
                                          + (" with per-channel / per-group scales" if on_chain_only else ""))
            if fields is not None and fused is None and fields[0] in HADAMARD_CHAIN_BY_DEFAULT:
                fields = None
            if fields is not None:
                sc, zp = affine(xl) if fixed else (None, None)
                if per_row and (sc.numel() != xl.numel() // max(xl.shape[-1], 1) or zp.numel() != sc.numel()):
                    raise ValueError("hadamard_qdq: per_row needs one scale and one zero point per row")
                try:
                    return _from_last(_ops.hadamard_qdq(xl, size, bool(inverse), fields, sc, zp, out_dtype), d)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched: a block that does not divide size, ...)
                    if fused:
                        raise
        r = _ops.hadamard_qdq(xl, size, False, [], None, None, torch.float32)
        if inverse:
            y = _ops.hadamard_qdq(cast(r, torch.float32), size, False, [], None, None, out_dtype)
        else:
            y = cast(r, out_dtype)
        return _from_last(y, d)

    if x.requires_grad and torch.is_grad_enabled():
        return _RotatedCast.apply(x, run, size, d, bool(inverse))
    with torch.no_grad():
        return run(x.detach())


# ---------------------------------------------------------------------------------------------------- dynamic integer cast
DYNAMIC_GRANULARITIES = ("per_token", "per_group", "per_tensor")
DYNAMIC_MAX_ROW = 16384          # the longest segment dmxq_dynamic_fixed_qdq keeps in registers
DYNAMIC_CHAIN_MAX_SEGMENTS = 65535   # groups of one dmxq_group_minmax call; more segments: the chain runs on pieces of ...
DYNAMIC_CHAIN_PIECE = 32768          # ... this many segments (the kernel has no such limit)
# Launch geometries of dmxq_dynamic_fixed_qdq (dynamic_class) that fused=None sends to the three-launch chain although the kernel takes
# them.  The rule: a class goes to the kernel by default only where tools/bench_dynamic_quant.py MEASURED it faster than the chain on the
# same buffers; a class that is not gets listed here with its row.  profiles/r12_dynamic_quant.txt (bf16 INT8, symmetric / affine, us per
# call, kernel against chain): wave_row [8192,4096] 27.7 / 28.0 against 75.1 / 74.4, [2048,768] 3.7 / 3.8 against 20.4 / 20.3; block_row
# [8192,14336] 85.9 / 84.4 against 143.1 / 143.2; group (128) [8192,4096] 28.3 / 31.2 against 1368 / 1370, [8192,14336] 77.3 / 83.6 against
# 4757 / 4755, [2048,768] 3.3 / 3.5 against 67.4; short_row [60000,48] 36.3 / 38.5 against 287.3 / 287.6 (4 % of 8 TB/s: most lanes idle,
# still 7.5-7.9 x the chain) -- every class is faster, none is listed.
DYNAMIC_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_dynamic_routes = {"fused": 0, "chain": 0}
_DYNAMIC_CLASS_NAMES = {1: "group", 2: "short_row", 3: "wave_row", 4: "block_row"}   # dmxq_dynamic_geometry (include/dmxq.h)


def dynamic_check(fmt, granularity, group_size=None, what: str = "dynamic_fixed_qdq"):
    """-> (format, granularity, group_size) of a dynamic cast, or ValueError: a format with an integer range (observer.get_qmin_qmax), a
    known granularity, a positive group size with per_group and none otherwise.  No GPU involved."""
    from .format import Format
    from .observer import get_qmin_qmax
    fmt = Format.from_shorthand(fmt) if isinstance(fmt, str) else fmt
    if not isinstance(fmt, Format) or get_qmin_qmax(fmt) == (None, None):
        raise ValueError(f"{what}: a dynamic cast derives integer scales, so it needs a clamped FixedPoint format without fraction bits "
                         f"(XP[p,0](C..)), got {fmt!r}")
    if granularity not in DYNAMIC_GRANULARITIES:
        raise ValueError(f"{what}: granularity must be one of {DYNAMIC_GRANULARITIES}, got {granularity!r}")
    if granularity == "per_group":
        if isinstance(group_size, bool) or not isinstance(group_size, int) or group_size < 1:
            raise ValueError(f"{what}: per_group needs a positive integer group_size, got {group_size!r}")
    elif group_size is not None:
        raise ValueError(f"{what}: group_size goes with granularity 'per_group', got {granularity!r} with group_size {group_size!r}")
    return fmt, granularity, group_size


def dynamic_class(segment: int, dtype: torch.dtype, whole_rows: bool) -> Optional[str]:
    """the launch geometry dmxq_dynamic_fixed_qdq picks for segments of `segment` elements of `dtype`, asked of the library itself
    (dmxq_dynamic_class: the function that makes the choice inside the entry; no GPU involved), or None when it refuses them: "group"
    (power-of-two segments of 16 .. 256 inside a wave), "short_row" (a wave per row of fewer than 64 vectors: lanes idle), "wave_row"
    (a wave per row, up to 16 vectors per lane), "block_row" (a workgroup per row, up to 16384 elements)"""
    from ._lib import dtype_code, lib
    return _DYNAMIC_CLASS_NAMES.get(lib().dmxq_dynamic_class(dtype_code(dtype), int(segment), int(bool(whole_rows))))


class _DynamicSTE(torch.autograd.Function):
    """the dynamic cast as a straight-through estimator (cast.py _FixedAffineCast: the scales are not differentiated either)"""

    @staticmethod
    def forward(ctx, x, run):
        ctx.set_materialize_grads(False)
        ctx.in_dtype = x.dtype
        out = run(x.detach())
        if isinstance(out, tuple):
            ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, g, *_):
        if g is not None and g.dtype != ctx.in_dtype:
            g = g.to(ctx.in_dtype)
        return g, None


def dynamic_fixed_qdq(x, fmt, granularity: str = "per_token", group_size: Optional[int] = None, symmetric_qscheme: bool = False,
                      out_dtype: Optional[torch.dtype] = None, return_qparams: bool = False, fused: Optional[bool] = None, seed: Optional[int] = None):
    """Integer Q->DQ with scales derived from the tensor itself on every call (not in the reference, whose integer casts
    need a calibration pass).  A segment is S consecutive elements along the last dim of the contiguous tensor: the whole row with
    "per_token" (per output channel of an [out, in] weight), `group_size` elements with "per_group" (it must divide the last dim), the
    whole tensor with "per_tensor".  By definition, with (qmin, qmax) = observer.get_qmin_qmax(fmt):
        x2 = x.reshape(-1, S);  mn, mx = group_minmax(x2, 0, 1);  sc, zp = qparams(mn, mx, qmin, qmax, symmetric_qscheme)
        y = fixed_qdq(x2, fmt..., scale=sc, zero_point=zp, ch_axis=0, out_dtype=out_dtype).reshape(x.shape)
    -- the reference's own formulas (numerical/observer.py:59-115, numerical/cast.py:278-296) per call; symmetric_qscheme as
    MinMaxObserver.calculate_qparams decides it (True for torch.per_tensor_symmetric / per_channel_symmetric).  A row with a NaN gets
    scale eps (qparams drops the NaN extrema); a row with an Inf gets scale Inf.  Nothing is read back to the host.
    ONE launch (dmxq_dynamic_fixed_qdq: 4 B per bf16 element instead of 6, one launch instead of three) for a nearest-rounding format,
    out_dtype == x.dtype, a 16-byte aligned tensor and S a power of two from 16 to 256 or -- per_token / per_tensor -- any multiple of a
    16-byte vector up to 16384; the chain otherwise, same bits (on more than 65535 segments, what one group_minmax call takes, the chain
    runs on pieces of 32768 segments and joins the results).  fused=None: the kernel where it applies and its geometry
    (dynamic_class) is not listed in DYNAMIC_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.
    seed: for a stochastic-rounding format (the chain only), as ops.fixed_qdq takes it; the draws are keyed by the element's index within
    its piece of the chain.
    return_qparams: (y, scale float32 [n_segments], zero_point int64 [n_segments]) on both routes.
    ValueError (before any GPU use): a format without an integer range, an unknown granularity, a group_size that does not divide the
    last dim.  Autograd: a straight-through estimator."""
    from .observer import get_qmin_qmax
    fmt, granularity, group_size = dynamic_check(fmt, granularity, group_size)
    if x.dim() < 1:
        raise ValueError("dynamic_fixed_qdq: expects a tensor with at least one dimension")
    L = x.shape[-1]
    if granularity == "per_group" and L % group_size:
        raise ValueError(f"dynamic_fixed_qdq: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    require_gpu(x, "dynamic_fixed_qdq")
    qmin, qmax = get_qmin_qmax(fmt)
    sym = bool(symmetric_qscheme)
    out_dtype = out_dtype or x.dtype
    S = {"per_token": L, "per_group": group_size, "per_tensor": x.numel()}[granularity]
    whole_rows = granularity != "per_group"

    def run(xd):
        xc = xd if xd.is_contiguous() else xd.contiguous()
        if xc.numel() == 0:
            y = torch.empty(xc.shape, dtype=out_dtype, device=xc.device)
            return (y, y.new_empty(0, dtype=torch.float32), y.new_empty(0, dtype=torch.int64)) if return_qparams else y
        if fused is not False:
            cls = dynamic_class(S, xc.dtype, whole_rows) if (fmt.rounding == "nearest" and out_dtype == xc.dtype and fmt.precision <= 22
                                                             and xc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"dynamic_fixed_qdq: no fused kernel for segments of {S} {xc.dtype} elements -> {out_dtype} "
                                          f"with {fmt!r} (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in DYNAMIC_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    y, sc, zp = _ops.dynamic_fixed_qdq(xc, S, whole_rows, fmt.precision, fmt.fraction, bool(fmt.clamp), bool(fmt.symmetric),
                                                       ROUNDING_CODE[fmt.rounding], qmin, qmax, sym, bool(return_qparams), out_dtype)
                    _dynamic_routes["fused"] += 1
                    return (y, sc, zp) if return_qparams else y
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _dynamic_routes["chain"] += 1
        x2 = xc.reshape(-1, S)

        def three(part):
            mn, mx = _ops.group_minmax(part, 0, 1)
            sc, zp = _ops.qparams(mn, mx, qmin, qmax, sym)
            return fixed_qdq(part, fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=sc, zero_point=zp, ch_axis=0,
                             out_dtype=out_dtype, seed=seed), sc, zp

        if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
            y, sc, zp = three(x2)
        else:   # (dmxq_group_minmax takes 65535 groups: segments are independent, so the chain runs on pieces and the results are joined)
            parts = [three(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)]
            y, sc, zp = (torch.cat([p[k] for p in parts]) for k in range(3))
        y = y.reshape(xc.shape)
        return (y, sc, zp) if return_qparams else y

    if x.requires_grad and torch.is_grad_enabled():
        return _DynamicSTE.apply(x, run)
    with torch.no_grad():
        return run(x.detach())


# ---------------------------------------------------------------------------------------------------- learned step size (LSQ / LSQ+)
# Launch geometries of dmxq_lsq_backward (lsq_class) that fused=None sends to the chain of torch operations although the kernel takes
# them: DYNAMIC_CHAIN_BY_DEFAULT's rule -- a class goes to the kernel by default only where tools/bench_lsq.py MEASURED it faster than the
# chain on the same buffers; a class that is not gets listed here with its row.  profiles/r19_lsq.txt (bf16 XP[4,0] affine, us per call,
# kernel against chain): group (128) [8192,4096] 50.2 against 1676.9, [8192,14336] 147.9 against 5703.5, [2048,768] 6.0 against 160.4;
# wave_row [8192,4096] 50.3 against 1648.0, [2048,768] 6.8 against 158.7; block_row [8192,14336] 135.6 against 5665.7; tensor [8192,4096]
# 57.9 against 1663.5, [8192,14336] 148.3 against 5669.8, [2048,768] 8.4 against 163.5, [60000,48] 11.4 against 215.1; short_row [60000,48]
# 39.6 against 218.1 (5 % of 8 TB/s: most lanes idle, still 5.5 x the chain) -- every class is faster, none is listed.
LSQ_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_lsq_routes = {"fused": 0, "chain": 0}
_LSQ_CLASS_NAMES = dict(_DYNAMIC_CLASS_NAMES)
_LSQ_CLASS_NAMES[6] = "tensor"   # DMXQ_LSQ_TENSOR (include/dmxq.h)
_LSQ_MODE = {"per_group": 0, "per_token": 1, "per_tensor": 2}   # dmxq_lsq_backward's whole_rows


def lsq_class(segment: int, dtype: torch.dtype, granularity: str) -> Optional[str]:
    """the launch geometry dmxq_lsq_backward picks for segments of `segment` elements of `dtype` under `granularity`, asked of the library
    itself (dmxq_lsq_class; no GPU involved), or None when it refuses them: dynamic_class's names for per_group / per_token, "tensor"
    (one segment over the grid, partial rows folded by a second launch) for per_tensor"""
    from ._lib import dtype_code, lib
    if granularity not in _LSQ_MODE:
        raise ValueError(f"lsq_class: granularity must be one of {DYNAMIC_GRANULARITIES}, got {granularity!r}")
    return _LSQ_CLASS_NAMES.get(lib().dmxq_lsq_class(dtype_code(dtype), int(segment), _LSQ_MODE[granularity]))


def lsq_scratch_bytes(n: int) -> int:
    """dmxq_lsq_scratch_bytes: the scratch a per_tensor dmxq_lsq_backward over n elements needs (16 bytes per workgroup).  A host
    function: no GPU involved."""
    from ._lib import lib
    return int(lib().dmxq_lsq_scratch_bytes(int(n)))


def lsq_grad_factor(grad_scale, segment: int, qmax: int) -> float:
    """grad_scale's three spellings -> the factor k of the definition: "lsq" 1 / sqrt(segment * qmax) (Esser et al., 2020), None 1, a
    float as given"""
    if grad_scale is None:
        return 1.0
    if isinstance(grad_scale, str):
        if grad_scale != "lsq":
            raise ValueError(f"lsq: grad_scale must be 'lsq', None or a float, got {grad_scale!r}")
        return 1.0 / math.sqrt(float(segment) * float(qmax)) if segment > 0 else 1.0
    if isinstance(grad_scale, bool) or not isinstance(grad_scale, (int, float)):
        raise ValueError(f"lsq: grad_scale must be 'lsq', None or a float, got {grad_scale!r}")
    return float(grad_scale)


def _lsq_segment(x, fmt, granularity, group_size, what):
    """-> (format, S): dynamic_check plus the shape rules, ValueError before any GPU use"""
    fmt, granularity, group_size = dynamic_check(fmt, granularity, group_size, what=what)
    if fmt.rounding != "nearest":
        raise ValueError(f"{what}: a learned step size is defined for nearest rounding, got {fmt!r}")
    if x.dim() < 1:
        raise ValueError(f"{what}: expects a tensor with at least one dimension")
    L = x.shape[-1]
    if granularity == "per_group" and L % group_size:
        raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    return fmt, {"per_token": L, "per_group": group_size, "per_tensor": x.numel()}[granularity]


def _lsq_params(scale, zero_point, n_seg, what):
    for name, t in (("scale", scale), ("zero_point", zero_point)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.numel() != n_seg:
            raise ValueError(f"{what}: {name} must be a floating point tensor of {n_seg} entries (one per segment), got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")


def _lsq_zq(zero_point, qmin, qmax):
    return torch.clamp(torch.round(zero_point.detach().float().reshape(-1)), qmin, qmax)


def lsq_backward(x, g, scale, zero_point, fmt, granularity: str = "per_token", group_size: Optional[int] = None, grad_factor: float = 1.0,
                 want_dz: bool = True, fused: Optional[bool] = None, want_dx: bool = True):
    """The backward pass of a learned step size integer cast (LSQ / LSQ+; DESIGN.md §8 "Learned step size") -> (dx, ds, dz): dx in x's
    dtype and shape (None without want_dx: nothing is stored), ds / dz float32 [n_segments] (dz None without want_dz).  Segments as in dynamic_fixed_qdq; scale / zero_point:
    float tensors of n_segments entries; (qmin, qmax) = observer.get_qmin_qmax(fmt); zq = clamp(rint(z), qmin, qmax).  Per element,
    every operation float32 in this order:
        v = x / s + zq;  r = the forward's nearest rounding of v;  in = qmin <= r <= qmax;  q = clamp(r, qmin, qmax)
        dx = in ? g : 0;  e = in ? q - v : q - zq;  ts = g * e;  tz = in ? 0 : -(g * s)
    and per segment ds = float(grad_factor * sum float64(ts)), dz = float(grad_factor * sum float64(tz)).
    ONE launch (dmxq_lsq_backward: one read of x and g, one write of dx) where x and g share one dtype and are 16-byte aligned and the
    segment is one of lsq_class's geometries; else the chain: the same definition in torch operations on the device, same dx bit for
    bit, ds / dz up to the order of a float64 sum.  fused=None: the kernel where it applies and its geometry is not listed in
    LSQ_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.  ValueError before any GPU use."""
    from .observer import get_qmin_qmax
    fmt, S = _lsq_segment(x, fmt, granularity, group_size, "lsq_backward")
    if g.shape != x.shape:
        raise ValueError(f"lsq_backward: g has shape {tuple(g.shape)}, x has {tuple(x.shape)}")
    n_seg = x.numel() // S if S else 0
    _lsq_params(scale, zero_point, n_seg, "lsq_backward")
    require_gpu(x, "lsq_backward")
    require_gpu(g, "lsq_backward")
    qmin, qmax = get_qmin_qmax(fmt)
    with torch.no_grad():
        xc, gc = x.detach(), g.detach()
        xc = xc if xc.is_contiguous() else xc.contiguous()
        gc = gc if gc.is_contiguous() else gc.contiguous()
        s = scale.detach().float().reshape(-1).contiguous()
        z = zero_point.detach().float().reshape(-1).contiguous()
        if xc.numel() == 0:
            return (torch.empty_like(xc) if want_dx else None), s.new_zeros(n_seg), (s.new_zeros(n_seg) if want_dz else None)
        if fused is not False:
            cls = lsq_class(S, xc.dtype, granularity) if (gc.dtype == xc.dtype and fmt.precision <= 22 and xc.data_ptr() % 16 == 0
                                                           and gc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"lsq_backward: no fused kernel for segments of {S} {xc.dtype} elements ({granularity}) with a "
                                          f"{gc.dtype} gradient and {fmt!r} (base addresses {xc.data_ptr() % 16} / {gc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in LSQ_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    dx, ds, dz = _ops.lsq_backward(xc, gc, s, z, S, _LSQ_MODE[granularity], fmt.precision, ROUNDING_CODE[fmt.rounding], qmin, qmax,
                                                   float(grad_factor), bool(want_dz), bool(want_dx))
                    _lsq_routes["fused"] += 1
                    return (dx if want_dx else None), ds, (dz if want_dz else None)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _lsq_routes["chain"] += 1
        # the definition, spelled in torch on the device
        x2, g2 = xc.reshape(-1, S).float(), gc.reshape(-1, S).float()
        sc, zq = s[:, None], _lsq_zq(z, qmin, qmax)[:, None]
        v = x2 / sc + zq
        r = torch.round((v + 0.5).double() - 0.5).float()
        inside = (r >= qmin) & (r <= qmax)
        q = torch.clamp(r, qmin, qmax)
        dx = torch.where(inside, g2, torch.zeros_like(g2)).to(xc.dtype).reshape(xc.shape) if want_dx else None
        ts = g2 * torch.where(inside, q - v, q - zq)
        ds = (ts.sum(dim=1, dtype=torch.float64) * float(grad_factor)).float()
        dz = None
        if want_dz:
            tz = torch.where(inside, torch.zeros_like(g2), -(g2 * sc))
            dz = (tz.sum(dim=1, dtype=torch.float64) * float(grad_factor)).float()
        return dx, ds, dz


class _LsqCast(torch.autograd.Function):
    """forward: the static affine cast (ops.fixed_qdq, one scale per segment); backward: lsq_backward, only the gradients that are needed"""

    @staticmethod
    def forward(ctx, x, scale, zero_point, fmt, granularity, group_size, S, k, out_dtype, fused):
        from .observer import get_qmin_qmax
        qmin, qmax = get_qmin_qmax(fmt)
        xd = x.detach()
        xc = xd if xd.is_contiguous() else xd.contiguous()
        zq = _lsq_zq(zero_point, qmin, qmax).to(torch.int64)
        s = scale.detach().float().reshape(-1).contiguous()
        if xc.numel() == 0:
            y = torch.empty(xc.shape, dtype=out_dtype, device=xc.device)
        else:
            y = fixed_qdq(xc.reshape(-1, S), fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=s, zero_point=zq, ch_axis=0,
                          out_dtype=out_dtype).reshape(xc.shape)
        ctx.save_for_backward(xc, scale, zero_point)
        ctx.args = (fmt, granularity, group_size, k, fused, x.dtype)
        return y

    @staticmethod
    def backward(ctx, g):
        xc, scale, zero_point = ctx.saved_tensors
        fmt, granularity, group_size, k, fused, in_dtype = ctx.args
        need_x, need_s, need_z = ctx.needs_input_grad[:3]
        if g.dtype != in_dtype:
            g = g.to(in_dtype)
        dx, ds, dz = lsq_backward(xc, g, scale, zero_point, fmt, granularity, group_size, grad_factor=k, want_dz=bool(need_z), fused=fused,
                                  want_dx=bool(need_x))
        return (dx, ds.reshape(scale.shape).to(scale.dtype) if need_s else None,
                dz.reshape(zero_point.shape).to(zero_point.dtype) if need_z else None, None, None, None, None, None, None, None)


def lsq_fixed_qdq(x, scale, zero_point, fmt, granularity: str = "per_token", group_size: Optional[int] = None, grad_scale="lsq",
                  out_dtype: Optional[torch.dtype] = None, fused: Optional[bool] = None):
    """Integer Q->DQ with a LEARNED scale and zero point per segment (LSQ / LSQ+; DESIGN.md §8 "Learned step size"; segments as in
    dynamic_fixed_qdq).  Forward, bit for bit the static affine cast:
        y = fixed_qdq(x.reshape(-1, S), fmt..., scale=s, zero_point=clamp(rint(z), qmin, qmax).to(int64), ch_axis=0).reshape(x.shape)
    Backward: lsq_backward with grad_factor from grad_scale ("lsq": 1 / sqrt(S * qmax); None: 1; a float as given) -- x.grad is the
    clipped straight-through estimator, scale.grad / zero_point.grad come in the parameters' shapes, and only the gradients autograd
    asks for are formed.  fused: lsq_backward's.  ValueError before any GPU use: dynamic_check's cases, a format without nearest
    rounding, parameters that are not one entry per segment."""
    from .observer import get_qmin_qmax
    fmt, S = _lsq_segment(x, fmt, granularity, group_size, "lsq_fixed_qdq")
    _lsq_params(scale, zero_point, x.numel() // S if S else 0, "lsq_fixed_qdq")
    k = lsq_grad_factor(grad_scale, S, get_qmin_qmax(fmt)[1])
    require_gpu(x, "lsq_fixed_qdq")
    return _LsqCast.apply(x, scale, zero_point, fmt, granularity, group_size, S, k, out_dtype or x.dtype, fused)


# ---------------------------------------------------------------------------------------------------- dynamic scaled float cast
DYNAMIC_FLOAT_GRANULARITIES = ("per_token", "per_group", "per_tensor", "per_tile")
DYNAMIC_FLOAT_TILES = (32, 64, 128)   # the tile sizes dmxq_dynamic_float_qdq keeps in registers
# Launch geometries of dmxq_dynamic_float_qdq (dynamic_float_class) that fused=None sends to the chain although the kernel takes them:
# DYNAMIC_CHAIN_BY_DEFAULT's rule -- a class goes to the kernel by default only where tools/bench_dynamic_float.py MEASURED it faster than
# the chain on the same buffers; a class that is not gets listed here with its row.  profiles/r15_dynamic_float.txt (bf16 E4M3, us per
# call, kernel against chain): wave_row per_token [8192,4096] 30.4 against 185.6; block_row per_token [8192,14336] 90.9 against 460.2;
# group per_group 128 [8192,4096] 33.3 against 1672.9; group per_group 128 [8192,14336] 91.2 against 5831.5; tile per_tile 128
# [4096,4096] 19.9 against 140.7; tile per_tile 128 [14336,4096] 45.8 against 378.9; wave_row per_token [2048,768] 5.3 against 56.8;
# short_row per_token [60000,48] 24.3 against 332.9
# -- every class is faster, none is listed.
DYNAMIC_FLOAT_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_dynamic_float_routes = {"fused": 0, "chain": 0}
_DYNAMIC_FLOAT_CLASS_NAMES = dict(_DYNAMIC_CLASS_NAMES)
_DYNAMIC_FLOAT_CLASS_NAMES[5] = "tile"
_DYNF_GROUP, _DYNF_ROWS, _DYNF_TILE = 0, 1, 2   # dmxq_dynamic_float_mode (include/dmxq.h)


def dynamic_float_fmax(fmt) -> float:
    """the largest output of a FloatingPoint format, 2^(2^(e-1)) (2 - 2^-m): what a segment's absolute maximum is scaled to"""
    return float(2.0 ** (2 ** (fmt.exponent - 1)) * (2.0 - 2.0 ** -fmt.mantissa))


def dynamic_float_check(fmt, granularity, group_size=None, what: str = "dynamic_float_qdq"):
    """-> (format, granularity, group_size) of a scaled float cast, or ValueError: a signed FloatingPoint format with fewer than 8 exponent
    bits (8: fp32's range, no finite maximum to scale to), a known granularity, a positive group size with per_group / per_tile and none
    otherwise.  No GPU involved."""
    from .format import FloatingPoint, Format
    fmt = Format.from_shorthand(fmt) if isinstance(fmt, str) else fmt
    if not isinstance(fmt, FloatingPoint):
        raise ValueError(f"{what}: a scaled cast scales to a float format's largest value, so it needs a FloatingPoint format "
                         f"(FP[1|e|m,bias]), got {fmt!r}")
    if fmt.unsigned:
        raise ValueError(f"{what}: an unsigned format cannot be scaled by the absolute maximum, got {fmt!r}")
    if fmt.exponent >= 8:
        raise ValueError(f"{what}: a format with {fmt.exponent} exponent bits has fp32's range and no finite maximum to scale to, got {fmt!r}")
    if granularity not in DYNAMIC_FLOAT_GRANULARITIES:
        raise ValueError(f"{what}: granularity must be one of {DYNAMIC_FLOAT_GRANULARITIES}, got {granularity!r}")
    if granularity in ("per_group", "per_tile"):
        if isinstance(group_size, bool) or not isinstance(group_size, int) or group_size < 1:
            raise ValueError(f"{what}: {granularity} needs a positive integer group_size, got {group_size!r}")
    elif group_size is not None:
        raise ValueError(f"{what}: group_size goes with granularity 'per_group' / 'per_tile', got {granularity!r} with group_size "
                         f"{group_size!r}")
    return fmt, granularity, group_size


def dynamic_float_class(segment: int, dtype: torch.dtype, granularity: str = "per_token") -> Optional[str]:
    """the launch geometry dmxq_dynamic_float_qdq picks for segments of `segment` elements of `dtype` (the tile size for "per_tile"),
    asked of the library itself (dmxq_dynamic_float_class; no GPU involved), or None when it refuses them: dynamic_class's names --
    "group", "short_row", "wave_row" (here up to 8 sixteen-bit vectors per lane), "block_row" -- and "tile" (32, 64, 128)"""
    from ._lib import dtype_code, lib
    mode = {"per_group": _DYNF_GROUP, "per_tile": _DYNF_TILE}.get(granularity, _DYNF_ROWS)
    return _DYNAMIC_FLOAT_CLASS_NAMES.get(lib().dmxq_dynamic_float_class(dtype_code(dtype), mode, int(segment)))


def _scale_from_amax(amax, fmax: float, pow2_scale: bool):
    """the scale rule of the definition on a float32 tensor of absolute maxima, in torch: an IEEE division by fmax (through
    scale_channels: torch divides by a Python scalar as a multiplication by its reciprocal), the round-up to a power of two on the bits,
    and 1 where the scale is not finite or below 2^-126"""
    n = amax.numel()
    f = fmax if isinstance(fmax, torch.Tensor) else torch.full((1,), fmax, dtype=torch.float32, device=amax.device)   # (a [1] device tensor: as is)
    s = _ops.scale_channels(amax.reshape(n, 1), f, 1, True, torch.float32).reshape(n)
    if pow2_scale:
        b = s.view(torch.int32)
        b = (b & 0x7F800000) + torch.where((b & 0x007FFFFF) != 0, 0x00800000, 0).to(torch.int32)   # (a NaN: wraps to the bits of -0)
        s = b.view(torch.float32)
    ok = torch.isfinite(s) & (s >= 2.0 ** -126)
    return torch.where(ok, s, torch.ones_like(s))


def dynamic_float_qdq(x, fmt, granularity: str = "per_token", group_size: Optional[int] = None, pow2_scale: bool = False,
                      out_dtype: Optional[torch.dtype] = None, return_scale: bool = False, fused: Optional[bool] = None,
                      seed: Optional[int] = None):
    """Low-bit float Q->DQ with a scale derived from the tensor itself on every call (not in the reference, whose float
    casts are unscaled): the FP8 recipe's per-token / per-group activations and per-channel / per-tile weights.  `fmt` is a signed
    FloatingPoint format with fewer than 8 exponent bits; fmax = 2^(2^(e-1)) (2 - 2^-m) is its largest output (480 for FP[1|4|3,7], 114688
    for FP[1|5|2,15], 6 for FP[1|2|1,1]).  A segment of the contiguous tensor is the whole row of the last dim ("per_token"; per output
    channel of an [out, in] weight), `group_size` consecutive elements of it ("per_group"; it must divide the last dim), the whole tensor
    ("per_tensor"), or a group_size x group_size tile of the last two dims ("per_tile"; it must divide both, leading dims are batch:
    x.reshape(B, R/g, g, C/g, g).permute(0, 1, 3, 2, 4).reshape(-1, g * g)).  Per segment, in fp32:
        amax = max |x| (one NaN anywhere makes it NaN);  s = amax / fmax (IEEE division)
        pow2_scale: s rounded UP to a power of two on its bits, b = (b & 0x7F800000) + ((b & 0x007FFFFF) ? 0x00800000 : 0)
        s = 1 if s is not finite or below 2^-126 (an all-zero, a NaN, an Inf segment)
        y = float_q(x / s) * s: IEEE quotient, the format's nearest cast (flush flag kept; NaN / Inf saturate as in float_qdq), one fp32
        multiply, one rounding to out_dtype.
    ONE launch (dmxq_dynamic_float_qdq) for a nearest-rounding format, out_dtype == x.dtype, a 16-byte aligned tensor and: a group that is
    a power of two from 16 to 256; a row / tensor of any multiple of a 16-byte vector up to 16384 elements; a tile of 32, 64 or 128.
    Otherwise the chain of existing launches, same bits: group_minmax -> max(|mn|, |mx|) -> the scale rule in torch -> scale_channels
    (divide, float32) -> float_qdq -> scale_channels (multiply, out_dtype), on pieces of 32768 segments above 65535 segments (tiles are
    gathered into rows first).  fused=None: the kernel where it applies and its geometry (dynamic_float_class) is not listed in
    DYNAMIC_FLOAT_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.  seed: for a stochastic-rounding
    format (the chain only), as ops.float_qdq takes it.  return_scale: (y, scale) with scale float32 [n_segments], or [..., R/g, C/g] for
    tiles, on both routes.  ValueError (before any GPU use): a format that cannot be scaled, an unknown granularity, a group_size that does
    not divide.  Autograd: a straight-through estimator.  Nothing is read back to the host."""
    fmt, granularity, group_size = dynamic_float_check(fmt, granularity, group_size)
    tile = granularity == "per_tile"
    if x.dim() < (2 if tile else 1):
        raise ValueError(f"dynamic_float_qdq: {granularity} expects a tensor with at least {2 if tile else 1} dimension(s)")
    L = x.shape[-1]
    if granularity == "per_group" and L % group_size:
        raise ValueError(f"dynamic_float_qdq: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    if tile and (L % group_size or x.shape[-2] % group_size):
        raise ValueError(f"dynamic_float_qdq: the last two dimensions are {tuple(x.shape[-2:])}, not multiples of the tile size {group_size}")
    require_gpu(x, "dynamic_float_qdq")
    out_dtype = out_dtype or x.dtype
    fmax = dynamic_float_fmax(fmt)
    S = {"per_token": L, "per_group": group_size, "per_tensor": x.numel(), "per_tile": group_size}[granularity]
    mode = {"per_group": _DYNF_GROUP, "per_tile": _DYNF_TILE}.get(granularity, _DYNF_ROWS)
    fields = (fmt.mantissa, fmt.exponent, fmt.bias, bool(fmt.flush_subnormal))

    def run(xd):
        xc = xd if xd.is_contiguous() else xd.contiguous()
        sc_shape = (tuple(xc.shape[:-2]) + (xc.shape[-2] // S, L // S)) if tile else None
        if xc.numel() == 0:
            y = torch.empty(xc.shape, dtype=out_dtype, device=xc.device)
            return (y, y.new_empty(sc_shape if tile else 0, dtype=torch.float32)) if return_scale else y
        if fused is not False:
            cls = dynamic_float_class(S, xc.dtype, granularity) if (fmt.rounding == "nearest" and out_dtype == xc.dtype and fmt.mantissa <= 22
                                                                    and xc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"dynamic_float_qdq: no fused kernel for {granularity} segments of {S} {xc.dtype} elements -> "
                                          f"{out_dtype} with {fmt!r} (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in DYNAMIC_FLOAT_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    y, sc = _ops.dynamic_float_qdq(xc, mode, S, *fields, ROUNDING_CODE[fmt.rounding], bool(pow2_scale), bool(return_scale),
                                                   out_dtype)
                    _dynamic_float_routes["fused"] += 1
                    return (y, sc) if return_scale else y
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _dynamic_float_routes["chain"] += 1
        if tile:
            B = xc.numel() // (xc.shape[-2] * L)
            x2 = xc.reshape(B, xc.shape[-2] // S, S, L // S, S).permute(0, 1, 3, 2, 4).reshape(-1, S * S)
        else:
            x2 = xc.reshape(-1, S)

        def chain(part):
            mn, mx = _ops.group_minmax(part, 0, 1)
            sc = _scale_from_amax(torch.maximum(mn.abs(), mx.abs()), fmax, pow2_scale)
            q = _ops.scale_channels(part, sc, 0, True, torch.float32)
            q = float_qdq(q, *fields, False, fmt.rounding, torch.float32, seed)
            return _ops.scale_channels(q, sc, 0, False, out_dtype), sc

        if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
            y, sc = chain(x2)
        else:   # (dmxq_group_minmax takes 65535 groups: segments are independent, so the chain runs on pieces and the results are joined)
            parts = [chain(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)]
            y, sc = (torch.cat([p[k] for p in parts]) for k in range(2))
        if tile:
            y = y.reshape(B, xc.shape[-2] // S, L // S, S, S).permute(0, 1, 3, 2, 4).reshape(xc.shape)
            sc = sc.reshape(sc_shape)
        else:
            y = y.reshape(xc.shape)
        return (y, sc) if return_scale else y

    if x.requires_grad and torch.is_grad_enabled():
        return _DynamicSTE.apply(x, run)
    with torch.no_grad():
        return run(x.detach())


# ---------------------------------------------------------------------------------------------------- codebook casts
CODEBOOK_GRANULARITIES = ("per_token", "per_group", "per_tensor")
CODEBOOK_KERNEL_LEVELS = 16   # the largest table dmxq_codebook_qdq / dmxq_codebook_accumulate hold in registers (the chain: up to 256)
# Launch geometries of dmxq_codebook_qdq (codebook_class) that fused=None sends to the chain although the kernel takes them:
# DYNAMIC_FLOAT_CHAIN_BY_DEFAULT's rule -- a class goes to the kernel by default only where tools/bench_codebook.py MEASURED it faster than
# the chain on the same buffers; a class that is not gets listed here with its row.  profiles/r20_codebook.txt (bf16 NF4, us per call,
# kernel against chain): group per_group 64 [8192,4096] 55.6 against 3858.5; wave_row per_token [8192,4096] 52.9 against 581.3; group
# per_group 64 [8192,14336] 176.7 against 13431.2; block_row per_token [8192,14336] 165.3 against 1827.6; group per_group 64 [2048,768]
# 5.7 against 197.5; wave_row per_token [2048,768] 6.3 against 96.9 -- every measured class is faster, none is listed (short_row was
# not measured: it runs wave_row's kernel body with idle lanes).
CODEBOOK_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_codebook_routes = {"fused": 0, "chain": 0}
_codebook_accumulate_routes = {"fused": 0, "chain": 0}
_CODEBOOK_ACC_REPLICAS = 4096   # copies of the [K, 3] rows that codebook_accumulate's torch form spreads its index_add_ over


def _uniform_codebook(K: int):
    """linspace(-1, 1, K) in float32, as a tuple of Python floats"""
    if isinstance(K, bool) or not isinstance(K, int) or not 2 <= K <= 256:
        raise ValueError(f"CODEBOOKS['uniform']: K must be an integer from 2 to 256, got {K!r}")
    return tuple(torch.linspace(-1.0, 1.0, K, dtype=torch.float32).tolist())


#: named tables: "nf4" -- the 16 levels of bitsandbytes' NormalFloat4 (QLoRA, Dettmers et al. 2023), each exactly representable in
#: float32; "fp4_e2m1" -- the values of FP[1|2|1,1] with -0 and +0 merged, 15 levels; "uniform" -- a function, K -> linspace(-1, 1, K)
#: (as a codebook name: "uniform<K>", e.g. "uniform8")
CODEBOOKS = {
    "nf4": (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
            -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
            0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0),
    "fp4_e2m1": (-6.0, -4.0, -3.0, -2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0),
    "uniform": _uniform_codebook,
}
#: the ready setting of CastTo.set_codebook / ops.codebook_qdq: NormalFloat4 under one absolute-maximum scale per 64 elements
NF4 = {"codebook": "nf4", "per_group": 64}
_codebook_device_cache = {}   # (levels, device) -> float32 [K] tensor: a named / host table is uploaded once per device


def _codebook_host_levels(codebook, what):
    """a name, list, tuple or CPU tensor -> the checked tuple of float32 values (ValueError); a device tensor -> None"""
    if isinstance(codebook, torch.Tensor) and codebook.is_cuda:
        return None
    if isinstance(codebook, str):
        if codebook.startswith("uniform") and codebook[7:].isdigit():
            return _uniform_codebook(int(codebook[7:]))
        lv = CODEBOOKS.get(codebook)
        if lv is None or callable(lv):
            raise ValueError(f"{what}: unknown codebook {codebook!r}; known: {sorted(k for k, v in CODEBOOKS.items() if not callable(v))} and "
                             f"'uniform<K>', or give the levels as a list or tensor")
        return tuple(lv)
    if isinstance(codebook, torch.Tensor):
        if codebook.dim() != 1 or not codebook.is_floating_point():
            raise ValueError(f"{what}: a codebook tensor must be a 1-d float tensor of levels, got shape {tuple(codebook.shape)} {codebook.dtype}")
        vals = codebook.detach().to(torch.float32).tolist()
    elif isinstance(codebook, (list, tuple)):
        try:
            vals = torch.tensor([float(v) for v in codebook], dtype=torch.float32).tolist()   # (rounded to float32 once, here)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: the levels of a codebook must be numbers, got {codebook!r}") from None
    else:
        raise ValueError(f"{what}: a codebook is a name, a list of levels or a 1-d tensor, got {type(codebook).__name__}")
    if not 2 <= len(vals) <= 256:
        raise ValueError(f"{what}: a codebook has 2 to 256 levels, got {len(vals)}")
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{what}: the levels of a codebook must be finite, got {vals}")
    if any(b < a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"{what}: the levels of a codebook must be non-decreasing, got {vals}")
    return tuple(vals)


def codebook_check(codebook, granularity="per_group", group_size=64, norm=None, what: str = "codebook_qdq"):
    """-> (levels, granularity, group_size, norm) of a codebook cast, or ValueError before any GPU use: `levels` is the checked tuple of
    float32 values of a name ("nf4", "fp4_e2m1", "uniform<K>"), list or CPU tensor -- 2 to 256 finite, non-decreasing levels -- or a
    device tensor as it is (1-d, 2 to 256 entries by its shape; never read back); a known granularity, a positive integer group_size
    with per_group and none otherwise (that it divides the last dimension is checked against the tensor); norm None or a positive finite
    number."""
    levels = _codebook_host_levels(codebook, what)
    if levels is None:
        if codebook.dim() != 1 or not codebook.is_floating_point() or not 2 <= codebook.shape[0] <= 256:
            raise ValueError(f"{what}: a codebook tensor must be a 1-d float tensor of 2 to 256 levels, got shape {tuple(codebook.shape)} "
                             f"{codebook.dtype}")
        levels = codebook
    if granularity not in CODEBOOK_GRANULARITIES:
        raise ValueError(f"{what}: granularity must be one of {CODEBOOK_GRANULARITIES}, got {granularity!r}")
    if granularity == "per_group":
        if isinstance(group_size, bool) or not isinstance(group_size, int) or group_size < 1:
            raise ValueError(f"{what}: per_group needs a positive integer group_size, got {group_size!r}")
    else:
        group_size = None   # (the default group_size of the signature means nothing without per_group)
    if norm is not None:
        if isinstance(norm, bool) or not isinstance(norm, (int, float)) or not (0.0 < float(norm) < math.inf):
            raise ValueError(f"{what}: norm must be None (the table's own largest magnitude) or a positive finite number, got {norm!r}")
        norm = float(torch.tensor(float(norm), dtype=torch.float32))   # (the float32 value the kernel receives)
        if not (0.0 < norm < math.inf):
            raise ValueError(f"{what}: norm is not a positive finite float32 number")
    return levels, granularity, group_size, norm


def _codebook_tensor(levels, device):
    """the float32 [K] device tensor of a checked table: a device tensor as it is (converted on the device if need be), a host tuple
    uploaded once per device and kept (a later call, also inside a graph capture, copies nothing)"""
    if isinstance(levels, torch.Tensor):
        t = levels.detach()
        t = t if t.dtype == torch.float32 else t.float()
        t = t if t.device == device else t.to(device)
        return t if t.is_contiguous() else t.contiguous()
    key = (levels, str(device))
    t = _codebook_device_cache.get(key)
    if t is None:
        t = _codebook_device_cache[key] = torch.tensor(levels, dtype=torch.float32, device=device)
    return t


def codebook_class(segment: int, dtype: torch.dtype, whole_rows: bool = False) -> Optional[str]:
    """the launch geometry dmxq_codebook_qdq / dmxq_codebook_accumulate pick for segments of `segment` elements of `dtype` (whole_rows:
    per_token / per_tensor), asked of the library itself (no GPU involved), or None when they refuse them: dynamic_float_class's names
    without "tile" """
    from ._lib import dtype_code, lib
    return _DYNAMIC_CLASS_NAMES.get(lib().dmxq_codebook_class(dtype_code(dtype), _DYNF_ROWS if whole_rows else _DYNF_GROUP, int(segment)))


def _codebook_per_group(granularity, group_size, per_group, what):
    """the per_group=g spelling of (granularity, group_size)"""
    if per_group is None:
        return granularity, group_size
    if granularity != "per_group":
        raise ValueError(f"{what}: per_group={per_group!r} names the granularity itself, got granularity {granularity!r} beside it")
    return "per_group", per_group


def _codebook_segment(x, granularity, group_size, what):
    if x.dim() < 1:
        raise ValueError(f"{what}: {granularity} expects a tensor with at least 1 dimension")
    L = x.shape[-1]
    if granularity == "per_group" and L % group_size:
        raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    return {"per_token": L, "per_group": group_size, "per_tensor": x.numel()}[granularity]


def _codebook_chain(x2, c, norm_t, want_lookup=True, out_dtype=None):
    """the definition on the rows of x2 [n, S] as a chain of launches -> (y or None, scale [n], u [n, S] float32, idx int64 [n, S])"""
    K = c.shape[0]
    t = (c[:-1] + c[1:]) * 0.5
    z = torch.argmin(c.abs())   # (the first of equal minima: the lowest index)

    def chain(part):
        mn, mx = _ops.group_minmax(part, 0, 1)
        sc = _scale_from_amax(torch.maximum(mn.abs(), mx.abs()), norm_t, False)
        u = _ops.scale_channels(part, sc, 0, True, torch.float32)
        idx = torch.bucketize(u, t, right=False)
        idx = torch.where(torch.isnan(u), z, idx)
        y = _ops.scale_channels(c[idx], sc, 0, False, out_dtype) if want_lookup else sc
        return y, sc, u, idx

    if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
        y, sc, u, idx = chain(x2)
    else:   # (dmxq_group_minmax takes 65535 groups: segments are independent, so the chain runs on pieces and the results are joined)
        parts = [chain(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)]
        y, sc, u, idx = (torch.cat([p[k] for p in parts]) for k in range(4))
    return (y if want_lookup else None), sc, u, idx


def _codebook_norm_tensor(c, norm):
    """the [1] float32 device tensor the chain divides the maxima by: the given norm, or max(|c_0|, |c_{K-1}|) formed on the device"""
    if norm is not None:
        return torch.full((1,), norm, dtype=torch.float32, device=c.device)
    return torch.maximum(c[:1].abs(), c[-1:].abs())


def codebook_qdq(x, codebook, granularity: str = "per_group", group_size: Optional[int] = 64, norm: Optional[float] = None,
                 out_dtype: Optional[torch.dtype] = None, return_scale: bool = False, return_index: bool = False,
                 fused: Optional[bool] = None, per_group: Optional[int] = None):
    """Q->DQ onto a small table of ARBITRARY levels under a per-segment absolute-maximum scale (DESIGN.md §8 "Codebook casts"; not in
    the reference): NF4 (ops.NF4), Lloyd-Max / k-means tables (ops.codebook_fit).  `codebook`: a name of ops.CODEBOOKS, a list / CPU tensor
    of K non-decreasing finite levels (checked: ValueError), or a device tensor (taken as is, never read back), 2 <= K <= 256.  In fp32:
    thresholds t_j = (c_j + c_{j+1}) * 0.5; z = the lowest index of the level with the smallest |c|; and per segment of the contiguous
    tensor (the row of the last dim with "per_token", `group_size` elements of it with "per_group", the whole tensor with "per_tensor"):
        amax = max |x| (one NaN anywhere makes it NaN);  s = amax / norm (IEEE; norm=None: max(|c_0|, |c_{K-1}|), formed on the device);
        s = 1 if s is not finite or below 2^-126;  u = x / s (IEEE);  idx = #{j : u > t_j} = bucketize(u, t, right=False), a tie goes
        to the lower level, a NaN u takes idx = z;  y = c[idx] * s: one fp32 multiply, one rounding to out_dtype.
    ONE launch (dmxq_codebook_qdq) for K <= 16, out_dtype == x.dtype, a 16-byte aligned tensor and: a group that is a power of two from
    16 to 256; a row / tensor of any multiple of a 16-byte vector up to 16384 elements.  Otherwise the chain, same bits: group_minmax ->
    the scale rule in torch -> scale_channels (divide, float32) -> torch.bucketize with the NaN override -> gather -> scale_channels
    (multiply, out_dtype), on pieces of 32768 segments above 65535 segments.  fused=None: the kernel where it applies and its geometry
    (codebook_class) is not listed in CODEBOOK_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.
    per_group=g spells granularity="per_group", group_size=g, so that a setting such as ops.NF4 unpacks into the call:
    codebook_qdq(x, **ops.NF4).
    Returns y, followed by scale (float32 [n_segments]) with return_scale and index (uint8, x's shape) with return_index.  Autograd: a
    straight-through estimator.  Nothing is read back to the host on either route."""
    granularity, group_size = _codebook_per_group(granularity, group_size, per_group, "codebook_qdq")
    levels, granularity, group_size, norm = codebook_check(codebook, granularity, group_size, norm)
    S = _codebook_segment(x, granularity, group_size, "codebook_qdq")
    require_gpu(x, "codebook_qdq")
    out_dtype = out_dtype or x.dtype
    mode = _DYNF_GROUP if granularity == "per_group" else _DYNF_ROWS
    K = len(levels) if not isinstance(levels, torch.Tensor) else levels.shape[0]

    def pick(y, sc, idx):
        out = (y,) + ((sc,) if return_scale else ()) + ((idx,) if return_index else ())
        return out if len(out) > 1 else y

    def run(xd):
        xc = xd if xd.is_contiguous() else xd.contiguous()
        if xc.numel() == 0:
            return pick(torch.empty(xc.shape, dtype=out_dtype, device=xc.device), torch.empty(0, dtype=torch.float32, device=xc.device),
                        torch.empty(xc.shape, dtype=torch.uint8, device=xc.device))
        c = _codebook_tensor(levels, xc.device)
        if fused is not False:
            cls = codebook_class(S, xc.dtype, mode == _DYNF_ROWS) if (K <= CODEBOOK_KERNEL_LEVELS and out_dtype == xc.dtype
                                                                       and xc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"codebook_qdq: no fused kernel for {granularity} segments of {S} {xc.dtype} elements -> {out_dtype} "
                                          f"with {K} levels (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in CODEBOOK_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    y, sc, idx = _ops.codebook_qdq(xc, mode, S, c, 0.0 if norm is None else norm, bool(return_scale), bool(return_index), out_dtype)
                    _codebook_routes["fused"] += 1
                    return pick(y, sc, idx)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _codebook_routes["chain"] += 1
        y, sc, _, idx = _codebook_chain(xc.reshape(-1, S), c, _codebook_norm_tensor(c, norm), True, out_dtype)
        return pick(y.reshape(xc.shape), sc, idx.to(torch.uint8).reshape(xc.shape) if return_index else None)

    if x.requires_grad and torch.is_grad_enabled():
        return _DynamicSTE.apply(x, run)
    with torch.no_grad():
        return run(x.detach())


def codebook_accumulate(x, codebook, granularity: str = "per_group", group_size: Optional[int] = 64, norm: Optional[float] = None, acc=None,
                        accumulate: bool = False, fused: Optional[bool] = None, per_group: Optional[int] = None):
    """The weighted Lloyd statistics of x under a table (DESIGN.md §8 "Codebook casts"), float64 [K, 3] on the device: with scale s,
    quotient u and index idx formed exactly as codebook_qdq forms them, over the elements whose u is finite,
        A[idx, 0] += w u;  A[idx, 1] += w;  A[idx, 2] += 1,   w = (double)s * (double)s
    -- the true-MSE form: an element's error is s^2 (u - c)^2, so the best level of a cell is A[k, 0] / A[k, 1].  accumulate=True adds
    into `acc` (several tensors or batches under one table), else `acc` (or a fresh tensor) is overwritten.  ONE pass over x plus a fold
    launch (dmxq_codebook_accumulate: no floating-point atomics, the same input gives the same bits) where codebook_qdq's kernel applies;
    otherwise the chain's (s, u, idx) and torch index_add_.  fused: as codebook_qdq.  Nothing is read back to the host."""
    granularity, group_size = _codebook_per_group(granularity, group_size, per_group, "codebook_accumulate")
    levels, granularity, group_size, norm = codebook_check(codebook, granularity, group_size, norm, what="codebook_accumulate")
    S = _codebook_segment(x, granularity, group_size, "codebook_accumulate")
    require_gpu(x, "codebook_accumulate")
    K = len(levels) if not isinstance(levels, torch.Tensor) else levels.shape[0]
    if acc is not None and (acc.dtype != torch.float64 or tuple(acc.shape) != (K, 3) or acc.device != x.device or not acc.is_contiguous()):
        raise ValueError(f"codebook_accumulate: acc must be a contiguous float64 [{K}, 3] tensor on x's device")
    if accumulate and acc is None:
        raise ValueError("codebook_accumulate: accumulate=True needs acc")
    mode = _DYNF_GROUP if granularity == "per_group" else _DYNF_ROWS
    with torch.no_grad():
        xd = x.detach()
        xc = xd if xd.is_contiguous() else xd.contiguous()
        if acc is None:
            acc = torch.zeros(K, 3, dtype=torch.float64, device=xc.device)
        elif not accumulate and xc.numel() == 0:
            acc.zero_()
        if xc.numel() == 0:
            return acc
        c = _codebook_tensor(levels, xc.device)
        if fused is not False:
            cls = codebook_class(S, xc.dtype, mode == _DYNF_ROWS) if (K <= CODEBOOK_KERNEL_LEVELS and xc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"codebook_accumulate: no fused kernel for {granularity} segments of {S} {xc.dtype} elements with {K} "
                                          f"levels (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None:
                try:
                    _ops.codebook_accumulate(xc, mode, S, c, 0.0 if norm is None else norm, acc, bool(accumulate))
                    _codebook_accumulate_routes["fused"] += 1
                    return acc
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _codebook_accumulate_routes["chain"] += 1
        _, sc, u, idx = _codebook_chain(xc.reshape(-1, S), c, _codebook_norm_tensor(c, norm), False)
        fin = torch.isfinite(u)
        w = (sc.double() * sc.double())[:, None].expand_as(u)
        zero = torch.zeros((), dtype=torch.float64, device=xc.device)
        terms = torch.stack([torch.where(fin, w * u.double(), zero), torch.where(fin, w, zero), fin.double()], dim=-1).reshape(-1, 3)
        # index_add_ adds with atomics: onto K rows alone every element of the tensor meets every other one (measured: seconds for 8 M
        # elements), so the rows are kept in _CODEBOOK_ACC_REPLICAS copies, element i adding to copy i mod R, and the copies are summed
        n = idx.numel()
        R = min(_CODEBOOK_ACC_REPLICAS, n)
        rows = idx.reshape(-1) + K * (torch.arange(n, device=xc.device) % R)
        A = torch.zeros(R * K, 3, dtype=torch.float64, device=xc.device).index_add_(0, rows, terms).reshape(R, K, 3).sum(dim=0)
        if accumulate:
            acc += A
        else:
            acc.copy_(A)
        return acc


def codebook_fit(x, codebook="nf4", granularity: str = "per_group", group_size: Optional[int] = 64, norm: Optional[float] = None, iters: int = 8,
                 return_history: bool = False, fused: Optional[bool] = None, per_group: Optional[int] = None):
    """Fits a table to a tensor (or a list of tensors sharing it) by weighted Lloyd iterations on the device (DESIGN.md §8 "Codebook
    casts") -> (levels float32 [K] on the device, norm) or (levels, norm, history).  Every iteration: A = codebook_accumulate over the
    tensors, then c_k <- float(A[k, 0] / A[k, 1]) where A[k, 2] > 0 (an empty level keeps its value) -- the minimiser of the true
    squared error sum s^2 (u - c)^2 over every cell, so the error never rises; cells are intervals, so the levels stay ordered.  The update
    is torch on the K-vector on the device: no host synchronisation inside the loop, an iteration is capturable.  `norm` stays FIXED across
    the iterations: None is resolved ONCE from the initial table, max(|c_0|, |c_{K-1}|) (the one read of a device table; a name or list
    needs none), and returned -- pass the same norm when casting with the fitted table.  return_history: the relative L2 error
    sqrt(sum_sq_err / sum_sq_ref) (ops.error_stats rows) before every iteration and after the last, float64 [iters + 1] on the device."""
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    if not xs:
        raise ValueError("codebook_fit: no tensor to fit the table to")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"codebook_fit: iters must be a non-negative integer, got {iters!r}")
    granularity, group_size = _codebook_per_group(granularity, group_size, per_group, "codebook_fit")
    levels, granularity, group_size, norm = codebook_check(codebook, granularity, group_size, norm, what="codebook_fit")
    for t in xs:
        _codebook_segment(t, granularity, group_size, "codebook_fit")
        require_gpu(t, "codebook_fit")
    if norm is None:
        if isinstance(levels, torch.Tensor):
            norm = float(torch.maximum(levels[0].abs(), levels[-1].abs()).float())   # (the ONE read of a device table, before the loop)
        else:
            norm = max(abs(levels[0]), abs(levels[-1]))
        if not (0.0 < norm < math.inf):
            raise ValueError(f"codebook_fit: the initial table gives norm {norm!r}; pass a positive finite norm")
    with torch.no_grad():
        c = _codebook_tensor(levels, xs[0].device).clone()
        K = c.shape[0]

        def rel_error():
            row = None
            for t in xs:
                y = codebook_qdq(t.detach(), c, granularity, group_size, norm, fused=fused)
                row = error_stats(t.detach(), y, out=row, accumulate=row is not None)
            return torch.sqrt(row[0] / row[1])

        history = []
        for _ in range(iters):
            if return_history:
                history.append(rel_error())
            A = torch.zeros(K, 3, dtype=torch.float64, device=c.device)
            for t in xs:
                codebook_accumulate(t, c, granularity, group_size, norm, acc=A, accumulate=True, fused=fused)
            c = torch.where(A[:, 2] > 0, (A[:, 0] / A[:, 1]).float(), c)
        if return_history:
            history.append(rel_error())
            return c, norm, torch.stack(history)
        return c, norm


# ---------------------------------------------------------------------------------------------------- vector codebook casts
VQ_DIMS = (2, 4, 8)
# Launch geometries of dmxq_vq_qdq (vq_class) that fused=None sends to the chain although the kernel takes them: CODEBOOK_CHAIN_BY_DEFAULT's
# rule -- a class goes to the kernel by default only where tools/bench_vq.py MEASURED it faster than the chain on the same buffers; a
# class that is not gets listed here with its row.
# profiles/r25_vq.txt (bf16, us per call, kernel against chain, tables [16,2] / [256,2] / [256,4] / [256,8]): group per_group 64 [4096,4096]
# 39.4 / 346.8 / 289.7 / 284.1 against 4145.6 / 28499.5 / 26168.5 / 27105.2, [14336,4096] 117.6 / 1205.6 / 987.6 / 976.2 against 14152.1 /
# 99508.5 / 91211.6 / 94449.5, [2048,768] 6.5 / 40.2 / 34.8 / 39.2 against 450.0 / 2719.1 / 2494.4 / 2599.1; wave_row per_token [4096,4096]
# 37.6 / 351.6 / 293.1 / 293.1 against 2500.4 / 26738.1 / 24441.1 / 25391.7, [14336,4096] 110.1 / 1194.4 / 989.9 / 977.0 against 8514.9 /
# 92825.1 / 85643.1 / 88395.6, [2048,768] 7.5 / 50.8 / 43.6 / 41.4 against 343.0 / 2610.1 / 2388.9 / 2504.7; block_row per_token
# [2048,8192], tables [16,2] / [256,4] / [256,8], 62.7 / 541.9 / 535.9 against 2500.6 / 24410.9 / 25365.5; short_row per_token [60000,48]
# 65.8 / 489.3 / 487.2 against 820.5 / 4530.0 / 4742.2 -- every class is faster (9 - 120 x), none is listed.
VQ_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_vq_routes = {"fused": 0, "chain": 0}
_vq_accumulate_routes = {"fused": 0, "chain": 0}
#: the chain's bound: its search forms float32 [vectors, K] distance tensors (never [vectors, K, d]: the components are subtracted, squared
#: and added one at a time) on pieces of at most this many entries -- 64 MiB each, three alive at a time
VQ_CHAIN_PIECE_ENTRIES = 1 << 24
_vq_device_cache = {}   # (rows, device) -> float32 [K, d] tensor: a host table is uploaded once per device


def vq_grid(levels, dim: int):
    """the product table of a scalar codebook: every dim-tuple of its levels as a row, rows in lexicographic order (the first component
    varies slowest) -> float32 CPU tensor [len(levels) ** dim, dim].  levels: a name of ops.CODEBOOKS ("nf4", "uniform4", ...) or a
    list of levels, checked as codebook_check checks them.  ValueError when dim is not 2, 4 or 8 or the table would exceed 256 rows:
    vq_grid("uniform4", 4) and vq_grid("nf4", 2) are the two largest common ones."""
    import itertools
    if isinstance(dim, bool) or not isinstance(dim, int) or dim not in VQ_DIMS:
        raise ValueError(f"vq_grid: dim must be one of {VQ_DIMS}, got {dim!r}")
    if isinstance(levels, torch.Tensor) and levels.is_cuda:
        raise ValueError("vq_grid: the levels are a name, a list or a CPU tensor (a device tensor would have to be read back)")
    lv = _codebook_host_levels(levels, "vq_grid")
    if len(lv) ** dim > 256:
        raise ValueError(f"vq_grid: {len(lv)} levels in {dim} dimensions give {len(lv) ** dim} rows, more than 256")
    return torch.tensor(list(itertools.product(lv, repeat=dim)), dtype=torch.float32)


def _vq_host_rows(codebook, what):
    """a list of rows or a CPU tensor [K, d] -> the checked tuple of tuples of float32 values (ValueError); a device tensor -> None"""
    if isinstance(codebook, torch.Tensor):
        if codebook.dim() != 2 or not codebook.is_floating_point():
            raise ValueError(f"{what}: a table tensor must be a 2-d float tensor [K, d], got shape {tuple(codebook.shape)} {codebook.dtype}")
        if codebook.is_cuda:
            return None
        rows = codebook.detach().to(torch.float32).tolist()
    elif isinstance(codebook, (list, tuple)):
        try:
            rows = [[float(v) for v in r] for r in codebook]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: a table is a list of rows of numbers, got {codebook!r}") from None
        if len({len(r) for r in rows}) > 1:
            raise ValueError(f"{what}: the rows of a table must have one length, got lengths {sorted({len(r) for r in rows})}")
        if rows and rows[0]:
            rows = torch.tensor(rows, dtype=torch.float32).tolist()   # (rounded to float32 once, here)
    else:
        raise ValueError(f"{what}: a table is a list of rows, a [K, d] tensor or {{'grid': name, 'dim': d}}, got {type(codebook).__name__}")
    return tuple(tuple(r) for r in rows)


def vq_check(codebook, dim=None, granularity="per_group", group_size=64, norm=None, what: str = "vq_qdq"):
    """-> (table, K, d, granularity, group_size, norm) of a vector codebook cast, or ValueError before any GPU use.  `table`: the checked
    tuple of K rows of d float32 values of a list of rows or a CPU tensor [K, d] (or of {"grid": levels, "dim": d}: vq_grid) -- finite,
    2 <= K <= 256, d in {2, 4, 8}; no order is required, duplicate rows are allowed -- or a device tensor as it is ([K, d] by its shape;
    never read back).  dim: None, or the d the table must have.  A known granularity; with per_group a positive integer group_size that is
    a multiple of d (that it divides the last dimension is checked against the tensor); norm None or a positive finite number."""
    if isinstance(codebook, dict):
        if set(codebook) != {"grid", "dim"}:
            raise ValueError(f"{what}: a table given as a dict is {{'grid': levels, 'dim': d}}, got {codebook!r}")
        codebook = vq_grid(codebook["grid"], codebook["dim"])
    rows = _vq_host_rows(codebook, what)
    K, d = (len(rows), len(rows[0]) if rows else 0) if rows is not None else tuple(codebook.shape)
    if not 2 <= K <= 256:
        raise ValueError(f"{what}: a table has 2 to 256 rows, got {K}")
    if d not in VQ_DIMS:
        raise ValueError(f"{what}: the rows of a table have {VQ_DIMS} components, got {d}")
    if dim is not None and (isinstance(dim, bool) or not isinstance(dim, int) or dim != d):
        raise ValueError(f"{what}: dim={dim!r} beside a table whose rows have {d} components")
    if rows is not None and not all(math.isfinite(v) for r in rows for v in r):
        raise ValueError(f"{what}: the entries of a table must be finite")
    if granularity not in CODEBOOK_GRANULARITIES:
        raise ValueError(f"{what}: granularity must be one of {CODEBOOK_GRANULARITIES}, got {granularity!r}")
    if granularity == "per_group":
        if isinstance(group_size, bool) or not isinstance(group_size, int) or group_size < 1:
            raise ValueError(f"{what}: per_group needs a positive integer group_size, got {group_size!r}")
        if group_size % d:
            raise ValueError(f"{what}: the group size {group_size} is not a multiple of the table's d = {d}: a vector would straddle two groups")
    else:
        group_size = None   # (the default group_size of the signature means nothing without per_group)
    if norm is not None:
        if isinstance(norm, bool) or not isinstance(norm, (int, float)) or not (0.0 < float(norm) < math.inf):
            raise ValueError(f"{what}: norm must be None (the table's own largest magnitude) or a positive finite number, got {norm!r}")
        norm = float(torch.tensor(float(norm), dtype=torch.float32))   # (the float32 value the kernel receives)
        if not (0.0 < norm < math.inf):
            raise ValueError(f"{what}: norm is not a positive finite float32 number")
    return (rows if rows is not None else codebook), K, d, granularity, group_size, norm


def _vq_tensor(table, device):
    """the float32 [K, d] device tensor of a checked table: a device tensor as it is (converted on the device if need be), a host tuple
    uploaded once per device and kept (a later call, also inside a graph capture, copies nothing)"""
    if isinstance(table, torch.Tensor):
        t = table.detach()
        t = t if t.dtype == torch.float32 else t.float()
        t = t if t.device == device else t.to(device)
        return t if t.is_contiguous() else t.contiguous()
    key = (table, str(device))
    t = _vq_device_cache.get(key)
    if t is None:
        t = _vq_device_cache[key] = torch.tensor(table, dtype=torch.float32, device=device)
    return t


def vq_class(segment: int, dtype: torch.dtype, dim: int, K: int, whole_rows: bool = False) -> Optional[str]:
    """the launch geometry dmxq_vq_qdq / dmxq_vq_accumulate pick for segments of `segment` elements of `dtype` under a [K, dim] table
    (whole_rows: per_token / per_tensor), asked of the library itself (no GPU involved), or None where they refuse: codebook_class's
    names.  float32 takes dim 2 and 4; the sixteen-bit dtypes 2, 4 and 8."""
    from ._lib import dtype_code, lib
    return _DYNAMIC_CLASS_NAMES.get(lib().dmxq_vq_class(dtype_code(dtype), _DYNF_ROWS if whole_rows else _DYNF_GROUP, int(segment), int(dim), int(K)))


def _vq_segment(x, d, granularity, group_size, what):
    if x.dim() < 1:
        raise ValueError(f"{what}: {granularity} expects a tensor with at least 1 dimension")
    L = x.shape[-1]
    if granularity == "per_group" and L % group_size:
        raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    if granularity == "per_token" and L % d:
        raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the table's d = {d}")
    if granularity == "per_tensor" and x.numel() % d:
        raise ValueError(f"{what}: the tensor has {x.numel()} elements, not a multiple of the table's d = {d}")
    return {"per_token": L, "per_group": group_size, "per_tensor": x.numel()}[granularity]


def _vq_distances(uv, c):
    """D_k(u) of the definition for the vectors uv [n, d] against the table c [K, d] -> float32 [n, K]: per component one subtract and one
    multiply, the products added left to right -- separate torch launches, each rounded on its own"""
    acc = None
    for j in range(c.shape[1]):
        t = uv[:, j:j + 1] - c[:, j][None, :]
        p = t * t
        acc = p if acc is None else acc + p
    return acc


def _vq_choose(uv, c, z):
    """the row choice: NaN distances count as +Inf, argmin takes the first minimum (the lowest index), a vector whose minimum is +Inf takes z"""
    D = _vq_distances(uv, c)
    D = torch.where(torch.isnan(D), torch.full_like(D, math.inf), D)
    idx = torch.argmin(D, dim=1)
    best = D.gather(1, idx[:, None])[:, 0]
    return torch.where(best == math.inf, z, idx)


def _vq_zero_row(c):
    """z, the lowest index minimising D_k(0), as a 0-d int64 device tensor"""
    return _vq_choose(torch.zeros(1, c.shape[1], dtype=torch.float32, device=c.device), c, torch.zeros((), dtype=torch.int64, device=c.device))[0]


def _vq_chain(x2, c, norm_t, want_lookup=True, out_dtype=None):
    """the definition on the rows of x2 [n, S] as a chain of launches -> (y or None, scale [n], u [n, S] float32, idx int64 [n, S / d]).
    Segments are independent: the chain runs on pieces of at most DYNAMIC_CHAIN_PIECE segments (dmxq_group_minmax takes 65535), and the
    search inside a piece on at most VQ_CHAIN_PIECE_ENTRIES // K vectors at a time."""
    K, d = c.shape
    z = _vq_zero_row(c)
    step = max(1, VQ_CHAIN_PIECE_ENTRIES // K)

    def chain(part):
        mn, mx = _ops.group_minmax(part, 0, 1)
        sc = _scale_from_amax(torch.maximum(mn.abs(), mx.abs()), norm_t, False)
        u = _ops.scale_channels(part, sc, 0, True, torch.float32)
        uv = u.reshape(-1, d)
        idx = torch.cat([_vq_choose(uv[i:i + step], c, z) for i in range(0, uv.shape[0], step)]) if uv.shape[0] > step else _vq_choose(uv, c, z)
        y = _ops.scale_channels(c[idx].reshape(part.shape), sc, 0, False, out_dtype) if want_lookup else sc
        return y, sc, u, idx.reshape(part.shape[0], -1)

    if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
        y, sc, u, idx = chain(x2)
    else:
        parts = [chain(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)]
        y, sc, u, idx = (torch.cat([p[k] for p in parts]) for k in range(4))
    return (y if want_lookup else None), sc, u, idx


def _vq_norm_tensor(c, norm):
    """the [1] float32 device tensor the chain divides the maxima by: the given norm, or max |c_kj| formed on the device"""
    if norm is not None:
        return torch.full((1,), norm, dtype=torch.float32, device=c.device)
    return c.abs().max().reshape(1)


def _vq_kernel_class(xc, S, d, K, mode, same_dtype=True):
    """the kernel's geometry for the call, or None where the front end must run the chain"""
    if not same_dtype or xc.data_ptr() % 16:
        return None
    return vq_class(S, xc.dtype, d, K, mode == _DYNF_ROWS)


def vq_qdq(x, codebook, granularity: str = "per_group", group_size: Optional[int] = 64, norm: Optional[float] = None,
           out_dtype: Optional[torch.dtype] = None, return_scale: bool = False, return_index: bool = False, fused: Optional[bool] = None,
           per_group: Optional[int] = None):
    """Q->DQ onto the rows of a [K, d] table under a per-segment absolute-maximum scale (DESIGN.md §8 "Vector codebook casts"; not in the
    reference): d consecutive elements of the last dimension are replaced together by one row -- GPTVQ / AQLM / QuIP#-style vector
    quantisation (d = 2, K = 256: 4 bits per weight; d = 4: 2 bits; d = 8: 1 bit).  `codebook`: a list of rows or CPU tensor [K, d]
    (checked: ValueError), {"grid": levels, "dim": d} (ops.vq_grid), or a device tensor (taken as is, never read back); 2 <= K <= 256,
    d in {2, 4, 8}.  In fp32, every operation rounded on its own:
        D_k(u) = (((t_0 t_0) + t_1 t_1) + ...) + t_{d-1} t_{d-1}, t_j = u_j - c_kj;  z = the lowest k minimising D_k(0);
    and per segment (codebook_qdq's segments; per_group needs g % d == 0, per_token L % d == 0, per_tensor numel % d == 0):
        amax, s = amax / norm (norm=None: max |c_kj|, formed on the device) and the fallback s = 1 as codebook_qdq;  u = x / s (IEEE);
        per vector: best = +Inf, idx = z, for k = 0 .. K-1: D_k(u) < best takes k -- a tie keeps the lower index, a vector whose distances
        are all NaN or +Inf takes z;  y_j = c[idx][j] * s: one fp32 multiply, one rounding to out_dtype.
    ONE launch (dmxq_vq_qdq) where vq_class takes the call, out_dtype == x.dtype and the base is 16-byte aligned.  Otherwise the chain,
    same bits: group_minmax -> the scale rule in torch -> scale_channels (divide, float32) -> per component subtract, multiply and
    left-to-right adds into a [vectors, K] distance tensor -> where(isnan(D), inf, D) -> argmin (the first minimum) -> the z override where
    the minimum is +Inf -> gather -> scale_channels (multiply, out_dtype); on pieces of 32768 segments above 65535 segments and of
    VQ_CHAIN_PIECE_ENTRIES // K vectors, so that no temporary exceeds 64 MiB.  fused=None: the kernel where it applies and its geometry
    is not listed in VQ_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.  per_group=g spells
    granularity="per_group", group_size=g.
    Returns y, followed by scale (float32 [n_segments]) with return_scale and index (uint8, x.shape[:-1] + (L / d,)) with return_index.
    Autograd: a straight-through estimator.  Nothing is read back to the host on either route."""
    granularity, group_size = _codebook_per_group(granularity, group_size, per_group, "vq_qdq")
    table, K, d, granularity, group_size, norm = vq_check(codebook, None, granularity, group_size, norm)
    S = _vq_segment(x, d, granularity, group_size, "vq_qdq")
    require_gpu(x, "vq_qdq")
    out_dtype = out_dtype or x.dtype
    mode = _DYNF_GROUP if granularity == "per_group" else _DYNF_ROWS

    def pick(y, sc, idx):
        out = (y,) + ((sc,) if return_scale else ()) + ((idx,) if return_index else ())
        return out if len(out) > 1 else y

    def run(xd):
        xc = xd if xd.is_contiguous() else xd.contiguous()
        ishape = tuple(xc.shape[:-1]) + (xc.shape[-1] // d,)
        if xc.numel() == 0:
            return pick(torch.empty(xc.shape, dtype=out_dtype, device=xc.device), torch.empty(0, dtype=torch.float32, device=xc.device),
                        torch.empty(ishape, dtype=torch.uint8, device=xc.device))
        c = _vq_tensor(table, xc.device)
        if fused is not False:
            cls = _vq_kernel_class(xc, S, d, K, mode, out_dtype == xc.dtype)
            if cls is None and fused:
                raise NotImplementedError(f"vq_qdq: no fused kernel for {granularity} segments of {S} {xc.dtype} elements -> {out_dtype} "
                                          f"with a [{K}, {d}] table (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in VQ_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    y, sc, idx = _ops.vq_qdq(xc, mode, S, c, 0.0 if norm is None else norm, bool(return_scale), bool(return_index), out_dtype)
                    _vq_routes["fused"] += 1
                    return pick(y, sc, idx)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _vq_routes["chain"] += 1
        y, sc, _, idx = _vq_chain(xc.reshape(-1, S), c, _vq_norm_tensor(c, norm), True, out_dtype)
        return pick(y.reshape(xc.shape), sc, idx.to(torch.uint8).reshape(ishape) if return_index else None)

    if x.requires_grad and torch.is_grad_enabled():
        return _DynamicSTE.apply(x, run)
    with torch.no_grad():
        return run(x.detach())


def vq_accumulate(x, codebook, granularity: str = "per_group", group_size: Optional[int] = 64, norm: Optional[float] = None, acc=None,
                  accumulate: bool = False, fused: Optional[bool] = None, per_group: Optional[int] = None):
    """The weighted k-means statistics of x under a [K, d] table (DESIGN.md §8 "Vector codebook casts"), float64 [K, d + 2] on the
    device: with scale s, quotients u and index idx formed exactly as vq_qdq forms them, over the vectors whose d quotients are all finite,
        A[idx, j] += w u_j;  A[idx, d] += w;  A[idx, d + 1] += 1,   w = (double)s * (double)s
    -- the true-MSE form: a vector's error is s^2 |u - c|^2, so the best row of a cell is A[k, :d] / A[k, d].  accumulate=True adds into
    `acc` (several tensors or batches under one table), else `acc` (or a fresh tensor) is overwritten.  ONE pass over x plus a fold launch
    (dmxq_vq_accumulate: no floating-point atomics, a fixed order, the same input gives the same bits) where vq_qdq's kernel applies;
    otherwise the chain's (s, u, idx) and torch index_add_.  fused: as vq_qdq.  Nothing is read back to the host."""
    granularity, group_size = _codebook_per_group(granularity, group_size, per_group, "vq_accumulate")
    table, K, d, granularity, group_size, norm = vq_check(codebook, None, granularity, group_size, norm, what="vq_accumulate")
    S = _vq_segment(x, d, granularity, group_size, "vq_accumulate")
    if acc is not None and (acc.dtype != torch.float64 or tuple(acc.shape) != (K, d + 2) or not acc.is_contiguous()):
        raise ValueError(f"vq_accumulate: acc must be a contiguous float64 [{K}, {d + 2}] tensor on x's device")
    if accumulate and acc is None:
        raise ValueError("vq_accumulate: accumulate=True needs acc")
    require_gpu(x, "vq_accumulate")
    if acc is not None and acc.device != x.device:
        raise ValueError(f"vq_accumulate: acc must be a contiguous float64 [{K}, {d + 2}] tensor on x's device")
    mode = _DYNF_GROUP if granularity == "per_group" else _DYNF_ROWS
    with torch.no_grad():
        xd = x.detach()
        xc = xd if xd.is_contiguous() else xd.contiguous()
        if acc is None:
            acc = torch.zeros(K, d + 2, dtype=torch.float64, device=xc.device)
        elif not accumulate and xc.numel() == 0:
            acc.zero_()
        if xc.numel() == 0:
            return acc
        c = _vq_tensor(table, xc.device)
        if fused is not False:
            cls = _vq_kernel_class(xc, S, d, K, mode)
            if cls is None and fused:
                raise NotImplementedError(f"vq_accumulate: no fused kernel for {granularity} segments of {S} {xc.dtype} elements with a "
                                          f"[{K}, {d}] table (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in VQ_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    _ops.vq_accumulate(xc, mode, S, c, 0.0 if norm is None else norm, acc, bool(accumulate))
                    _vq_accumulate_routes["fused"] += 1
                    return acc
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _vq_accumulate_routes["chain"] += 1
        _, sc, u, idx = _vq_chain(xc.reshape(-1, S), c, _vq_norm_tensor(c, norm), False)
        uv = u.reshape(-1, d)
        fin = torch.isfinite(uv).all(dim=1, keepdim=True)
        w = (sc.double() * sc.double())[:, None].expand(-1, S // d).reshape(-1, 1)
        zero = torch.zeros((), dtype=torch.float64, device=xc.device)
        terms = torch.cat([torch.where(fin, w * uv.double(), zero), torch.where(fin, w, zero), fin.double()], dim=1)
        # index_add_ adds with atomics: onto K rows alone every vector meets every other one, so the rows are kept in R copies, vector i
        # adding to copy i mod R, and the copies are summed (codebook_accumulate's form; R shrinks with K to bound the copies)
        n = uv.shape[0]
        R = max(1, min(_CODEBOOK_ACC_REPLICAS, 65536 // K, n))
        rows = idx.reshape(-1) + K * (torch.arange(n, device=xc.device) % R)
        A = torch.zeros(R * K, d + 2, dtype=torch.float64, device=xc.device).index_add_(0, rows, terms).reshape(R, K, d + 2).sum(dim=0)
        if accumulate:
            acc += A
        else:
            acc.copy_(A)
        return acc


def _vq_update(c, A):
    """the k-means update of the table from the statistics: c_k <- float(A[k, :d] / A[k, d]) where A[k, d + 1] > 0, else c_k stays"""
    d = c.shape[1]
    return torch.where(A[:, d + 1:d + 2] > 0, (A[:, :d] / A[:, d:d + 1]).float(), c)


def _vq_sample_init(x, K, d, granularity, group_size, norm):
    """the deterministic sample init: row i = the quotient vector number floor((2 i + 1) n / (2 K)) of x (u under `norm`), n vectors in all"""
    S = _vq_segment(x, d, granularity, group_size, "vq_fit")
    xd = x.detach()
    xc = xd if xd.is_contiguous() else xd.contiguous()
    x2 = xc.reshape(-1, S)
    norm_t = torch.full((1,), norm, dtype=torch.float32, device=xc.device)

    def quotients(part):
        mn, mx = _ops.group_minmax(part, 0, 1)
        return _ops.scale_channels(part, _scale_from_amax(torch.maximum(mn.abs(), mx.abs()), norm_t, False), 0, True, torch.float32)

    if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
        u = quotients(x2)
    else:
        u = torch.cat([quotients(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)])
    uv = u.reshape(-1, d)
    n = uv.shape[0]
    pick = torch.tensor([(2 * i + 1) * n // (2 * K) for i in range(K)], dtype=torch.int64).to(xc.device)
    return uv[pick].contiguous()


def vq_fit(x, K: Optional[int] = None, dim: Optional[int] = None, codebook=None, granularity: str = "per_group", group_size: Optional[int] = 64,
           norm: Optional[float] = None, iters: int = 8, return_history: bool = False, fused: Optional[bool] = None,
           per_group: Optional[int] = None):
    """Fits a [K, d] table to a tensor (or a list of tensors sharing it) by weighted k-means iterations on the device (DESIGN.md §8
    "Vector codebook casts") -> (table float32 [K, d] on the device, norm) or (table, norm, history).  Every iteration: A = vq_accumulate
    over the tensors, then c_k <- float(A[k, :d] / A[k, d]) where A[k, d + 1] > 0 (an empty row keeps its value) -- the minimiser of the
    true squared error sum s^2 |u - c|^2 over every cell.  The update is torch on the [K, d] table on the device: no host synchronisation
    inside the loop, an iteration is capturable.  The start: `codebook` when one is given (K, dim: None or its shape); otherwise the
    deterministic sample init -- with n quotient vectors in the FIRST tensor, row i is vector number floor((2 i + 1) n / (2 K)) of it, u
    under the fit's norm.  `norm` stays FIXED across the iterations and is returned -- pass it when casting with the fitted table: the
    given one; else 1.0 for the sample init; else resolved ONCE from the given table, max |c_kj| (the one read of a device table, before
    the loop).  return_history: the relative L2 error sqrt(sum_sq_err / sum_sq_ref) (ops.error_stats rows) before every iteration and
    after the last, float64 [iters + 1] on the device."""
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    if not xs:
        raise ValueError("vq_fit: no tensor to fit the table to")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"vq_fit: iters must be a non-negative integer, got {iters!r}")
    granularity, group_size = _codebook_per_group(granularity, group_size, per_group, "vq_fit")
    if codebook is None:
        if isinstance(K, bool) or not isinstance(K, int) or not 2 <= K <= 256:
            raise ValueError(f"vq_fit: without a codebook K must be an integer from 2 to 256, got {K!r}")
        if isinstance(dim, bool) or not isinstance(dim, int) or dim not in VQ_DIMS:
            raise ValueError(f"vq_fit: without a codebook dim must be one of {VQ_DIMS}, got {dim!r}")
        # (the remaining arguments are checked against a stand-in table of the same shape)
        _, _, d, granularity, group_size, norm = vq_check([[0.0] * dim] * K, dim, granularity, group_size, norm, what="vq_fit")
        table = None
        norm = 1.0 if norm is None else norm
    else:
        table, Kc, d, granularity, group_size, norm = vq_check(codebook, dim, granularity, group_size, norm, what="vq_fit")
        if K is not None and K != Kc:
            raise ValueError(f"vq_fit: K={K!r} beside a codebook of {Kc} rows")
        K = Kc
    for t in xs:
        _vq_segment(t, d, granularity, group_size, "vq_fit")
        require_gpu(t, "vq_fit")
    if xs[0].numel() // d < 1 and table is None:
        raise ValueError("vq_fit: the sample init needs a non-empty first tensor")
    if norm is None:
        norm = float(table.detach().abs().max().float()) if isinstance(table, torch.Tensor) else max(abs(v) for r in table for v in r)
        norm = float(torch.tensor(norm, dtype=torch.float32))
        if not (0.0 < norm < math.inf):
            raise ValueError(f"vq_fit: the initial table gives norm {norm!r}; pass a positive finite norm")
    with torch.no_grad():
        c = _vq_tensor(table, xs[0].device).clone() if table is not None else _vq_sample_init(xs[0], K, d, granularity, group_size, norm)

        def rel_error():
            row = None
            for t in xs:
                y = vq_qdq(t.detach(), c, granularity, group_size, norm, fused=fused)
                row = error_stats(t.detach(), y, out=row, accumulate=row is not None)
            return torch.sqrt(row[0] / row[1])

        history = []
        for _ in range(iters):
            if return_history:
                history.append(rel_error())
            A = torch.zeros(K, d + 2, dtype=torch.float64, device=c.device)
            for t in xs:
                vq_accumulate(t, c, granularity, group_size, norm, acc=A, accumulate=True, fused=fused)
            c = _vq_update(c, A)
        if return_history:
            history.append(rel_error())
            return c, norm, torch.stack(history)
        return c, norm


# ---------------------------------------------------------------------------------------------------- HQQ
# Group classes of dmxq_hqq_qdq (hqq_class) that fused=None sends to the chain of torch operations although the kernel takes them:
# DYNAMIC_CHAIN_BY_DEFAULT's rule -- a class goes to the kernel by default only where tools/bench_hqq.py MEASURED it faster than the chain
# on the same buffers; a class that is not gets listed here with its row.  profiles/r21_hqq.txt (bf16 XP[4,0], lp_norm 0.5, us per call,
# kernel against chain at iters = 20 and at iters = 0): group (64) [4096,4096] 428.9 against 24721.9 and 27.9 against 2449.9, [14336,4096]
# 1478.6 against 86934.0 and 78.2 against 8513.7, [2048,768] 43.6 against 2721.2 and 4.8 against 252.8; group (128) [4096,4096] 429.7
# against 16814.0 and 29.2 against 1403.5, [14336,4096] 1494.4 against 58455.9 and 76.1 against 4898.4, [2048,768] 43.8 against 2767.8 and
# 4.4 against 197.2 -- every row is faster (39 - 109 x), the class is not listed.
HQQ_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_hqq_routes = {"fused": 0, "chain": 0}
HQQ_KERNEL_NORMS = (0.5, 1.0)   # the l_p norms dmxq_hqq_qdq takes: their shrink needs no pow


def hqq_check(fmt, group_size=64, lp_norm=0.5, beta=10.0, kappa=1.01, iters=20, what: str = "hqq_qdq"):
    """-> (format, group_size, lp_norm, beta, kappa, iters) of an HQQ call, or ValueError: a clamped fraction-free FixedPoint format
    with nearest rounding (observer.get_qmin_qmax gives its integer range), a positive integer group size, lp_norm in (0, 1], a finite
    beta > 0, a finite kappa >= 1, an integer iters >= 0.  No GPU involved."""
    from .format import Format
    from .observer import get_qmin_qmax
    fmt = Format.from_shorthand(fmt) if isinstance(fmt, str) else fmt
    if not isinstance(fmt, Format) or get_qmin_qmax(fmt) == (None, None):
        raise ValueError(f"{what}: HQQ solves the zero point of an integer grid, so it needs a clamped FixedPoint format without fraction "
                         f"bits (XP[p,0](C..)), got {fmt!r}")
    if fmt.rounding != "nearest":
        raise ValueError(f"{what}: the definition rounds to nearest, got a format with {fmt.rounding!r} rounding: {fmt!r}")
    if isinstance(group_size, bool) or not isinstance(group_size, int) or group_size < 1:
        raise ValueError(f"{what}: group_size must be a positive integer, got {group_size!r}")

    def real(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
        return float(v)

    lp_norm, beta, kappa = real(lp_norm, "lp_norm"), real(beta, "beta"), real(kappa, "kappa")
    if not 0.0 < lp_norm <= 1.0:
        raise ValueError(f"{what}: lp_norm must lie in (0, 1], got {lp_norm!r}")
    if not beta > 0.0:
        raise ValueError(f"{what}: beta must be positive, got {beta!r}")
    if not kappa >= 1.0:
        raise ValueError(f"{what}: kappa must be at least 1, got {kappa!r}")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"{what}: iters must be a non-negative integer, got {iters!r}")
    return fmt, group_size, lp_norm, beta, kappa, iters


def hqq_class(group_size: int, dtype: torch.dtype) -> Optional[str]:
    """"group" where dmxq_hqq_qdq takes groups of `group_size` elements of `dtype` (a power of two from 16 to 256, whole 16-byte vectors
    in adjacent lanes of a wave), None where it refuses them; asked of the library itself (dmxq_hqq_class; no GPU involved)"""
    from ._lib import dtype_code, lib
    return _DYNAMIC_CLASS_NAMES.get(lib().dmxq_hqq_class(dtype_code(dtype), int(group_size)))


def _hqq_tree_sum(v):
    """the adjacent-pair tree over the last dim (an odd length carries its last value up unchanged)"""
    while v.shape[-1] > 1:
        n = v.shape[-1]
        h = v[..., 0:n - 1:2] + v[..., 1::2]
        v = torch.cat([h, v[..., -1:]], -1) if n % 2 else h
    return v[..., 0]


def _hqq_betas(beta, kappa, iters):
    """(beta_k, 1 / beta_k) for k < iters as Python floats holding float32 values: float32 products and IEEE float32 quotients,
    formed on the host (they depend on the arguments alone)"""
    import numpy as np
    b, k, out = np.float32(beta), np.float32(kappa), []
    for _ in range(iters):
        out.append((float(b), float(np.float32(1.0) / b)))
        b = np.float32(b * k)
    return out


def _hqq_chain(part, qmin, qmax, lp_norm, beta, kappa, iters, out_dtype, want_codes):
    """DESIGN.md §8 "HQQ" on the rows of part [n, g] in torch operations -> (y [n, g], s [n], z_best [n], codes or None)"""
    import numpy as np
    n, g = part.shape
    dev = part.device
    mn, mx = _ops.group_minmax(part, 0, 1)
    W = part.float()
    s = _div_ieee(mx - mn, _one(qmax - qmin, dev))
    s = torch.where(_usable_scale(s), s, torch.ones_like(s))
    rs = _ops.scale_channels(torch.ones(n, 1, dtype=torch.float32, device=dev), s, 0, True, torch.float32).reshape(n)
    z = (_one(qmin, dev) - mn * rs)[:, None]
    s2, rs2 = s[:, None], rs[:, None]
    inv_g = float(np.float32(1.0 / g))
    betas = _hqq_betas(beta, kappa, iters)
    zb = eb = None
    for k in range(iters + 1):
        q = torch.clamp(torch.round(W * rs2 + z), qmin, qmax)
        d = W - (q - z) * s2
        a = d.abs()
        err = _hqq_tree_sum(a)[:, None]
        if k == 0:
            zb, eb = z, err
        else:
            better = err < eb
            zb, eb = torch.where(better, z, zb), torch.where(better, err, eb)
        if k == iters:
            break
        ib = betas[k][1]
        if lp_norm == 1.0:
            m = a - ib
        elif lp_norm == 0.5:
            m = a - torch.full_like(a, ib) / a.sqrt()
        else:   # (torch.pow: not pinned to the bit)
            m = a - a.pow(lp_norm - 1.0) * ib
        e = torch.copysign(torch.clamp(m, min=0), d)
        z = _hqq_tree_sum(q - (W - e) * rs2)[:, None] * inv_g
    q = torch.clamp(torch.round(W * rs2 + zb), qmin, qmax)
    y = ((q - zb) * s2).to(out_dtype)
    codes = torch.where(q == q, q - qmin, torch.zeros_like(q)).to(torch.uint8) if want_codes else None
    return y, s, zb.reshape(n), codes


def hqq_qdq(x, fmt, group_size: int = 64, lp_norm: float = 0.5, beta: float = 10.0, kappa: float = 1.01, iters: int = 20,
            out_dtype: Optional[torch.dtype] = None, return_qparams: bool = False, return_codes: bool = False, fused: Optional[bool] = None):
    """Half-Quadratic Quantization (HQQ; Badri and Shaji, 2023; DESIGN.md §8 "HQQ", whose text is the contract; not in the reference): a
    calibration-free integer Q->DQ of a weight.  Every group of `group_size` consecutive elements of the last dim keeps the min/max
    scale of ops.dynamic_fixed_qdq and re-solves its float ZERO POINT with `iters` proximal steps under the l_p norm, beta_k = beta *
    kappa^k, keeping the zero point whose summed |x - y| over the group was smallest: iters=0 is round-to-nearest on the min/max grid with
    a float zero point, and no group's L1 error ever exceeds that one's.  Best-tracking is per group (upstream stops on a whole-tensor mean,
    a host round trip per iteration).
    lp_norm defaults to 0.5, not upstream's 0.7: at p = 0.5 the shrink is a square root and a division, both correctly rounded on every
    device and host, so the kernel, the chain and a CPU reference agree to the bit; a general p needs pow, which differs between math
    libraries (ops.smoothquant_scale's exponent has the same problem).  p = 1 needs neither.
    ONE launch (dmxq_hqq_qdq: load a group once, iterate in registers, store once) for group_size a power of two from 16 to 256,
    lp_norm 0.5 or 1, out_dtype == x.dtype and a 16-byte aligned tensor.  Otherwise the chain -- the definition in torch operations on
    the device, with the library's own launches where torch would not give the bits (group_minmax, IEEE divisions through
    scale_channels) -- same bits for lp_norm 0.5 and 1, and NOT pinned to the bit for any other lp_norm (torch.pow); on more than 65535
    groups it runs on pieces of 32768.  fused=None: the kernel where it applies and its class (hqq_class) is not listed in
    HQQ_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.
    Returns y, followed by (scale, zero), float32 [n_groups], with return_qparams and codes = q - qmin (uint8, x's shape, formats of up
    to 8 bits; 0 where q is NaN) with return_codes: y == ((codes + qmin) - zero) * scale in float32, rounded once to out_dtype.
    ValueError (before any GPU use): hqq_check's, a group size that does not divide the last dim, codes of a wider format.  Autograd:
    a straight-through estimator.  Nothing is read back to the host on either route: capturable."""
    from .observer import get_qmin_qmax
    fmt, group_size, lp_norm, beta, kappa, iters = hqq_check(fmt, group_size, lp_norm, beta, kappa, iters)
    if x.dim() < 1:
        raise ValueError("hqq_qdq: expects a tensor with at least one dimension")
    if x.shape[-1] % group_size:
        raise ValueError(f"hqq_qdq: the last dimension has {x.shape[-1]} elements, not a multiple of the group size {group_size}")
    qmin, qmax = get_qmin_qmax(fmt)
    if return_codes and qmax - qmin > 255:
        raise ValueError(f"hqq_qdq: uint8 codes hold formats of up to 8 bits, got {fmt!r}")
    require_gpu(x, "hqq_qdq")
    out_dtype = out_dtype or x.dtype
    g = group_size

    def pick(y, sc, zero, codes):
        out = (y,) + ((sc, zero) if return_qparams else ()) + ((codes,) if return_codes else ())
        return out if len(out) > 1 else y

    def run(xd):
        xc = xd if xd.is_contiguous() else xd.contiguous()
        if xc.numel() == 0:
            e = torch.empty(0, dtype=torch.float32, device=xc.device)
            return pick(torch.empty(xc.shape, dtype=out_dtype, device=xc.device), e, e.clone(),
                        torch.empty(xc.shape, dtype=torch.uint8, device=xc.device))
        if fused is not False:
            cls = hqq_class(g, xc.dtype) if (lp_norm in HQQ_KERNEL_NORMS and out_dtype == xc.dtype and fmt.precision <= 22
                                             and xc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"hqq_qdq: no fused kernel for groups of {g} {xc.dtype} elements -> {out_dtype} with {fmt!r} and "
                                          f"lp_norm {lp_norm} (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in HQQ_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    y, sc, zero, codes = _ops.hqq_qdq(xc, g, ROUNDING_CODE[fmt.rounding], qmin, qmax, lp_norm, beta, kappa, iters,
                                                      bool(return_qparams), bool(return_codes), out_dtype)
                    _hqq_routes["fused"] += 1
                    return pick(y, sc, zero, codes)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _hqq_routes["chain"] += 1
        x2 = xc.reshape(-1, g)

        def chain(part):
            return _hqq_chain(part, qmin, qmax, lp_norm, beta, kappa, iters, out_dtype, return_codes)

        if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
            y, sc, zero, codes = chain(x2)
        else:   # (dmxq_group_minmax takes 65535 groups: groups are independent, so the chain runs on pieces and the results are joined)
            parts = [chain(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)]
            y, sc, zero = (torch.cat([p[k] for p in parts]) for k in range(3))
            codes = torch.cat([p[3] for p in parts]) if return_codes else None
        return pick(y.reshape(xc.shape), sc, zero, codes.reshape(xc.shape) if return_codes else None)

    if x.requires_grad and torch.is_grad_enabled():
        return _DynamicSTE.apply(x, run)
    with torch.no_grad():
        return run(x.detach())


# ---------------------------------------------------------------------------------------------------- outlier-aware dynamic cast
# Group classes of dmxq_outlier_fixed_qdq (outlier_class) that fused=None sends to the chain although the kernel takes them:
# DYNAMIC_CHAIN_BY_DEFAULT's rule -- a class goes to the kernel by default only where tools/bench_outlier.py MEASURED it faster than the
# chain on the same buffers; a class that is not gets listed here with its row.  profiles/r22_outlier.txt (bf16 XP[4,0] affine, us per call,
# kernel at k = 1 / 2 / 4 against chain at k = 1 / 2 / 4): group (64) [4096,4096] 26.3 / 29.4 / 32.7 against 1373.7 / 1373.6 / 1373.4,
# [14336,4096] 80.2 / 87.5 / 100.8 against 4751.4 / 4743.8 / 4747.9, [2048,768] 5.8 / 5.2 / 5.4 against 175.6 / 176.9 / 176.7; group (128)
# [4096,4096] 26.2 / 29.5 / 33.0 against 778.6 / 782.6 / 782.0, [14336,4096] 80.0 / 89.4 / 99.4 against 2680.5 / 2681.4 / 2679.1, [2048,768]
# 5.7 / 5.1 / 5.5 against 121.0 / 121.2 / 121.7 -- every row is faster (21 - 59 x), the class is not listed.
OUTLIER_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_outlier_routes = {"fused": 0, "chain": 0}
OUTLIER_KERNEL_MAX_K = 8   # the most outliers per group dmxq_outlier_fixed_qdq selects in registers (the chain: any k < S)
OUTLIER_GRANULARITIES = ("per_group", "per_token")


def outlier_check(fmt, group_size, k, outlier_format=None, granularity="per_group", what: str = "outlier_fixed_qdq"):
    """-> (format, group_size, k, outlier_format) of an outlier-aware cast, or ValueError: dynamic_check's format rule (a clamped
    FixedPoint format without fraction bits), granularity "per_group" with a positive integer group size or "per_token" with none, an
    integer k with 0 <= k (and k < group_size where the group size is given; the row length is checked with the tensor), an
    outlier_format that is None or a FloatingPoint format with fewer than 23 mantissa bits.  No GPU involved."""
    from .format import FloatingPoint, Format
    if granularity not in OUTLIER_GRANULARITIES:
        raise ValueError(f"{what}: granularity must be one of {OUTLIER_GRANULARITIES}, got {granularity!r}")
    fmt, _, group_size = dynamic_check(fmt, granularity, group_size, what)
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError(f"{what}: k must be a non-negative integer, got {k!r}")
    if group_size is not None and k >= group_size:
        raise ValueError(f"{what}: k must be smaller than the segment, got k = {k} with segments of {group_size}")
    if outlier_format is not None:
        outlier_format = Format.from_shorthand(outlier_format) if isinstance(outlier_format, str) else outlier_format
        if not isinstance(outlier_format, FloatingPoint):
            raise ValueError(f"{what}: outlier_format must be None (the value itself) or a per-element FloatingPoint format, got "
                             f"{outlier_format!r}")
        if outlier_format.mantissa > 22:
            raise ValueError(f"{what}: a 23-bit mantissa through float_qdq is undefined, got {outlier_format!r}; pass None for the value itself")
    return fmt, group_size, k, outlier_format


def outlier_class(group_size: int, dtype: torch.dtype) -> Optional[str]:
    """"group" where dmxq_outlier_fixed_qdq takes groups of `group_size` elements of `dtype` (dynamic_class's group rule: a power of
    two from 16 to 256, whole 16-byte vectors in adjacent lanes of a wave), None where it refuses them; asked of the library itself
    (dmxq_outlier_class; no GPU involved)"""
    from ._lib import dtype_code, lib
    return _DYNAMIC_CLASS_NAMES.get(lib().dmxq_outlier_class(dtype_code(dtype), int(group_size)))


def outlier_bits_per_element(fmt, group_size: int, k: int, outlier_bits: int = 16, scale_bits: int = 16, zero_point_bits: Optional[int] = None,
                             symmetric_qscheme: bool = False) -> float:
    """the storage cost of the outlier-aware cast in bits per element: p + (scale_bits + zp_bits + k (outlier_bits + ceil(log2 S))) / S
    for a p-bit format on segments of S = group_size elements -- per segment one scale, one zero point and k (value, position) pairs.
    zero_point_bits defaults to p under an affine scheme and to 0 under a symmetric one.  XP[4,0] affine, S = 128, k = 2:
    4 + (16 + 4 + 2 * 23) / 128.  A host helper: what a user compares k against a wider format with."""
    fmt, group_size, k, _ = outlier_check(fmt, group_size, k, None, "per_group", "outlier_bits_per_element")
    p = int(fmt.precision)
    zp_bits = (0 if symmetric_qscheme else p) if zero_point_bits is None else int(zero_point_bits)
    pos_bits = (group_size - 1).bit_length()   # ceil(log2 S)
    return p + (int(scale_bits) + zp_bits + k * (int(outlier_bits) + pos_bits)) / group_size


def outlier_fixed_qdq(x, fmt, group_size: Optional[int] = None, k: int = 0, symmetric_qscheme: bool = False, outlier_format=None,
                      granularity: str = "per_group", out_dtype: Optional[torch.dtype] = None, return_qparams: bool = False,
                      return_outliers: bool = False, fused: Optional[bool] = None):
    """Outlier-aware dynamic integer Q->DQ (DESIGN.md §8 "Outlier-aware dynamic cast", whose text is the contract; SpQR, Dettmers et al.
    2023; SqueezeLLM, Kim et al. 2023; not in the reference): every segment keeps its k largest magnitudes at higher precision and
    casts the rest on a range that no longer has to cover them.  A segment is S consecutive elements of the last dim of the contiguous
    tensor: `group_size` elements with "per_group" (it must divide the last dim), the row with "per_token".  With x2 = x.reshape(-1, S):
        key = x2.float().abs() viewed as int32 (a NaN ranks above Inf, Inf above every finite value); the outliers of a segment are the
        first k positions of torch.sort(key, dim=1, descending=True, stable=True): equal keys go to the lower index; mask is True there
        xin = where(mask, +0.0, x2);  y_in, sc, zp = dynamic_fixed_qdq(xin, fmt, "per_token", symmetric_qscheme, return_qparams=True)
        (qparams take min(mn, 0) and max(mx, 0), so the zeros give exactly the qparams of the inliers alone; NaN / Inf beyond the k
        outliers follow dynamic_fixed_qdq's rule)
        y = where(mask, O(x2), y_in):  O(v) = v itself for outlier_format None (the same bits when out_dtype == x.dtype, .to(out_dtype)
        otherwise), ops.float_qdq(v, outlier_format...) for a per-element FloatingPoint format.
    k = 0 is dynamic_fixed_qdq itself on every route.
    ONE launch (dmxq_outlier_fixed_qdq: the selection runs in registers, k rounds of an integer maximum over the group's lanes) for
    per_group with group_size a power of two from 16 to 256, 1 <= k <= 8, a nearest-rounding format, out_dtype == x.dtype, a 16-byte
    aligned tensor and outlier_format None or a signed nearest-rounding FloatingPoint format.  Otherwise the chain: the definition above in
    torch operations and library calls on the device, same bits.  fused=None: the kernel where it applies and its class (outlier_class) is
    not listed in OUTLIER_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.
    Returns y, followed by (scale float32 [n_seg], zero_point int64 [n_seg]) with return_qparams and (idx int32 [n_seg, k], val out_dtype
    [n_seg, k]) with return_outliers: the outliers' positions in their segment and O(x), in rank order; the same on both routes.
    ValueError (before any GPU use): outlier_check's, a k that is not smaller than the segment, a segment that does not divide the last
    dim.  Autograd: a straight-through estimator.  Nothing is read back to the host on either route."""
    from .observer import get_qmin_qmax
    fmt, group_size, k, ofmt = outlier_check(fmt, group_size, k, outlier_format, granularity)
    if x.dim() < 1:
        raise ValueError("outlier_fixed_qdq: expects a tensor with at least one dimension")
    L = x.shape[-1]
    if granularity == "per_group" and L % group_size:
        raise ValueError(f"outlier_fixed_qdq: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    S = group_size if granularity == "per_group" else L
    if k and k >= S:
        raise ValueError(f"outlier_fixed_qdq: k must be smaller than the segment, got k = {k} with segments of {S}")
    require_gpu(x, "outlier_fixed_qdq")
    qmin, qmax = get_qmin_qmax(fmt)
    sym = bool(symmetric_qscheme)
    out_dtype = out_dtype or x.dtype
    ofields = [] if ofmt is None else [ofmt.mantissa, ofmt.exponent, ofmt.bias, int(bool(ofmt.flush_subnormal))]
    okernel = ofmt is None or (ofmt.rounding == "nearest" and not ofmt.unsigned)

    def pick(y, sc, zp, idx, val):
        out = (y,) + ((sc, zp) if return_qparams else ()) + ((idx, val) if return_outliers else ())
        return out if len(out) > 1 else y

    def run(xd):
        xc = xd if xd.is_contiguous() else xd.contiguous()
        n_seg = xc.numel() // S if S else 0
        if xc.numel() == 0 or k == 0:   # (k = 0: the dynamic cast itself, by its own routing -- fused is passed on)
            idx = torch.empty((n_seg, k), dtype=torch.int32, device=xc.device)
            val = torch.empty((n_seg, k), dtype=out_dtype, device=xc.device)
            if xc.numel() == 0:
                y = torch.empty(xc.shape, dtype=out_dtype, device=xc.device)
                return pick(y, y.new_empty(0, dtype=torch.float32), y.new_empty(0, dtype=torch.int64), idx, val)
            y, sc, zp = dynamic_fixed_qdq(xc, fmt, granularity, group_size if granularity == "per_group" else None, sym, out_dtype, True, fused)
            return pick(y, sc, zp, idx, val)
        if fused is not False:
            cls = outlier_class(S, xc.dtype) if (granularity == "per_group" and k <= OUTLIER_KERNEL_MAX_K and okernel and fmt.rounding == "nearest"
                                                 and out_dtype == xc.dtype and fmt.precision <= 22 and xc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"outlier_fixed_qdq: no fused kernel for {granularity} segments of {S} {xc.dtype} elements -> "
                                          f"{out_dtype} with {fmt!r}, k = {k} and outlier format {ofmt!r} (base address "
                                          f"{xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in OUTLIER_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    y, sc, zp, idx, val = _ops.outlier_fixed_qdq(xc, S, k, fmt.precision, fmt.fraction, bool(fmt.clamp), bool(fmt.symmetric),
                                                                 ROUNDING_CODE[fmt.rounding], qmin, qmax, sym, ofields, bool(return_qparams),
                                                                 bool(return_outliers), out_dtype)
                    _outlier_routes["fused"] += 1
                    return pick(y, sc, zp, idx, val)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _outlier_routes["chain"] += 1
        x2 = xc.reshape(-1, S)
        key = x2.float().abs().view(torch.int32)
        order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :k]
        mask = torch.zeros(x2.shape, dtype=torch.bool, device=x2.device).scatter_(1, order, True)
        xin = torch.where(mask, torch.zeros((), dtype=x2.dtype, device=x2.device), x2)
        y_in, sc, zp = dynamic_fixed_qdq(xin, fmt, "per_token", None, sym, out_dtype, True)
        if ofmt is None:
            ox = x2 if out_dtype == x2.dtype else x2.to(out_dtype)
        else:
            ox = float_qdq(x2, ofmt.mantissa, ofmt.exponent, ofmt.bias, bool(ofmt.flush_subnormal), bool(ofmt.unsigned), ofmt.rounding, out_dtype)
        y = torch.where(mask, ox, y_in).reshape(xc.shape)
        return pick(y, sc, zp, order.to(torch.int32), ox.gather(1, order) if return_outliers else None)

    if x.requires_grad and torch.is_grad_enabled():
        return _DynamicSTE.apply(x, run)
    with torch.no_grad():
        return run(x.detach())


# ---------------------------------------------------------------------------------------------------- block-scaled float cast
# Group classes of dmxq_block_scaled_float_qdq (block_scaled_float_class) that fused=None sends to the chain although the kernel takes
# them: DYNAMIC_FLOAT_CHAIN_BY_DEFAULT's rule -- a class goes to the kernel by default only where tools/bench_block_scaled.py MEASURED it
# faster than the chain on the same buffers; a class that is not gets listed here with its row.  profiles/r18_block_scaled.txt:
# (bf16, E4M3 scale capped at 448, us per call, kernel against chain; a dynamic t is reduction plus cast): E2M1 g16 dynamic t [8192,4096]
# 82.3 against 14165.7; E2M1 g16 static t [8192,4096] 49.6 against 14127.0; E4M3 g128 dynamic t [8192,4096] 66.5 against 2129.7; E4M3 g128
# static t [8192,4096] 34.1 against 2104.1; E2M1 g16 dynamic t [8192,14336] 194.2 against 49487.9; E2M1 g16 static t [8192,14336] 101.5
# against 49406.3; E4M3 g128 dynamic t [8192,14336] 179.3 against 7376.7; E4M3 g128 static t [8192,14336] 100.6 against 7360.4; E2M1 g16
# dynamic t [2048,768] 11.4 against 712.2; E2M1 g16 static t [2048,768] 4.0 against 696.1; E4M3 g128 dynamic t [2048,768] 11.6 against
# 177.0; E4M3 g128 static t [2048,768] 4.0 against 159.0 -- every row is faster, the class is not listed.
BLOCK_SCALED_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_block_scaled_routes = {"fused": 0, "chain": 0}
#: the ready setting of CastTo.set_scaling / ops.block_scaled_float_qdq for format FP[1|2|1,1](_N): E2M1 elements in groups of 16, an E4M3
#: group scale capped at 448 (the OCP E4M3FN code range; the library's FP[1|4|3,7] reaches 480), one float32 scale per tensor
NVFP4 = {"per_group": 16, "scale_format": "FP[1|4|3,7](_N)", "scale_max": 448.0, "tensor_scale": "dynamic"}


def block_scaled_check(fmt, group_size, scale_format, scale_max=None, tensor_scale="dynamic", what: str = "block_scaled_float_qdq"):
    """-> (format, scale format, scale_max) of a block-scaled cast, or ValueError: an element format dynamic_float_check accepts per group;
    a FloatingPoint scale format with fewer than 8 exponent bits and nearest rounding; 0 < scale_max <= the scale format's largest value
    (the default); tensor_scale "dynamic", None, a float or a one-element tensor.  No GPU involved."""
    from .format import FloatingPoint, Format
    fmt, _, _ = dynamic_float_check(fmt, "per_group", group_size, what=what)
    sf = Format.from_shorthand(scale_format) if isinstance(scale_format, str) else scale_format
    if not isinstance(sf, FloatingPoint):
        raise ValueError(f"{what}: the group scales are quantised to a float format, so scale_format must be a FloatingPoint format "
                         f"(FP[1|e|m,bias]), got {scale_format!r}")
    if sf.exponent >= 8:
        raise ValueError(f"{what}: a scale format with {sf.exponent} exponent bits has fp32's range and no largest value to cap the scale "
                         f"codes at, got {sf!r}; use ops.dynamic_float_qdq for float32 scales")
    if sf.rounding != "nearest":
        raise ValueError(f"{what}: the scale format must round to nearest, got {sf!r}")
    sfmax = dynamic_float_fmax(sf)
    if scale_max is None:
        scale_max = sfmax
    if isinstance(scale_max, bool) or not isinstance(scale_max, (int, float)) or not (0.0 < float(scale_max) <= sfmax):
        raise ValueError(f"{what}: scale_max must be a number in (0, {sfmax:g}] (the largest value of {sf!r}), got {scale_max!r}")
    if not (tensor_scale is None or (isinstance(tensor_scale, str) and tensor_scale == "dynamic")
            or (isinstance(tensor_scale, (int, float)) and not isinstance(tensor_scale, bool))
            or (isinstance(tensor_scale, torch.Tensor) and tensor_scale.numel() == 1)):
        raise ValueError(f"{what}: tensor_scale must be 'dynamic', None, a float or a one-element tensor, got {tensor_scale!r}")
    return fmt, sf, float(scale_max)


def block_scaled_float_class(group_size: int, dtype: torch.dtype) -> Optional[str]:
    """"group" where dmxq_block_scaled_float_qdq takes groups of `group_size` elements of `dtype` (a power of two from 16 to 256, in
    adjacent lanes of a wave), None where it refuses them; asked of the library itself (dmxq_block_scaled_float_class; no GPU involved)"""
    from ._lib import dtype_code, lib
    return _DYNAMIC_CLASS_NAMES.get(lib().dmxq_block_scaled_float_class(dtype_code(dtype), int(group_size)))


def _div_ieee(v, d):
    """v / d as an IEEE division of a float32 vector by ONE float32 on the device (through scale_channels: torch divides by a Python
    scalar as a multiplication by its reciprocal)"""
    n = v.numel()
    return _ops.scale_channels(v.reshape(n, 1), d.reshape(1), 1, True, torch.float32).reshape(n)


def _one(value, device):
    return torch.full((1,), float(value), dtype=torch.float32, device=device)


def _usable_scale(s):
    return torch.isfinite(s) & (s >= 2.0 ** -126)


def _bs_tensor_scale(xc, tensor_scale, fmax, scale_max, native=True):
    """step 1 of the definition -> float32 [1] on xc's device, already 1 where it is not finite or below 2^-126.  The dynamic t: the
    library's own small reduction (dmxq_block_scaled_tensor_scale: three launches) where `native` and it takes the tensor (whole aligned
    16-byte vectors); else -- the chain -- dmxq_group_minmax's whole-tensor reduction (one group over everything: one NaN makes it NaN)
    and the two divisions as scale_channels launches.  A maximum is exact in any order: the same bits on both routes."""
    dev = xc.device
    if tensor_scale is None:
        return _one(1.0, dev)
    if isinstance(tensor_scale, str):
        if native:
            try:
                return _ops.block_scaled_tensor_scale(xc, fmax, scale_max)
            except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                pass
        mn, mx = _ops.group_minmax(xc.reshape(1, -1), 0, 1)
        t = _div_ieee(_div_ieee(torch.maximum(mn.abs(), mx.abs()), _one(fmax, dev)), _one(scale_max, dev))
    elif isinstance(tensor_scale, torch.Tensor):
        t = tensor_scale.detach().reshape(1)
    else:
        t = _one(tensor_scale, dev)
    return torch.where(_usable_scale(t), t, torch.ones_like(t))


def block_scaled_tensor_scale(x, fmt, scale_format, scale_max=None):
    """Step 1 of ops.block_scaled_float_qdq alone, for calibrating a static tensor scale: t = (max |x| / fmax) / scale_max (two IEEE
    divisions; 1 where that is not finite -- a NaN or Inf anywhere -- or below 2^-126), float32 [1] on x's device, never read back."""
    fmt, sf, scale_max = block_scaled_check(fmt, 16, scale_format, scale_max, what="block_scaled_tensor_scale")
    require_gpu(x, "block_scaled_tensor_scale")
    with torch.no_grad():
        xc = x.detach()
        xc = xc if xc.is_contiguous() else xc.contiguous()
        if xc.numel() == 0:
            return _one(1.0, xc.device)
        return _bs_tensor_scale(xc, "dynamic", dynamic_float_fmax(fmt), scale_max)


def block_scaled_float_qdq(x, fmt, group_size: int, scale_format, scale_max: Optional[float] = None, tensor_scale="dynamic",
                           out_dtype: Optional[torch.dtype] = None, return_scale: bool = False, fused: Optional[bool] = None,
                           seed: Optional[int] = None):
    """Low-bit float Q->DQ with a QUANTISED scale per group under one float32 scale per tensor (not in the reference): the
    numerics of a stored block-scaled format -- E2M1 in groups of 16 with an E4M3 scale ("NVFP4": ops.NVFP4), E4M3 with quantised group
    scales -- where ops.dynamic_float_qdq keeps every scale as a full float32 number.  `fmt`: the element format E, a signed
    FloatingPoint with fewer than 8 exponent bits and largest output fmax; `scale_format`: the scale format Sf, a FloatingPoint with fewer
    than 8 exponent bits, nearest rounding and largest output sfmax; 0 < scale_max <= sfmax (default sfmax) caps the scale code (448: an
    FP[1|4|3,7] scale stays inside the OCP E4M3FN codes); a group is `group_size` consecutive elements of the last dim, which it must
    divide.  In fp32:
        t  = the tensor scale: "dynamic" -- (max |x| / fmax) / scale_max over the whole tensor, two IEEE divisions, one NaN anywhere makes
             the maximum NaN; None -- 1; a float, or a one-element float32 tensor on x's device (never read back); in every case 1 where it
             is not finite or below 2^-126
        a  = max |x| over the group (one NaN makes it NaN);  c = (a / fmax) / t, two IEEE divisions
        sq = min(float_q_Sf(c), scale_max): the scale format's nearest cast, NaN / Inf saturating to sfmax -- never NaN
        s  = sq * t, one multiply;  usable when finite and >= 2^-126
        usable: y = float_q_E(x / s) * s -- IEEE quotient, the format's nearest cast (NaN / Inf saturate as in float_qdq), one multiply,
                one rounding to out_dtype;  else: y = a zero with the sign bit of float_q_E(x) and the reported s is 0 (an all-zero
                group, or one so far below the tensor's maximum that its scale code is 0: a stored format holds zeros there)
    The output holds no NaN.  ONE launch for the groups (dmxq_block_scaled_float_qdq) for nearest-rounding formats, out_dtype == x.dtype,
    a 16-byte aligned tensor and a group that is a power of two from 16 to 256; the dynamic t is the library's own small reduction in
    front (dmxq_block_scaled_tensor_scale: three launches; in the chain group_minmax over the whole tensor).  Otherwise the chain of existing launches, same bits: group_minmax ->
    max(|mn|, |mx|) -> scale_channels divisions by fmax and t -> float_qdq with Sf -> minimum, multiply, where -> scale_channels (divide,
    float32) -> float_qdq with E -> scale_channels (multiply, out_dtype), on pieces of 32768 groups above 65535.  fused=None: the kernel
    where it applies and its class is not listed in BLOCK_SCALED_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back;
    False: the chain.  seed: for a stochastic-rounding element format (the chain only).  return_scale: (y, scale, scale_code_value,
    tensor_scale) -- float32 [n_groups] s and sq, float32 [1] t -- on both routes.  ValueError (before any GPU use): a format that cannot be
    used, a scale_max out of range, a group_size that does not divide.  Autograd: a straight-through estimator.  Nothing is read back to
    the host."""
    fmt, sf, scale_max = block_scaled_check(fmt, group_size, scale_format, scale_max, tensor_scale)
    if x.dim() < 1:
        raise ValueError("block_scaled_float_qdq expects a tensor with at least 1 dimension")
    L, g = x.shape[-1], group_size
    if L % g:
        raise ValueError(f"block_scaled_float_qdq: the last dimension has {L} elements, not a multiple of the group size {g}")
    require_gpu(x, "block_scaled_float_qdq")
    if isinstance(tensor_scale, torch.Tensor) and (tensor_scale.device != x.device or tensor_scale.dtype != torch.float32):
        raise ValueError(f"block_scaled_float_qdq: a tensor_scale tensor must be float32 on the input's device, got {tensor_scale.dtype} on "
                         f"{tensor_scale.device}")
    out_dtype = out_dtype or x.dtype
    fmax = dynamic_float_fmax(fmt)
    fields = (fmt.mantissa, fmt.exponent, fmt.bias, bool(fmt.flush_subnormal))
    sfields = (sf.mantissa, sf.exponent, sf.bias, bool(sf.flush_subnormal))

    def run(xd):
        xc = xd if xd.is_contiguous() else xd.contiguous()
        dev = xc.device
        if xc.numel() == 0:
            y = torch.empty(xc.shape, dtype=out_dtype, device=dev)
            e = y.new_empty(0, dtype=torch.float32)
            return (y, e, e.clone(), _one(1.0, dev)) if return_scale else y
        cls = None
        if fused is not False:
            cls = block_scaled_float_class(g, xc.dtype) if (fmt.rounding == "nearest" and out_dtype == xc.dtype and fmt.mantissa <= 22
                                                            and sf.mantissa <= 22 and xc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"block_scaled_float_qdq: no fused kernel for groups of {g} {xc.dtype} elements -> {out_dtype} "
                                          f"with {fmt!r} under {sf!r} scales (base address {xc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in BLOCK_SCALED_CHAIN_BY_DEFAULT:
                cls = None
        if cls is not None:
            # an absent and a given t go to the kernel as they are (it applies the t = 1 rule itself) unless the caller wants to see t
            if not return_scale and (tensor_scale is None or isinstance(tensor_scale, torch.Tensor)):
                t = None if tensor_scale is None else tensor_scale.detach().reshape(1)
            else:
                t = _bs_tensor_scale(xc, tensor_scale, fmax, scale_max, True)
            try:
                y, sc, sq = _ops.block_scaled_float_qdq(xc, g, [*fields, ROUNDING_CODE[fmt.rounding]], [*sfields, ROUNDING_CODE["nearest"]],
                                                        scale_max, t, bool(return_scale), bool(return_scale), out_dtype)
                _block_scaled_routes["fused"] += 1
                return (y, sc, sq, t) if return_scale else y
            except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                if fused:
                    raise
        _block_scaled_routes["chain"] += 1
        t = _bs_tensor_scale(xc, tensor_scale, fmax, scale_max, False)
        x2 = xc.reshape(-1, g)
        fmax_t, smax_t = _one(fmax, dev), _one(scale_max, dev)

        def chain(part):
            mn, mx = _ops.group_minmax(part, 0, 1)
            c = _div_ieee(_div_ieee(torch.maximum(mn.abs(), mx.abs()), fmax_t), t)
            sq = torch.minimum(float_qdq(c, *sfields, False, "nearest", torch.float32), smax_t.expand_as(c))
            s = sq * t.expand_as(sq)
            ok = _usable_scale(s)
            s1 = torch.where(ok, s, torch.ones_like(s))
            q = _ops.scale_channels(part, s1, 0, True, torch.float32)
            q = float_qdq(q, *fields, False, fmt.rounding, torch.float32, seed)
            y = _ops.scale_channels(q, s1, 0, False, out_dtype)
            # an unusable group: zeros carrying the sign bit of float_q_E(x)
            z = float_qdq(part, *fields, False, fmt.rounding, torch.float32, seed)
            y = torch.where(ok[:, None], y, torch.copysign(torch.zeros_like(z), z).to(out_dtype))
            return y, torch.where(ok, s, torch.zeros_like(s)), sq

        if x2.shape[0] <= DYNAMIC_CHAIN_MAX_SEGMENTS:
            y, sc, sq = chain(x2)
        else:   # (dmxq_group_minmax takes 65535 groups: groups are independent once t is known, so the chain runs on pieces)
            parts = [chain(x2[i:i + DYNAMIC_CHAIN_PIECE]) for i in range(0, x2.shape[0], DYNAMIC_CHAIN_PIECE)]
            y, sc, sq = (torch.cat([p[k] for p in parts]) for k in range(3))
        y = y.reshape(xc.shape)
        return (y, sc, sq, t) if return_scale else y

    if x.requires_grad and torch.is_grad_enabled():
        return _DynamicSTE.apply(x, run)
    with torch.no_grad():
        return run(x.detach())


# ---------------------------------------------------------------------------------------------------- Wanda
# Geometries of dmxq_wanda_nm -- the group size M: 0 (score only), 4, 8, 16 -- that fused=None sends to the chain although the kernel
# takes them: DYNAMIC_FLOAT_CHAIN_BY_DEFAULT's rule, a class goes to the kernel by default only where tools/bench_wanda.py MEASURED it
# faster than the chain (wanda_score, then nm_sparsify) on the same buffers.  profiles/r16_wanda.txt (bf16, us per call, kernel against
# chain): y alone 2:4 [4096,4096] 18.6 against 46.6, 4:8 21.5 against 48.3, 2:4 [14336,4096] 51.2 against 151.5, 4:8 60.1 against 156.2;
# score + mask 46.0 against 46.6, 45.0 against 47.3, 153.7 against 156.2, 155.3 against 156.2 -- no row is slower, none is listed.
WANDA_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_wanda_routes = {"fused": 0, "chain": 0}
_sumsq_workspaces = {}   # (device, bytes) -> the workspace of channel_sumsq outside captures


def channel_sumsq_workspace_bytes(rows: int, C: int) -> int:
    """dmxq_channel_sumsq_workspace_bytes: what one channel_sumsq call over [rows, C] needs.  A host query of the library itself."""
    from ._lib import lib
    return int(lib().dmxq_channel_sumsq_workspace_bytes(int(rows), int(C)))


def _sumsq_workspace(device, nbytes):
    """The slabs' partial sums of one channel_sumsq call: kept per (device, size) between calls -- a calibration run calls with a handful
    of shapes, once per forward of every observed module, on one stream -- except under a hipGraph capture, where the graph's own pool
    has to own the memory its kernels write."""
    n = max(nbytes, 8)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n // 8 + 1, dtype=torch.float64, device=device)
    key = (device, n)
    ws = _sumsq_workspaces.get(key)
    if ws is None:
        ws = _sumsq_workspaces[key] = torch.empty(n // 8 + 1, dtype=torch.float64, device=device)
    return ws


def channel_sumsq(x, out=None):
    """Per-channel sum of squares of x over every dimension but the last, in float64 (dmxq_channel_sumsq_accumulate; DESIGN.md §8
    "Wanda"): a float64 [C] tensor on x's device, C = x.shape[-1]; with `out` the sums are ADDED into it (statistics over many batches)
    and it is returned.  Every square is formed in double and the sum takes a fixed order without atomics: the same batches in the same
    order give the same bits.  A non-contiguous x is made contiguous first.  Two launches, nothing read back: capturable."""
    require_gpu(x, "channel_sumsq")
    if x.dim() < 1:
        raise ValueError("channel_sumsq: x needs a channel dimension")
    C = x.shape[-1]
    if out is None:
        out = torch.zeros(C, dtype=torch.float64, device=x.device)
    elif not (out.is_cuda and out.device == x.device and out.dtype == torch.float64 and out.is_contiguous() and out.shape == (C,)):
        raise ValueError(f"channel_sumsq: out must be a contiguous float64 [{C}] tensor on the input's device")
    if x.numel() == 0:
        return out
    xd = x.detach()
    _ops.channel_sumsq(xd, out, _sumsq_workspace(x.device, channel_sumsq_workspace_bytes(x.numel() // C, C)))
    return out


def wanda_class(dtype: torch.dtype, L: int, M: int) -> bool:
    """whether dmxq_wanda_nm takes rows of L elements of `dtype` with groups of M (0: score only) in its one-pass kernel, asked of the
    library itself (dmxq_wanda_class; no GPU involved): M in {0, 4, 8, 16} and L a multiple of 16"""
    from ._lib import dtype_code, lib
    return bool(lib().dmxq_wanda_class(dtype_code(dtype), int(L), int(M)))


def _wanda_check(w, act_norm, K, M, what):
    """the argument errors of the Wanda ops, before any GPU use (ValueError / TypeError)"""
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        raise ValueError(f"{what}: the weight must be a [rows, L] matrix")
    if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: the weight must be float32, float16 or bfloat16, got {w.dtype}")
    L = w.shape[1]
    if not isinstance(act_norm, torch.Tensor) or act_norm.dtype != torch.float32:
        raise TypeError(f"{what}: act_norm must be a float32 tensor, got {getattr(act_norm, 'dtype', type(act_norm))}")
    if act_norm.shape != (L,):
        raise ValueError(f"{what}: act_norm must hold one entry per input channel, [{L}], got {tuple(act_norm.shape)}")
    if M or K:
        if isinstance(K, bool) or isinstance(M, bool) or not isinstance(K, int) or not isinstance(M, int) or M < 1 or M > 64 or K < 1:
            raise ValueError(f"{what}: K and M must be integers with 1 <= K <= M <= 64, got {K!r}:{M!r}")
        if K > M:
            raise ValueError(f"{what}: K = {K} non-zeros do not fit a group of M = {M}")
        if L % M:
            raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the group size {M}")


def _wanda(w, act_norm, K, M, want_score, want_mask, want_y, fused, out_dtype, what):
    _wanda_check(w, act_norm, K, M, what)
    if not (want_score or want_mask or want_y):
        raise ValueError(f"{what}: nothing to compute: none of score, mask and y was asked for")
    if not M and (want_mask or want_y):
        raise ValueError(f"{what}: K = M = 0 asks for the score alone; a mask or y needs a K:M pattern")
    require_gpu(w, what)
    require_gpu(act_norm, what)
    with torch.no_grad():
        wc = w.detach()
        wc = wc if wc.is_contiguous() else wc.contiguous()
        an = act_norm.detach()
        an = an if an.is_contiguous() else an.contiguous()
        y_dtype = out_dtype or torch.promote_types(wc.dtype, torch.float32)
        if wc.numel() == 0:
            e = lambda dt: torch.empty(wc.shape, dtype=dt, device=wc.device)
            return (e(torch.float32) if want_score else None, e(torch.float32) if want_mask else None, e(y_dtype) if want_y else None)
        if fused is not False:
            ok = wanda_class(wc.dtype, wc.shape[1], M) and wc.data_ptr() % 16 == 0 and an.data_ptr() % 16 == 0
            if not ok and fused:
                raise NotImplementedError(f"{what}: no one-pass kernel for groups of {M} in rows of {wc.shape[1]} {wc.dtype} elements "
                                          f"(weight base address {wc.data_ptr() % 16} mod 16)")
            if ok and fused is None and M in WANDA_CHAIN_BY_DEFAULT:
                ok = False
            if ok:
                try:
                    score, mask, y = _ops.wanda_nm(wc, an, int(K), int(M), bool(want_score), bool(want_mask), bool(want_y), None, y_dtype)
                    _wanda_routes["fused"] += 1
                    return (score if want_score else None), (mask if want_mask else None), (y if want_y else None)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _wanda_routes["chain"] += 1
        score = wc.float().abs() * an   # (the definition: one fp32 multiply per element)
        mask = y = None
        if want_mask or want_y:
            mask, y = _nm(score, wc if want_y else None, K, M, -1, want_mask, want_y, None, y_dtype if want_y else None)
        return (score if want_score else None), mask, y


def wanda_score(w, act_norm, fused: Optional[bool] = None):
    """The Wanda score of a [rows, L] weight (Sun et al., 2023): float32 |w| * act_norm, act_norm the float32 [L] vector of
    the input channels' activation norms (channel_sumsq(...).sqrt().float()).  One launch (dmxq_wanda_nm with K = M = 0) where L is a
    multiple of 16 and the tensors are 16-byte aligned, else the same multiply in torch; `fused` as in wanda_nm_sparsify."""
    return _wanda(w, act_norm, 0, 0, True, False, False, fused, None, "wanda_score")[0]


def wanda_nm_sparsify(w, act_norm, K: int, M: int, return_mask: bool = False, return_score: bool = False, fused: Optional[bool] = None,
                      out_dtype: Optional[torch.dtype] = None, return_y: bool = True):
    """N:M pruning of a [rows, L] weight by its Wanda score in ONE pass over the weight (dmxq_wanda_nm): by definition
        score = w.float().abs() * act_norm;   y, mask = nm_sparsify(w, score, K, M, -1, return_mask=True)
    bit for bit -- the K highest scores of every group of M along the last dim are kept (stable ascending rank, the lower index zeroed
    first among ties, NaN highest, -0 == +0), y = w * mask is a real multiply (a masked negative weight gives -0.0) in torch's promotion
    of (w.dtype, float32) unless out_dtype says otherwise, the mask is float32.  The score is formed in registers and only written when
    return_score asks for it.  Returns y, or the tuple (y, mask, score) of what was asked for, in that order; return_y=False leaves y out
    (mask and / or score alone).
    fused=None: the kernel where it applies (M in {4, 8, 16}, L a multiple of 16, 16-byte aligned tensors) and M is not listed in
    WANDA_CHAIN_BY_DEFAULT, else the chain above; True: NotImplementedError instead of falling back; False: the chain.
    ValueError / TypeError before any GPU use: K > M, a last dim that M does not divide, an act_norm of the wrong length or dtype,
    nothing asked for."""
    score, mask, y = _wanda(w, act_norm, K, M, bool(return_score), bool(return_mask), bool(return_y), fused, out_dtype, "wanda_nm_sparsify")
    out = tuple(t for t, want in ((y, return_y), (mask, return_mask), (score, return_score)) if want)
    return out[0] if len(out) == 1 else out


# ---------------------------------------------------------------------------------------------------- AWQ
# Group sizes of dmxq_awq_group_error that fused=None sends to the four-launch chain although the kernel takes them: WANDA_CHAIN_BY_DEFAULT's
# rule, a class goes to the kernel by default only where tools/bench_awq.py MEASURED it faster than the chain (scale_channels ->
# dynamic_fixed_qdq -> scale_channels to float32 -> the subtraction) on the same buffers.  profiles/r17_awq.txt (bf16 XP[4,0] g128, us per
# candidate, kernel against chain): [4096,4096] 32.0 against 93.5, [14336,4096] 95.3 against 327.2, [4096,14336] 90.4 against 325.3 -- no
# row is slower, none is listed.
AWQ_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_awq_routes = {"fused": 0, "chain": 0}
AWQ_SCALE_MIN = 1e-4   # the floor of a candidate scale before it is normalised


def channel_sumabs(x, out=None):
    """Per-channel sum of |x| over every dimension but the last, in float64 (dmxq_channel_sumabs_accumulate; DESIGN.md §8 "AWQ"): the
    twin of channel_sumsq -- the same kernel body with |x| as the term, the same workspace, slab partition and fixed order without
    atomics (the same batches in the same order give the same bits), `out` ADDED into and returned.  Two launches, nothing read back:
    capturable."""
    require_gpu(x, "channel_sumabs")
    if x.dim() < 1:
        raise ValueError("channel_sumabs: x needs a channel dimension")
    C = x.shape[-1]
    if out is None:
        out = torch.zeros(C, dtype=torch.float64, device=x.device)
    elif not (out.is_cuda and out.device == x.device and out.dtype == torch.float64 and out.is_contiguous() and out.shape == (C,)):
        raise ValueError(f"channel_sumabs: out must be a contiguous float64 [{C}] tensor on the input's device")
    if x.numel() == 0:
        return out
    _ops.channel_sumabs(x.detach(), out, _sumsq_workspace(x.device, channel_sumsq_workspace_bytes(x.numel() // C, C)))
    return out


def awq_class(dtype: torch.dtype, L: int, group: int) -> bool:
    """whether dmxq_awq_group_error takes rows of L elements of `dtype` with groups of `group` in its one-launch kernel, asked of the
    library itself (dmxq_awq_class; no GPU involved): group a power of two from 16 to 256 that divides L"""
    from ._lib import dtype_code, lib
    return bool(lib().dmxq_awq_class(dtype_code(dtype), int(L), int(group)))


def awq_candidate_scales(x_mean, n_grid: int, scale_cast=None):
    """The candidate scale vectors of an AWQ search (Lin et al., 2023): float32 [n_grid, in] on x_mean's device.  x_mean is
    the float32 [in] vector of the input channels' mean magnitudes; for k = 0 .. n_grid - 1 and r = k / n_grid
        s_k = clamp(x_mean ** r, min=1e-4);   s_k /= sqrt(max(s_k) * min(s_k));   s_k = scale_cast(s_k)
    in float32 torch arithmetic on the device (scale_cast: SmoothQuant's cast of its scale, or None).  Row 0 is exactly all ones: plain
    round-to-nearest.  Nothing is read back."""
    if isinstance(n_grid, bool) or not isinstance(n_grid, int) or n_grid < 1:
        raise ValueError(f"awq_candidate_scales: n_grid must be a positive integer, got {n_grid!r}")
    if not isinstance(x_mean, torch.Tensor) or x_mean.dim() != 1 or x_mean.dtype != torch.float32:
        raise ValueError("awq_candidate_scales: x_mean must be a float32 [in] vector")
    with torch.no_grad():
        rows = []
        for k in range(n_grid):
            s = x_mean.pow(k / n_grid).clamp(min=AWQ_SCALE_MIN)
            s = s / (s.max() * s.min()).sqrt()
            rows.append(scale_cast(s) if scale_cast is not None else s)
        return torch.stack(rows).to(torch.float32).contiguous()


def _awq_check(w, s, fmt, group_size, what):
    """the argument errors of the AWQ ops, before any GPU use (ValueError / TypeError)"""
    fmt, _, group_size = dynamic_check(fmt, "per_group", group_size, what=what)
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        raise ValueError(f"{what}: the weight must be an [out, in] matrix")
    if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: the weight must be float32, float16 or bfloat16, got {w.dtype}")
    L = w.shape[1]
    if not isinstance(s, torch.Tensor) or s.dtype != torch.float32:
        raise TypeError(f"{what}: s must be a float32 tensor, got {getattr(s, 'dtype', type(s))}")
    if s.shape != (L,):
        raise ValueError(f"{what}: s must hold one entry per input channel, [{L}], got {tuple(s.shape)}")
    if L % group_size:
        raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    return fmt, group_size


def awq_scaled_error(w, s, fmt, group_size: int, symmetric_qscheme: bool = False, return_wq: bool = False, fused: Optional[bool] = None):
    """The error of ONE AWQ candidate on an [out, in] weight: with the float32 [in] scale vector s, by definition
        ws = scale_channels(w, s, -1, divide=False, out_dtype=w.dtype)
        wq = dynamic_fixed_qdq(ws, fmt, "per_group", group_size, symmetric_qscheme)
        d  = scale_channels(wq, s, -1, divide=True, out_dtype=torch.float32) - w.float()
    -- the weight as the layer would hold it under SmoothQuant's scale s, cast by a per-group dynamic integer cast, brought back and
    compared: d = Q(w s) / s - w in float32.  Returns d, or (d, wq) with return_wq.
    ONE launch (dmxq_awq_group_error: 6 B per bf16 element, 8 with wq, against the chain's four launches and ~22 B) for a
    nearest-rounding format, group_size a power of two from 16 to 256 and 16-byte aligned tensors; the chain otherwise, same bits.
    fused=None: the kernel where it applies and group_size is not listed in AWQ_CHAIN_BY_DEFAULT; True: NotImplementedError instead of
    falling back; False: the chain.
    ValueError / TypeError before any GPU use: a format without an integer range, a group_size that does not divide the last dim, an s
    of the wrong length or dtype, a weight that is no matrix."""
    from .observer import get_qmin_qmax
    fmt, group_size = _awq_check(w, s, fmt, group_size, "awq_scaled_error")
    require_gpu(w, "awq_scaled_error")
    require_gpu(s, "awq_scaled_error")
    qmin, qmax = get_qmin_qmax(fmt)
    sym = bool(symmetric_qscheme)
    with torch.no_grad():
        wc = w.detach()
        wc = wc if wc.is_contiguous() else wc.contiguous()
        sc = s.detach()
        sc = sc if sc.is_contiguous() else sc.contiguous()
        if wc.numel() == 0:
            d = torch.empty(wc.shape, dtype=torch.float32, device=wc.device)
            return (d, torch.empty_like(wc)) if return_wq else d
        if fused is not False:
            ok = (fmt.rounding == "nearest" and fmt.precision <= 22 and awq_class(wc.dtype, wc.shape[1], group_size)
                  and wc.data_ptr() % 16 == 0 and sc.data_ptr() % 16 == 0)
            if not ok and fused:
                raise NotImplementedError(f"awq_scaled_error: no one-launch kernel for groups of {group_size} in rows of {wc.shape[1]} {wc.dtype} "
                                          f"elements with {fmt!r} (weight base address {wc.data_ptr() % 16} mod 16)")
            if ok and fused is None and group_size in AWQ_CHAIN_BY_DEFAULT:
                ok = False
            if ok:
                try:
                    d, wq = _ops.awq_group_error(wc, sc, int(group_size), fmt.precision, fmt.fraction, bool(fmt.clamp), bool(fmt.symmetric),
                                                 qmin, qmax, sym, bool(return_wq))
                    _awq_routes["fused"] += 1
                    return (d, wq) if return_wq else d
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _awq_routes["chain"] += 1
        ws = _ops.scale_channels(wc, sc, -1, False, wc.dtype)
        wq = dynamic_fixed_qdq(ws, fmt, "per_group", group_size, symmetric_qscheme=sym)
        d = _ops.scale_channels(wq, sc, -1, True, torch.float32) - wc.float()
        return (d, wq) if return_wq else d


class _full_fp32_matmul:
    """float32 GEMMs in full precision inside the block (no TF32 or other reduced-precision mode), the setting restored on exit"""

    def __enter__(self):
        self.prev = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False

    def __exit__(self, *exc):
        torch.backends.cuda.matmul.allow_tf32 = self.prev


def awq_search(w, gram, scales, error_fn):
    """The AWQ search over candidate scales: for every row s_k of `scales` (float32 [n_grid, in]) the error
    D_k = error_fn(k, s_k) (float32 [out, in]: Q(w s_k) / s_k - w, e.g. awq_scaled_error) is weighed by the calibration inputs' second
    moment `gram` (float32 [in, in], the mean of x^T x over the tokens):
        loss_k = sum((D_k @ gram) * D_k) / out        -- the mean squared output error over the calibration tokens
    with the GEMM in full float32 and the final sum in float64.  Returns (losses float64 [n_grid], best 0-d int64), both on the device:
    best is the argmin over the finite losses, 0 when none is finite.  Nothing is read back to the host.
    ValueError before any GPU use: shapes of w, gram and scales that do not belong together."""
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        raise ValueError("awq_search: the weight must be an [out, in] matrix")
    out_f, in_f = w.shape
    if not isinstance(gram, torch.Tensor) or gram.shape != (in_f, in_f) or gram.dtype != torch.float32:
        raise ValueError(f"awq_search: gram must be a float32 [{in_f}, {in_f}] matrix, got "
                         f"{getattr(gram, 'dtype', type(gram))} {tuple(getattr(gram, 'shape', ()))}")
    if not isinstance(scales, torch.Tensor) or scales.dim() != 2 or scales.shape[1] != in_f or scales.shape[0] < 1 or scales.dtype != torch.float32:
        raise ValueError(f"awq_search: scales must be a float32 [n_grid, {in_f}] matrix with at least one row, got "
                         f"{getattr(scales, 'dtype', type(scales))} {tuple(getattr(scales, 'shape', ()))}")
    if out_f < 1:
        raise ValueError("awq_search: the weight has no rows")
    require_gpu(w, "awq_search")
    require_gpu(gram, "awq_search")
    require_gpu(scales, "awq_search")
    with torch.no_grad(), _full_fp32_matmul():
        losses = torch.empty(scales.shape[0], dtype=torch.float64, device=w.device)
        for k in range(scales.shape[0]):
            d = error_fn(k, scales[k])
            if d.shape != w.shape or d.dtype != torch.float32:
                raise ValueError(f"awq_search: error_fn must return a float32 {tuple(w.shape)} tensor, got {d.dtype} {tuple(d.shape)}")
            losses[k] = ((d @ gram) * d).sum(dtype=torch.float64) / out_f
        finite = torch.isfinite(losses)
        best = torch.where(finite, losses, torch.full_like(losses, float("inf"))).argmin()
        best = torch.where(finite.any(), best, torch.zeros_like(best))
        return losses, best


# ---------------------------------------------------------------------------------------------------- AWQ clipping
# Group sizes of dmxq_awq_clip that fused=None sends to the chain although the kernel takes them: AWQ_CHAIN_BY_DEFAULT's rule, a class
# goes to the kernel by default only where tools/bench_awq_clip.py MEASURED it faster than the pinned chain on the same buffers
# (profiles/r23_awq_clip.txt).
AWQ_CLIP_CHAIN_BY_DEFAULT = frozenset()
AWQ_CLIP_MAX_RATIOS = 32
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_awq_clip_routes = {"fused": 0, "chain": 0}
_awq_clip_ratio_cache = {}   # (the ratios' bytes, device) -> the device copy: a capture replays without a host-to-device copy


def awq_clip_ratios(n_grid: int = 20, max_shrink: float = 0.5):
    """AutoAWQ's list of clipping ratios as a float32 CPU tensor: 1 - i / n_grid for i = 0 .. int(max_shrink * n_grid) - 1, each formed
    in double and rounded once to float32 (the defaults: 1.0, 0.95, .. 0.55).  ValueError: a list that would be empty or longer than 32."""
    if isinstance(n_grid, bool) or not isinstance(n_grid, int) or n_grid < 1:
        raise ValueError(f"awq_clip_ratios: n_grid must be a positive integer, got {n_grid!r}")
    if isinstance(max_shrink, bool) or not isinstance(max_shrink, (int, float)) or not 0.0 < max_shrink <= 1.0:
        raise ValueError(f"awq_clip_ratios: max_shrink must lie in (0, 1], got {max_shrink!r}")
    n = int(max_shrink * n_grid)
    if not 1 <= n <= AWQ_CLIP_MAX_RATIOS:
        raise ValueError(f"awq_clip_ratios: int(max_shrink * n_grid) must lie in 1 .. {AWQ_CLIP_MAX_RATIOS}, got {n}")
    return torch.tensor([1.0 - i / n_grid for i in range(n)], dtype=torch.float64).to(torch.float32)


def awq_gram_blocks(gram, g: int):
    """the float32 [L / g, g, g] diagonal blocks of a float32 [L, L] matrix, contiguous: blocks[k][j][l] = gram[k g + j][k g + l]"""
    if not isinstance(gram, torch.Tensor) or gram.dim() != 2 or gram.shape[0] != gram.shape[1] or gram.dtype != torch.float32:
        raise ValueError("awq_gram_blocks: gram must be a square float32 matrix")
    if isinstance(g, bool) or not isinstance(g, int) or g < 1 or gram.shape[0] % g:
        raise ValueError(f"awq_gram_blocks: the group size must be a positive integer dividing {gram.shape[0]}, got {g!r}")
    G = gram.shape[0] // g
    return gram.reshape(G, g, G, g).permute(1, 3, 0, 2).diagonal(dim1=2, dim2=3).permute(2, 0, 1).contiguous()


def awq_clip_class(dtype: torch.dtype, L: int, group: int) -> bool:
    """whether dmxq_awq_clip takes rows of L elements of `dtype` with groups of `group` in its one-launch kernel, asked of the library
    itself (dmxq_awq_clip_class; no GPU involved): group 16, 32, 64 or 128 dividing L"""
    from ._lib import dtype_code, lib
    return bool(lib().dmxq_awq_clip_class(dtype_code(dtype), int(L), int(group)))


def awq_clip_check(w, blocks, fmt, group_size, ratios=None, out=None, what: str = "awq_clip"):
    """-> (format, group_size, ratios) of an AWQ clip call, or the argument error (ValueError / TypeError), before any GPU use: a clamped
    fraction-free FixedPoint format with nearest rounding, a group size dividing the weight's columns, float32 [G, g, g] contiguous
    blocks, and ratios -- None (awq_clip_ratios()), a sequence or a float32 tensor of 1 .. 32 entries; held on the host they are checked
    (first entry 1.0, every entry in (0, 1], non-increasing) and come back as a float32 CPU tensor, a tensor on a device comes back as it
    is (its values are the caller's contract: reading them would synchronise)."""
    fmt, _, group_size = dynamic_check(fmt, "per_group", group_size, what=what)
    if fmt.rounding != "nearest":
        raise ValueError(f"{what}: the definition rounds to nearest, got a format with {fmt.rounding!r} rounding: {fmt!r}")
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        raise ValueError(f"{what}: the weight must be an [out, in] matrix")
    if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: the weight must be float32, float16 or bfloat16, got {w.dtype}")
    L = w.shape[1]
    if L % group_size:
        raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    G = L // group_size
    if not isinstance(blocks, torch.Tensor) or blocks.dtype != torch.float32:
        raise TypeError(f"{what}: blocks must be a float32 tensor, got {getattr(blocks, 'dtype', type(blocks))}")
    if tuple(blocks.shape) != (G, group_size, group_size) or not blocks.is_contiguous():
        raise ValueError(f"{what}: blocks must be a contiguous [{G}, {group_size}, {group_size}] tensor, got {tuple(blocks.shape)}")
    if ratios is None:
        ratios = awq_clip_ratios()
    elif isinstance(ratios, torch.Tensor):
        if ratios.dtype != torch.float32:
            raise TypeError(f"{what}: ratios must be float32, got {ratios.dtype}")
    else:
        try:
            ratios = torch.tensor([float(r) for r in ratios], dtype=torch.float64).to(torch.float32)
        except (TypeError, ValueError):
            raise TypeError(f"{what}: ratios must be None, a sequence of numbers or a float32 tensor, got {ratios!r}") from None
    if ratios.dim() != 1 or not 1 <= ratios.numel() <= AWQ_CLIP_MAX_RATIOS:
        raise ValueError(f"{what}: ratios must hold 1 .. {AWQ_CLIP_MAX_RATIOS} entries in one dimension, got {tuple(ratios.shape)}")
    if not ratios.is_cuda:
        r = ratios.tolist()
        if r[0] != 1.0 or not all(0.0 < v <= 1.0 for v in r) or any(b > a for a, b in zip(r, r[1:])):
            raise ValueError(f"{what}: ratios must start at 1.0, lie in (0, 1] and never increase, got {r}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.shape != w.shape or out.dtype != w.dtype or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous tensor of the weight's shape and dtype")
    return fmt, group_size, ratios


def _awq_clip_device_ratios(ratios, device):
    if ratios.is_cuda:
        return ratios if ratios.is_contiguous() else ratios.contiguous()
    key = (ratios.numpy().tobytes(), device)
    r = _awq_clip_ratio_cache.get(key)
    if r is None:
        if len(_awq_clip_ratio_cache) >= 64:
            _awq_clip_ratio_cache.clear()
        r = _awq_clip_ratio_cache[key] = ratios.to(device)
    return r


def _awq_clip_chain(wc, blocks, r, fmt, g, sym):
    """DESIGN.md §8 "AWQ clipping" as written, in torch operations and library calls -> (y, best, clip, losses)"""
    rows, L = wc.shape
    G, n, T = L // g, r.numel(), wc.dtype
    W = wc.float().reshape(rows, G, g)
    a = W.abs().amax(dim=-1, keepdim=True)
    ordinary = torch.isfinite(a) & (a > 0)
    nan = torch.full_like(a, float("nan"))
    y, clip = wc.reshape(rows, G, g).clone(), a.clone()
    best = torch.zeros(rows, G, 1, dtype=torch.uint8, device=wc.device)
    best_loss = torch.full_like(a, float("inf"))
    losses = torch.empty(rows, G, n, dtype=torch.float32, device=wc.device)
    for i in range(n):
        c = (a * r[i]).to(T).float()
        v = torch.where(W > c, c, torch.where(W < -c, -c, W)).to(T)
        q = dynamic_fixed_qdq(v.reshape(rows, L), fmt, "per_group", g, symmetric_qscheme=sym).float().reshape(rows, G, g)
        d = q - W
        t = blocks[:, :, 0] * d[:, :, 0:1]
        for l in range(1, g):   # (the sum in index order: 2 (g - 1) launches per candidate -- slow by construction)
            t = t + blocks[:, :, l] * d[:, :, l:l + 1]
        p = d * t
        while p.shape[-1] > 1:
            p = p[..., 0::2] + p[..., 1::2]
        loss = torch.where(ordinary, p, nan)
        losses[:, :, i:i + 1] = loss
        better = torch.isfinite(loss) & (loss < best_loss)
        best_loss = torch.where(better, loss, best_loss)
        y = torch.where(better, v, y)
        clip = torch.where(better, c, clip)
        best = torch.where(better, torch.full_like(best, i), best)
    return y.reshape(rows, L), best.reshape(rows, G), clip.reshape(rows, G), losses


def awq_clip(w, blocks, fmt, group_size: int, ratios=None, symmetric_qscheme: bool = False, return_best: bool = False, return_clip: bool = False,
             return_losses: bool = False, out=None, fused: Optional[bool] = None):
    """AWQ weight clipping (AutoAWQ's clip search; DESIGN.md §8 "AWQ clipping"): every group of group_size columns of every row of the
    [out, in] weight w keeps the clipping range c = T(max|W| * ratio), among the candidate `ratios`, whose per-group dynamic integer cast
    q = dynamic_fixed_qdq(clamp(W, -c, c)) disturbs the layer's output least: loss = d^T blocks[k] d with d = q - W and blocks the float32
    [G, g, g] diagonal blocks of the calibration inputs' second moment (awq_gram_blocks).  Returns y, the clamped weight in w's dtype
    (written into `out` when given; out may be w), followed by those asked for of best (uint8 [out, G], the chosen candidate), clip
    (float32 [out, G], its c) and losses (float32 [out, G, n]).  Candidate 0 is no clip, and no group's loss rises above its unclipped
    one; the guarantee is per group -- the off-diagonal blocks of the second moment are not looked at.
    ONE launch (dmxq_awq_clip) for group_size 16, 32, 64 or 128 and 16-byte aligned tensors; the chain of torch operations that spells
    the definition otherwise -- any group size, unaligned views, same bits, and slow by construction (2 (g - 1) launches per candidate
    for the sum in index order alone).  fused=None: the kernel where it applies and group_size is not listed in
    AWQ_CLIP_CHAIN_BY_DEFAULT; True: NotImplementedError instead of falling back; False: the chain.
    ValueError / TypeError before any GPU use: see awq_clip_check."""
    from .observer import get_qmin_qmax
    fmt, group_size, ratios = awq_clip_check(w, blocks, fmt, group_size, ratios, out)
    require_gpu(w, "awq_clip")
    require_gpu(blocks, "awq_clip")
    if out is not None:
        require_gpu(out, "awq_clip")
    qmin, qmax = get_qmin_qmax(fmt)
    sym = bool(symmetric_qscheme)
    with torch.no_grad():
        wc = w.detach()
        wc = wc if wc.is_contiguous() else wc.contiguous()
        rows, L = wc.shape
        G, n = L // group_size, ratios.numel()
        y = out.detach() if out is not None else torch.empty_like(wc)

        def result(best, clip, losses):
            got = tuple(t for t, want in ((y, True), (best, return_best), (clip, return_clip), (losses, return_losses)) if want)
            return got[0] if len(got) == 1 else got

        if wc.numel() == 0:
            return result(torch.empty(rows, G, dtype=torch.uint8, device=wc.device), torch.empty(rows, G, dtype=torch.float32, device=wc.device),
                          torch.empty(rows, G, n, dtype=torch.float32, device=wc.device))
        r = _awq_clip_device_ratios(ratios, wc.device)
        if fused is not False:
            ok = (fmt.precision <= 22 and awq_clip_class(wc.dtype, L, group_size)
                  and all(t.data_ptr() % 16 == 0 for t in (wc, blocks, r, y)))
            if not ok and fused:
                raise NotImplementedError(f"awq_clip: no one-launch kernel for groups of {group_size} in rows of {L} {wc.dtype} elements with "
                                          f"{fmt!r} (weight base address {wc.data_ptr() % 16} mod 16)")
            if ok and fused is None and group_size in AWQ_CLIP_CHAIN_BY_DEFAULT:
                ok = False
            if ok:
                try:
                    best, clip, losses = _ops.awq_clip(wc, blocks.detach(), r, y, int(group_size), fmt.precision, fmt.fraction, bool(fmt.clamp),
                                                       bool(fmt.symmetric), qmin, qmax, sym, bool(return_best), bool(return_clip),
                                                       bool(return_losses))
                    _awq_clip_routes["fused"] += 1
                    return result(best, clip, losses)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _awq_clip_routes["chain"] += 1
        yc, best, clip, losses = _awq_clip_chain(wc, blocks.detach(), r, fmt, group_size, sym)
        y.copy_(yc)
        return result(best, clip, losses)


# ---------------------------------------------------------------------------------------------------- AdaRound (learned weight rounding)
# Classes of dmxq_adaround_forward / dmxq_adaround_backward (adaround_class) that fused=None sends to the chain of torch operations
# although the kernels take them: DYNAMIC_CHAIN_BY_DEFAULT's rule -- a class goes to the kernel by default only where
# tools/bench_adaround.py MEASURED it faster than the chain on the same buffers; a class that is not gets listed here with its row.
ADAROUND_CHAIN_BY_DEFAULT = frozenset()
# which route the calls of this front end took, counted on the host: private, for the tests (fused=True must have run the kernel)
_adaround_routes = {"fused": 0, "chain": 0}
_ADAROUND_CLASS_NAMES = {1: "shift", 2: "divide"}   # dmxq_adaround_geometry (include/dmxq.h)


def _f32(v) -> float:
    """the float32 nearest to v, as a Python float"""
    return torch.tensor(v, dtype=torch.float32).item()


# the stretch constants, float32: G = -0.1f, ZG = 1.1f - (-0.1f) (one float32 subtraction; equals float32(1.2))
ADAROUND_G = _f32(-0.1)
ADAROUND_ZG = (torch.tensor(1.1, dtype=torch.float32) - torch.tensor(-0.1, dtype=torch.float32)).item()


def adaround_check(fmt, granularity="per_group", group_size=None, what: str = "adaround_qdq"):
    """-> (format, granularity, group_size) of an AdaRound cast, or ValueError: dynamic_check's cases (a clamped XP[p,0] format, a known
    granularity, a positive group size with per_group and none otherwise) and nearest rounding.  No GPU involved."""
    fmt, granularity, group_size = dynamic_check(fmt, granularity, group_size, what=what)
    if fmt.rounding != "nearest":
        raise ValueError(f"{what}: learned rounding replaces nearest rounding and is defined for it alone, got {fmt!r}")
    return fmt, granularity, group_size


def adaround_class(segment: int, dtype: torch.dtype, granularity: str = "per_group") -> Optional[str]:
    """how a 16-byte vector of dmxq_adaround_forward / dmxq_adaround_backward finds its segment, asked of the library itself
    (dmxq_adaround_class; no GPU involved), or None when the kernels refuse segments of `segment` elements of `dtype`: "shift" (a
    power-of-two number of vectors per segment), "divide" (any other whole number), "tensor" (per_tensor: ONE segment, no lookup
    arithmetic)"""
    from ._lib import dtype_code, lib
    if granularity not in DYNAMIC_GRANULARITIES:
        raise ValueError(f"adaround_class: granularity must be one of {DYNAMIC_GRANULARITIES}, got {granularity!r}")
    name = _ADAROUND_CLASS_NAMES.get(lib().dmxq_adaround_class(dtype_code(dtype), int(segment)))
    return "tensor" if name is not None and granularity == "per_tensor" else name


def adaround_scratch_bytes(n: int) -> int:
    """dmxq_adaround_scratch_bytes: the scratch dmxq_adaround_backward needs for the regulariser's sum over n elements (8 bytes per
    workgroup).  A host function: no GPU involved."""
    from ._lib import lib
    return int(lib().dmxq_adaround_scratch_bytes(int(n)))


def _adaround_segment(w, V, scale, zero_point, fmt, granularity, group_size, what):
    """-> (format, S, n_seg): every ValueError of the front end, before any GPU use"""
    fmt, granularity, group_size = adaround_check(fmt, granularity, group_size, what=what)
    if not isinstance(w, torch.Tensor) or not w.is_floating_point() or w.dim() < 1:
        raise ValueError(f"{what}: expects a floating point weight with at least one dimension")
    L = w.shape[-1]
    if granularity == "per_group" and L % group_size:
        raise ValueError(f"{what}: the last dimension has {L} elements, not a multiple of the group size {group_size}")
    S = {"per_token": L, "per_group": group_size, "per_tensor": w.numel()}[granularity]
    n_seg = w.numel() // S if S else 0
    if not isinstance(scale, torch.Tensor) or not scale.is_floating_point() or scale.numel() != n_seg:
        raise ValueError(f"{what}: scale must be a floating point tensor of {n_seg} entries (one per segment), got "
                         f"{tuple(scale.shape) if isinstance(scale, torch.Tensor) else scale!r}")
    if not isinstance(zero_point, torch.Tensor) or zero_point.dtype == torch.bool or zero_point.numel() != n_seg:
        raise ValueError(f"{what}: zero_point must be a tensor of {n_seg} integer entries (one per segment), got "
                         f"{tuple(zero_point.shape) if isinstance(zero_point, torch.Tensor) else zero_point!r}")
    if V is not None and (not isinstance(V, torch.Tensor) or V.shape != w.shape or V.dtype != torch.float32):
        raise ValueError(f"{what}: V must be a float32 tensor of the weight's shape {tuple(w.shape)}, got "
                         f"{(tuple(V.shape), V.dtype) if isinstance(V, torch.Tensor) else V!r}")
    return fmt, S, n_seg


def _adaround_beta(beta, reg_weight, what):
    if isinstance(reg_weight, bool) or not isinstance(reg_weight, (int, float)) or not math.isfinite(reg_weight):
        raise ValueError(f"{what}: reg_weight must be a finite number, got {reg_weight!r}")
    if beta is not None and (isinstance(beta, bool) or not isinstance(beta, (int, float)) or not math.isfinite(beta) or beta < 1.0):
        raise ValueError(f"{what}: beta must be a finite number of at least 1 (a^(beta - 1) at a = 0), got {beta!r}")


def adaround_init(w, scale, zero_point, fmt, granularity: str = "per_group", group_size: Optional[int] = None):
    """The rounding variable that starts AdaRound at the weight itself: V0 = -log(ZG / (frac - G) - 1) with v = w / s, frac = v - floor(v),
    a float32 torch chain on w's device (CPU tensors are served too; it runs once).  The soft cast of V0 gives h = frac up to rounding,
    so y = w where nothing clips; the hard cast of V0 is round-HALF-UP of v (frac = 0.5 gives V0 = -0.0, which counts as >= 0): it
    differs from the cast's own round-to-nearest only at exact ties.  -> float32, w's shape.  ValueError as adaround_qdq."""
    fmt, S, _ = _adaround_segment(w, None, scale, zero_point, fmt, granularity, group_size, "adaround_init")
    with torch.no_grad():
        if w.numel() == 0:
            return torch.empty(w.shape, dtype=torch.float32, device=w.device)
        v = w.detach().reshape(-1, S).float() / scale.detach().float().reshape(-1, 1).to(w.device)
        frac = v - torch.floor(v)
        return (-torch.log(ADAROUND_ZG / (frac - ADAROUND_G) - 1.0)).reshape(w.shape)


def _adaround_operands(w, V, scale, zero_point, S):
    wd = w.detach()
    wc = wd if wd.is_contiguous() else wd.contiguous()
    Vd = V.detach()
    Vc = Vd if Vd.is_contiguous() else Vd.contiguous()
    s = scale.detach().to(wc.device, torch.float32).reshape(-1).contiguous()
    z = zero_point.detach().to(wc.device, torch.float32).reshape(-1).contiguous()
    return wc, Vc, s, z


def _adaround_soft(V2):
    """(sg, hr, h) of the definition, float32 torch operations in its order"""
    sg = 1.0 / (1.0 + torch.exp(-V2))
    hr = sg * ADAROUND_ZG + ADAROUND_G
    return sg, hr, torch.clamp(hr, 0.0, 1.0)


def _adaround_forward(wc, Vc, s, z, S, qmin, qmax, hard, out_dtype, fused, granularity):
    """y of the contiguous operands: the kernel where it applies, else the chain"""
    if fused is not False:
        cls = adaround_class(S, wc.dtype, granularity) if (out_dtype in (wc.dtype, torch.float32) and wc.data_ptr() % 16 == 0
                                                            and Vc.data_ptr() % 16 == 0) else None
        if cls is None and fused:
            raise NotImplementedError(f"adaround_qdq: no fused kernel for segments of {S} {wc.dtype} elements with a {out_dtype} output "
                                      f"(base addresses {wc.data_ptr() % 16} / {Vc.data_ptr() % 16} mod 16)")
        if cls is not None and fused is None and cls in ADAROUND_CHAIN_BY_DEFAULT:
            cls = None
        if cls is not None:
            try:
                y = _ops.adaround_forward(wc, Vc, s, z, S, qmin, qmax, bool(hard), out_dtype)
                _adaround_routes["fused"] += 1
                return y
            except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                if fused:
                    raise
    _adaround_routes["chain"] += 1
    # the definition, spelled in torch on the device
    w2, V2 = wc.reshape(-1, S).float(), Vc.reshape(-1, S)
    sc, zq = s[:, None], z[:, None]
    f = torch.floor(w2 / sc)
    h = (V2 >= 0).to(torch.float32) if hard else _adaround_soft(V2)[2]
    q = torch.clamp((f + h) + zq, qmin, qmax)
    return ((q - zq) * sc).to(out_dtype).reshape(wc.shape)


def adaround_backward(w, V, g, scale, zero_point, fmt, granularity: str = "per_group", group_size: Optional[int] = None, beta: float = 2.0,
                      reg_weight: float = 0.0, reg_out=None, want_reg: bool = True, fused: Optional[bool] = None):
    """The backward pass of the AdaRound soft cast (DESIGN.md §8 "AdaRound") -> (dV, reg): dV float32 in w's shape, the gradient of
    sum(g * y) + reg_weight * reg with respect to V (the weight is frozen); reg = sum(1 - |2 h - 1|^beta) over the tensor, a float64
    0-d tensor on the device (None without want_reg and reg_out), also copied into reg_out (float64, one element) when given.
    Per element, every operation float32 in this order:
        v = w / s;  f = floor(v);  sg = 1 / (1 + exp(-V));  hr = sg * ZG + G;  h = clamp(hr, 0, 1)
        in01 = 0 < hr < 1;  cell = qmin <= f + zq <= qmax - 1;  dh = (sg * (1 - sg)) * ZG;  rec = (in01 and cell) ? (g * s) * dh : 0
        t2 = 2 h - 1;  a = |t2|;  p1 = pow(a, beta - 1);  r = 1 - p1 * a;  dreg = in01 ? reg_weight * (((-2 beta * p1) * sign(t2)) * dh) : 0
        dV = rec + dreg (rec alone when reg_weight == 0)
    ONE launch (dmxq_adaround_backward) plus the small fold of the partial sums, where g has the weight's dtype or float32, the
    segment is whole 16-byte vectors of the weight and everything is 16-byte aligned; else the chain: the same definition in torch
    operations.  The same call twice gives the same bits, reg included.  fused: None -- the kernel where it applies and its class is
    not listed in ADAROUND_CHAIN_BY_DEFAULT; True -- NotImplementedError instead of falling back; False -- the chain.  ValueError before
    any GPU use."""
    from .observer import get_qmin_qmax
    fmt, S, n_seg = _adaround_segment(w, V, scale, zero_point, fmt, granularity, group_size, "adaround_backward")
    if not isinstance(g, torch.Tensor) or g.shape != w.shape:
        raise ValueError(f"adaround_backward: g must have the weight's shape {tuple(w.shape)}")
    _adaround_beta(beta, reg_weight, "adaround_backward")
    if beta is None:
        raise ValueError("adaround_backward: beta must be a number")
    if reg_out is not None and not (isinstance(reg_out, torch.Tensor) and reg_out.dtype == torch.float64 and reg_out.numel() == 1):
        raise ValueError("adaround_backward: reg_out must be a float64 tensor of one element")
    require_gpu(w, "adaround_backward")
    require_gpu(V, "adaround_backward")
    require_gpu(g, "adaround_backward")
    qmin, qmax = get_qmin_qmax(fmt)
    want = bool(want_reg) or reg_out is not None
    with torch.no_grad():
        wc, Vc, s, z = _adaround_operands(w, V, scale, zero_point, S)
        gd = g.detach()
        gc = gd if gd.is_contiguous() else gd.contiguous()

        def done(dV, reg):
            if reg_out is not None:
                reg_out.copy_(reg.reshape(reg_out.shape))
            return dV, (reg if want else None)

        if wc.numel() == 0:
            return done(torch.empty(wc.shape, dtype=torch.float32, device=wc.device), torch.zeros((), dtype=torch.float64, device=wc.device))
        if fused is not False:
            cls = adaround_class(S, wc.dtype, granularity) if (gc.dtype in (wc.dtype, torch.float32) and wc.data_ptr() % 16 == 0
                                                                and Vc.data_ptr() % 16 == 0 and gc.data_ptr() % 16 == 0) else None
            if cls is None and fused:
                raise NotImplementedError(f"adaround_backward: no fused kernel for segments of {S} {wc.dtype} elements with a {gc.dtype} "
                                          f"gradient (base addresses {wc.data_ptr() % 16} / {Vc.data_ptr() % 16} / {gc.data_ptr() % 16} mod 16)")
            if cls is not None and fused is None and cls in ADAROUND_CHAIN_BY_DEFAULT:
                cls = None
            if cls is not None:
                try:
                    dV, reg = _ops.adaround_backward(wc, Vc, gc, s, z, S, qmin, qmax, float(beta), float(reg_weight), want)
                    _adaround_routes["fused"] += 1
                    return done(dV, reg.reshape(()) if want else None)
                except NotImplementedError:   # (DMXQ_ERR_UNSUPPORTED, nothing launched)
                    if fused:
                        raise
        _adaround_routes["chain"] += 1
        # the definition, spelled in torch on the device
        w2, V2, g2 = wc.reshape(-1, S).float(), Vc.reshape(-1, S), gc.reshape(-1, S).float()
        sc, zq = s[:, None], z[:, None]
        fz = torch.floor(w2 / sc) + zq
        cell = (fz >= qmin) & (fz <= qmax - 1)
        sg, hr, h = _adaround_soft(V2)
        in01 = (hr > 0) & (hr < 1)
        dh = (sg * (1.0 - sg)) * ADAROUND_ZG
        zero = torch.zeros_like(dh)
        dV = torch.where(in01 & cell, (g2 * sc) * dh, zero)
        reg = None
        rw = _f32(reg_weight)
        if rw != 0.0 or want:
            b = torch.tensor(float(beta), dtype=torch.float32)
            bm1, m2b = (b - 1.0).item(), (-2.0 * b).item()
            t2 = 2.0 * h - 1.0
            a = torch.abs(t2)
            p1 = torch.pow(a, bm1)
            if rw != 0.0:
                dV = dV + torch.where(in01, rw * (((m2b * p1) * torch.sign(t2)) * dh), zero)
            if want:
                reg = (1.0 - p1 * a).sum(dtype=torch.float64)
        return done(dV.reshape(wc.shape), reg)


class _AdaRoundCast(torch.autograd.Function):
    """forward: the soft (or hard) cast; backward: adaround_backward -- the gradient of V alone"""

    @staticmethod
    def forward(ctx, w, V, scale, zero_point, fmt, granularity, group_size, S, hard, beta, reg_weight, reg_out, out_dtype, fused):
        from .observer import get_qmin_qmax
        qmin, qmax = get_qmin_qmax(fmt)
        wc, Vc, s, z = _adaround_operands(w, V, scale, zero_point, S)
        if wc.numel() == 0:
            y = torch.empty(wc.shape, dtype=out_dtype, device=wc.device)
        else:
            y = _adaround_forward(wc, Vc, s, z, S, qmin, qmax, hard, out_dtype, fused, granularity)
        ctx.save_for_backward(wc, Vc, s, z)
        ctx.args = (fmt, granularity, group_size, beta, reg_weight, reg_out, fused, hard)
        return y

    @staticmethod
    def backward(ctx, g):
        wc, Vc, s, z = ctx.saved_tensors
        fmt, granularity, group_size, beta, reg_weight, reg_out, fused, hard = ctx.args
        dV = None
        if ctx.needs_input_grad[1]:
            if hard:
                raise RuntimeError("adaround_qdq: the hard cast has no gradient; optimise the soft cast (hard=False)")
            if g.dtype not in (wc.dtype, torch.float32):
                g = g.to(torch.float32)
            dV, _ = adaround_backward(wc, Vc, g, s, z, fmt, granularity, group_size, beta=2.0 if beta is None else beta, reg_weight=reg_weight,
                                      reg_out=reg_out, want_reg=False, fused=fused)
        return (None, dV) + (None,) * 12


def adaround_qdq(w, V, scale, zero_point, fmt, granularity: str = "per_group", group_size: Optional[int] = None, hard: bool = False,
                 beta: Optional[float] = None, reg_weight: float = 0.0, reg_out=None, out_dtype: Optional[torch.dtype] = None,
                 fused: Optional[bool] = None):
    """The AdaRound cast (Nagel et al., 2020; DESIGN.md §8 "AdaRound"): the weight on the grid of an integer cast with one (scale,
    integer zero point) per segment (segments as in lsq_fixed_qdq), rounded down or up per element by the float32 variable V.  Per
    element, every operation float32 in this order, G = -0.1f, ZG = 1.1f - (-0.1f):
        v = w / s;  f = floor(v);  h = clamp((1 / (1 + exp(-V))) * ZG + G, 0, 1)   (hard=True: h = V >= 0 ? 1 : 0)
        y = (clamp((f + h) + zq, qmin, qmax) - zq) * s, rounded once more to out_dtype (default: w's dtype)
    An autograd Function: its backward is adaround_backward and forms ONLY the gradient of V -- w, scale and zero_point get none -- as
    the gradient of sum(g * y) + reg_weight * sum(1 - |2 h - 1|^beta); the regulariser's VALUE is written into reg_out (float64, one
    element) during the backward when given.  beta None: no regulariser (reg_weight must be 0 and reg_out None).
    ONE launch (dmxq_adaround_forward) where out_dtype is w's dtype or float32, the segment is whole 16-byte vectors of the weight and
    w / V are 16-byte aligned; else the chain of torch operations that spells the definition (any S, unaligned views, any out_dtype).
    fused: None -- the kernel where it applies and its class is not listed in ADAROUND_CHAIN_BY_DEFAULT; True -- NotImplementedError
    instead of falling back; False -- the chain.  ValueError before any GPU use: a format that is not a clamped XP[p,0] with nearest
    rounding, a group size that does not divide the last dimension, parameters that are not one entry per segment, a V of another shape
    or dtype."""
    fmt, S, _ = _adaround_segment(w, V, scale, zero_point, fmt, granularity, group_size, "adaround_qdq")
    _adaround_beta(beta, reg_weight, "adaround_qdq")
    if beta is None and (reg_weight != 0 or reg_out is not None):
        raise ValueError("adaround_qdq: the regulariser (reg_weight, reg_out) needs beta")
    if reg_out is not None and not (isinstance(reg_out, torch.Tensor) and reg_out.dtype == torch.float64 and reg_out.numel() == 1):
        raise ValueError("adaround_qdq: reg_out must be a float64 tensor of one element")
    if out_dtype is not None and not (isinstance(out_dtype, torch.dtype) and out_dtype.is_floating_point):
        raise ValueError(f"adaround_qdq: out_dtype must be a floating point dtype, got {out_dtype!r}")
    require_gpu(w, "adaround_qdq")
    require_gpu(V, "adaround_qdq")
    return _AdaRoundCast.apply(w, V, scale, zero_point, fmt, granularity, group_size, S, bool(hard), beta, float(reg_weight), reg_out,
                               out_dtype or w.dtype, fused)
