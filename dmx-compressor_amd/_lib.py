"""ctypes binding of libdmxq.so (C ABI: include/dmxq.h).

This is the ONLY compute back-end of the package: there is no CPU or eager-PyTorch fallback.  If the HIP
library is missing or a tensor is not on a GPU, the ops raise instead of silently computing elsewhere.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DMXQ_LIB_PATH") or os.path.join(_HERE, "lib", "libdmxq.so")  # (override: A/B runs of two builds; DMXQ_BINDING=ctypes only, ops.py refuses it otherwise)

F32, F16, BF16 = 0, 1, 2
ROUND_UP, ROUND_DOWN, ROUND_NEAREST, ROUND_STOCHASTIC = 0, 1, 2, 3
ROUNDING_CODE = {"up": ROUND_UP, "down": ROUND_DOWN, "nearest": ROUND_NEAREST, "stochastic": ROUND_STOCHASTIC}
OK, ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_PENDING = 0, 1, 2, 3, 4

_DTYPE_CODE = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}

_vp, _i64, _i32, _u64, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_float

# name -> argtypes; mirrors include/dmxq.h one to one (tests/test_abi.py checks header <-> table <-> .so)
SIGNATURES = {
    "dmxq_bfp_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _u64, _vp],
    "dmxq_bfp_qdq_multi": [_vp, _i64, _i32, _i32, _i64, _i32, _i32, _i32, _u64, _vp],
    "dmxq_bfp_qdq_describe": [_i32, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, ctypes.c_char_p, _i64],
    "dmxq_sbfp_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "dmxq_mxfp_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _vp],
    "dmxq_bfp_pack": [_vp, _i32, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp],
    "dmxq_bfp_unpack": [_vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp],
    "dmxq_weight_hypernet": [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _vp],
    "dmxq_weight_hypernet_multi": [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i64, _i32, _i32, _vp],
    "dmxq_weight_hypernet_strided": [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _vp],
    "dmxq_input_hypernet": [_vp, _i32, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _vp],
    "dmxq_binary_cast": [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp],
    "dmxq_relu_cast": [_vp, _vp, _i32, _i64, _vp, _vp, _vp],
    "dmxq_binary_cast_bfp": [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "dmxq_relu_cast_bfp": [_vp, _vp, _i32, _i64, _vp, _vp, _i64, _i64, _i32, _vp],
    "dmxq_unary_cast": [_vp, _vp, _i32, _i64, _i32, _f32, _vp, _vp, _vp],
    "dmxq_unary_cast_table": [_i32, _i32, _f32, _vp, _vp, _vp, _vp],
    "dmxq_lut16_apply": [_vp, _vp, _i64, _vp, _vp],
    "dmxq_softmax_cast": [_vp, _vp, _i32, _i64, _i64, _f32, _vp, _vp, _vp],
    "dmxq_softmax_cast_bfp": [_vp, _vp, _i32, _i64, _i64, _f32, _vp, _vp, _i64, _i32, _vp],
    "dmxq_layernorm_cast": [_vp, _vp, _i32, _i64, _i64, _vp, _vp, _f32, _vp, _vp, _vp],
    "dmxq_rmsnorm_cast": [_vp, _vp, _i32, _i64, _i64, _vp, _f32, _vp, _vp, _vp],
    "dmxq_layernorm_cast_bfp": [_vp, _vp, _i32, _i64, _i64, _vp, _vp, _f32, _vp, _vp, _i64, _i32, _vp],
    "dmxq_rmsnorm_cast_bfp": [_vp, _vp, _i32, _i64, _i64, _vp, _f32, _vp, _vp, _i64, _i32, _vp],
    "dmxq_float_qdq": [_vp, _vp, _i32, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _vp],
    "dmxq_fixed_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _u64, _vp],
    "dmxq_fixed_qdq_multi": [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i64, _u64, _vp],
    "dmxq_float_qdq_multi": [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _vp],
    "dmxq_fixed_float_qdq_multi": [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _vp],
    "dmxq_nm_mask": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _vp],
    "dmxq_nm_mask_class": [_i32, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "dmxq_topk_workspace_bytes": [_i64],
    "dmxq_topk_mask": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i64, _i64, _vp, _vp],
    "dmxq_bernoulli_mask": [_vp, _vp, _i32, _i32, _i64, _u64, _vp],
    "dmxq_group_minmax": [_vp, _i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp],
    "dmxq_group_minmax_accumulate": [_vp, _i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp],
    "dmxq_qparams": [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp],
    "dmxq_histc": [_vp, _i32, _i64, _i64, _f32, _f32, _vp, _vp],
    "dmxq_channel_maxabs": [_vp, _i32, _i64, _i64, _i64, _vp, _vp],
    "dmxq_smoothquant_scale": [_vp, _vp, _i64, _f32, _f32, _vp, _vp],
    "dmxq_scale_channels": [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _vp, _i32, _vp],
    "dmxq_gelu": [_vp, _vp, _i32, _i32, _i64, _i32, _vp],
    "dmxq_unary": [_vp, _vp, _i32, _i32, _i64, _i32, _f32, _vp],
    "dmxq_rmsnorm": [_vp, _vp, _i32, _i32, _i64, _i64, _vp, _i32, _f32, _vp],
    "dmxq_rope": [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i64, _i32, _vp],
    "dmxq_rope_cast": [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    "dmxq_softmax": [_vp, _vp, _i32, _i32, _i64, _i64, _f32, _vp],
    "dmxq_layernorm": [_vp, _vp, _i32, _i32, _i64, _i64, _vp, _vp, _i32, _f32, _vp],
    "dmxq_gptq_block": [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp],
    "dmxq_gptq_block_dynamic": [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i32, _i64, _i32, _i32, _i32, _vp, _i64,
                                _vp, _i64, _vp],
    "dmxq_hist_observe": [_vp, _i32, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "dmxq_hist_qparams": [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "dmxq_error_scratch_bytes": [_i64, _i32],
    "dmxq_error_stats": [_vp, _i32, _vp, _i32, _i64, _i32, _vp, _vp, _i64, _vp],
    "dmxq_cast_error": [_vp, _i32, _i64, _i64, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i64, _vp],
    "dmxq_hadamard_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "dmxq_dynamic_class": [_i32, _i64, _i32],
    "dmxq_dynamic_float_class": [_i32, _i32, _i64],
    "dmxq_dynamic_float_qdq": [_vp, _vp, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "dmxq_dynamic_fixed_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "dmxq_channel_sumsq_workspace_bytes": [_i64, _i64],
    "dmxq_channel_sumsq_accumulate": [_vp, _i32, _i64, _i64, _vp, _vp, _vp],
    "dmxq_wanda_class": [_i32, _i64, _i32],
    "dmxq_wanda_nm": [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i64, _i64, _i32, _i32, _vp],
    "dmxq_channel_sumabs_accumulate": [_vp, _i32, _i64, _i64, _vp, _vp, _vp],
    "dmxq_awq_class": [_i32, _i64, _i64],
    "dmxq_awq_group_error": [_vp, _i32, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "dmxq_block_scaled_float_class": [_i32, _i64],
    "dmxq_block_scaled_tensor_scale": [_vp, _i32, _i64, _f32, _f32, _vp, _vp],
    "dmxq_block_scaled_float_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp],
    "dmxq_lsq_class": [_i32, _i64, _i32],
    "dmxq_lsq_scratch_bytes": [_i64],
    "dmxq_lsq_backward": [_vp, _vp, _vp, _i32, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, ctypes.c_double, _i32, _vp, _vp, _vp, _i64,
                          _vp],
    "dmxq_codebook_class": [_i32, _i32, _i64],
    "dmxq_codebook_qdq": [_vp, _vp, _i32, _i32, _i32, _i64, _i64, _vp, _i32, _f32, _vp, _vp, _vp],
    "dmxq_codebook_workspace_bytes": [_i32, _i32, _i64, _i64],
    "dmxq_codebook_accumulate": [_vp, _i32, _i32, _i64, _i64, _vp, _i32, _f32, _vp, _i32, _vp, _vp],
    "dmxq_hqq_class": [_i32, _i64],
    "dmxq_hqq_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _f32, _f32, _f32, _i32, _vp, _vp, _vp, _vp],
    "dmxq_outlier_class": [_i32, _i64],
    "dmxq_outlier_fixed_qdq": [_vp, _vp, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "dmxq_awq_clip_class": [_i32, _i64, _i64],
    "dmxq_awq_clip": [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "dmxq_vq_class": [_i32, _i32, _i64, _i32, _i32],
    "dmxq_vq_qdq": [_vp, _vp, _i32, _i32, _i32, _i64, _i64, _vp, _i32, _i32, _f32, _vp, _vp, _vp],
    "dmxq_vq_workspace_bytes": [_i32, _i32, _i64, _i64, _i32, _i32],
    "dmxq_vq_accumulate": [_vp, _i32, _i32, _i64, _i64, _vp, _i32, _i32, _f32, _vp, _i32, _vp, _vp],
    "dmxq_adaround_class": [_i32, _i64],
    "dmxq_adaround_scratch_bytes": [_i64],
    "dmxq_adaround_forward": [_vp, _vp, _vp, _i32, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _i32, _vp],
    "dmxq_adaround_backward": [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _f32, _f32, _vp, _vp, _i64, _vp],
    "dmxq_row_class_of": [_i32, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _vp],
}

# dmxq_row_op / dmxq_row_cast_kind / dmxq_row_family / dmxq_row_grid (include/dmxq.h)
ROW_SOFTMAX, ROW_LAYERNORM, ROW_RMSNORM = 0, 1, 2
ROWCAST_NONE, ROWCAST_RANGE, ROWCAST_GENERAL, ROWCAST_MAN16 = 0, 1, 2, 3
ROWK_UNSUPPORTED, ROWK_WAVE, ROWK_BLOCK, ROWK_LDS_ROWS, ROWK_GLOBAL_ROWS = 0, 1, 2, 3, 4
ROWGRID_NONE, ROWGRID_PERSISTENT, ROWGRID_ONE_PASS, ROWGRID_MID_ONE_PASS, ROWGRID_MODULE_ONE_PASS, ROWGRID_MODULE_ROWS4, ROWGRID_CAPPED = range(7)

# dmxq_nm_route (include/dmxq.h) and the grid cap of the grid-stride kernels (DMXQ_GRID_CAP)
NM_NONE, NM_TYPED, NM_F32_MASK, NM_VECTOR, NM_GROUP_M, NM_ANY_M = range(6)
NM_ROUTE_NAMES = {NM_NONE: "none", NM_TYPED: "typed", NM_F32_MASK: "f32_mask", NM_VECTOR: "vector", NM_GROUP_M: "group_m", NM_ANY_M: "any_m"}
GRID_CAP = 2048


class RowClass(ctypes.Structure):
    """dmxq_row_class (include/dmxq.h)"""
    _fields_ = [(n, _i32) for n in ("family", "epl", "vpl", "lpr", "rag", "half_vec", "fast32", "bfpout", "grid", "rows_per_iter")]

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


class TensorDesc(ctypes.Structure):
    """dmxq_tensor_desc (include/dmxq.h)"""
    _fields_ = [("in_", _vp), ("out", _vp), ("outer", _i64), ("L", _i64), ("inner", _i64)]


class HypernetDesc(ctypes.Structure):
    """dmxq_hypernet_desc (include/dmxq.h)"""
    _fields_ = [("w", _vp), ("score", _vp), ("sq_scale", _vp), ("out", _vp), ("rows", _i64), ("L", _i64)]


class FloatFmt(ctypes.Structure):
    """dmxq_float_fmt (include/dmxq.h)"""
    _fields_ = [("man_bits", _i32), ("exp_bits", _i32), ("exp_bias", _i32), ("flush_subnormal", _i32)]


class AffineDesc(ctypes.Structure):
    """dmxq_affine_desc (include/dmxq.h)"""
    _fields_ = [("in_", _vp), ("out", _vp), ("scale", _vp), ("zero_point", _vp), ("outer", _i64), ("C", _i64), ("inner", _i64)]


class GptqFormat(ctypes.Structure):
    """dmxq_gptq_format (include/dmxq.h)"""
    _fields_ = [("kind", _i32), ("precision", _i32), ("block_size", _i32), ("symmetric", _i32), ("man_bits", _i32), ("exp_bits", _i32),
                ("exp_bias", _i32), ("flush_subnormal", _i32), ("unsigned_abs", _i32), ("fraction", _i32), ("clamp", _i32), ("per_row", _i32)]


GPTQ_BFP, GPTQ_FLOAT, GPTQ_FIXED, GPTQ_MXFP = 0, 1, 2, 3   # (MXFP: dmxq_hadamard_qdq only)


class DmxqError(RuntimeError):
    pass


_lib = None


def lib():
    """Loads libdmxq.so; raises DmxqError (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DmxqError(
                f"{LIB_PATH} not found: build the HIP library first (python dmx-compressor_amd/build.py or "
                "__graft_entry__.build()).  dmx_compressor_amd has no CPU/eager fallback."
            )
        L = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int
        L.dmxq_topk_workspace_bytes.restype = ctypes.c_int64
        L.dmxq_error_scratch_bytes.restype = ctypes.c_int64
        L.dmxq_channel_sumsq_workspace_bytes.restype = ctypes.c_int64
        L.dmxq_lsq_scratch_bytes.restype = ctypes.c_int64
        L.dmxq_codebook_workspace_bytes.restype = ctypes.c_int64
        L.dmxq_adaround_scratch_bytes.restype = ctypes.c_int64
        L.dmxq_vq_workspace_bytes.restype = ctypes.c_int64
        L.dmxq_status_string.argtypes = [ctypes.c_int]
        L.dmxq_status_string.restype = ctypes.c_char_p
        L.dmxq_abi_version.restype = ctypes.c_int
        _lib = L
    return _lib


def check(status: int, what: str):
    if status != OK:
        msg = lib().dmxq_status_string(status).decode()
        if status == ERR_UNSUPPORTED:
            raise NotImplementedError(f"{what}: {msg}")
        raise DmxqError(f"{what}: {msg} (status {status})")


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DTYPE_CODE[dt]
    except KeyError:
        raise TypeError(f"dmxq kernels take float32/float16/bfloat16 tensors, got {dt}") from None


def require_gpu(x: torch.Tensor, what: str):
    if not x.is_cuda:
        raise DmxqError(
            f"{what}: tensor is on {x.device}; dmx_compressor_amd runs on MI355X (HIP) tensors only and has no "
            "CPU fallback"
        )


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream_of(x: torch.Tensor):
    """hipStream_t of torch's current stream on x's device (kernels are enqueued there, never on the null stream)."""
    idx = x.device.index
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx))


def split3(shape, dim):
    """[outer, L, inner] factorisation of a contiguous tensor around `dim`."""
    nd = len(shape)
    d = dim % nd
    outer = 1
    for s in shape[:d]:
        outer *= s
    inner = 1
    for s in shape[d + 1:]:
        inner *= s
    return outer, shape[d], inner
