"""CastTo / CastToDict / CastToFormat — mirror of the reference's `numerical/cast.py` op containers.

`CastTo.forward` keeps the reference's order of operations (cast.py:261-306: remember physical dtype ->
pre_transform {shaping, noquant_shortcut, format} -> [hadamard rotation: not in the reference, DESIGN.md §8] -> observer step ->
[affine] -> format cast -> [inverse affine] -> [inverse rotation] -> shortcut restore -> inverse shaping -> `.to(physical_dtype)`), but the arithmetic part
(`.float()`, `x/sc + zp`, the format cast, `(x - zp)*sc`, the final narrowing) is ONE kernel launch with the
input and output in the tensor's own dtype, instead of 5-7 elementwise ATen passes around a chunked native call.
"""
import warnings
from typing import Dict, Optional, Union

import torch
from torch.autograd import Function

from . import ops
from ._flags import HostFlags
from .format import FixedPoint, FloatingPoint, Format, Same
from .observer import _PER_CHANNEL, _SYMMETRIC, DummyObserver, HistogramObserver, MinMaxObserver, ObserverBase

__all__ = ["CastToFormat", "CastTo", "CastToDict"]

_LEARNED_SCALE_MIN = float(torch.finfo(torch.float32).eps)   # learned_scale is clamped from below to this before every forward
_CODEBOOK_HADAMARD = ("CastTo: a codebook (set_codebook) under a 'hadamard' pre_transform is not supported: the fused rotated cast runs the "
                      "format's arithmetic, not a table's")
_VQ_HADAMARD = ("CastTo: a vector codebook (set_vq) under a 'hadamard' pre_transform is not supported: the fused rotated cast runs the "
                "format's own arithmetic with the stored scales; drop one of the two")
_VQ_EXCLUSIVE = ("this cast has a vector codebook (set_vq), which replaces the format's arithmetic and its scales: set_vq(None) first")
_CODEBOOK_EXCLUSIVE = ("this cast has a codebook (set_codebook), which replaces the format's arithmetic and its scales: "
                       "set_codebook(None) first")
_LEARNABLE_HADAMARD = ("CastTo: learned scales (set_learnable) under a 'hadamard' pre_transform are not supported: the fused rotated cast "
                       "reads the stored scale / zero_point buffers, and the rotated straight-through estimator would give the learned "
                       "parameters no gradient; drop one of the two settings")


class CastToFormat(Function):
    """Numerical cast with a straight-through-estimator backward (cast.py:20-32)."""

    @staticmethod
    def forward(ctx, x, fmt, block_dim, out_dtype=torch.float32):
        ctx.set_materialize_grads(False)
        ctx.in_dtype = x.dtype
        return fmt.cast(x, block_dim, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, g):
        if g is not None and g.dtype != ctx.in_dtype:
            g = g.to(ctx.in_dtype)
        return g, None, None, None


class _FixedAffineCast(Function):
    """x/sc + zp -> FixedPoint cast -> (x - zp)*sc as one launch (cast.py:278-296), STE backward."""

    @staticmethod
    def forward(ctx, x, fmt, scale, zero_point, ch_axis, group_size, out_dtype):
        ctx.set_materialize_grads(False)
        ctx.in_dtype = x.dtype
        return ops.fixed_qdq(x, fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=scale,
                             zero_point=zero_point, ch_axis=ch_axis, group_size=group_size, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, g):
        if g is not None and g.dtype != ctx.in_dtype:
            g = g.to(ctx.in_dtype)
        return g, None, None, None, None, None, None


class _RotatedSTE(Function):
    """rotation -> observer step -> cast -> inverse rotation of a CastTo with a "hadamard" pre_transform, as ONE straight-through
    estimator: R is its own inverse, so the backward is the identity (not R(R(g)), which is g only up to rounding)."""

    @staticmethod
    def forward(ctx, x, cast, had):
        ctx.set_materialize_grads(False)
        ctx.in_dtype = x.dtype
        return cast._rotate_observe_cast(x.detach(), had)

    @staticmethod
    def backward(ctx, g):
        if g is not None and g.dtype != ctx.in_dtype:
            g = g.to(ctx.in_dtype)
        return g, None, None


def _parse_hadamard(spec):
    """pre_transform["hadamard"]: 64 or {"size": 64, "inverse": False} -> {"size", "inverse"} (inverse defaults to True)"""
    if isinstance(spec, dict):
        extra = set(spec) - {"size", "inverse"}
        if extra or "size" not in spec:
            raise ValueError(f"pre_transform['hadamard']: expected {{'size': int, 'inverse': bool}}, got {spec!r}")
        size, inverse = spec["size"], spec.get("inverse", True)
    else:
        size, inverse = spec, True
    if not isinstance(inverse, bool):
        raise ValueError(f"pre_transform['hadamard']: inverse must be a bool, got {inverse!r}")
    return {"size": ops.hadamard_check_size(size, "pre_transform['hadamard']"), "inverse": inverse}


def _parse_dynamic(granularity, group_size=None):
    """set_dynamic's arguments -> None or (granularity, group_size): None / False, "per_token", "per_tensor", ("per_group", g) or
    {"per_group": g}"""
    if granularity is None or granularity is False:
        if group_size is not None:
            raise ValueError(f"set_dynamic: group_size {group_size!r} without a granularity")
        return None
    if isinstance(granularity, dict):
        if set(granularity) != {"per_group"} or group_size is not None:
            raise ValueError(f"set_dynamic: expected {{'per_group': int}}, got {granularity!r}")
        granularity, group_size = "per_group", granularity["per_group"]
    return granularity, group_size


_OUTLIER_KEYS = ("outliers", "outlier_format")


def _parse_outliers(setting):
    """set_dynamic's dict spellings with "outliers" -> (the setting without the outlier keys, None or {"k", "outlier_format"}):
    {"per_group": g, "outliers": k} and {"granularity": "per_token", "outliers": k}, each optionally with "outlier_format" (None or a
    per-element FloatingPoint format).  Every other setting passes through with None."""
    if not isinstance(setting, dict) or not set(setting) & set(_OUTLIER_KEYS):
        return setting, None
    if "outliers" not in setting:
        raise ValueError(f"set_dynamic: 'outlier_format' goes with 'outliers', got {setting!r}")
    d = dict(setting)
    k, ofmt = d.pop("outliers"), d.pop("outlier_format", None)
    if set(d) == {"granularity"}:
        if d["granularity"] != "per_token":
            raise ValueError(f"set_dynamic: outliers go with {{'per_group': g}} or {{'granularity': 'per_token'}}, got {setting!r}")
        d = "per_token"
    elif set(d) != {"per_group"}:
        raise ValueError(f"set_dynamic: outliers go with {{'per_group': g}} or {{'granularity': 'per_token'}}, got {setting!r}")
    return d, {"k": k, "outlier_format": ofmt}


def _parse_scaling(granularity, group_size=None, pow2_scale=False):
    """set_scaling's arguments -> None or (granularity, group_size, pow2_scale).  granularity: None / False, "per_token", "per_tensor",
    "per_group" or "per_tile" (these two with group_size as the second argument), the pair ("per_group" | "per_tile", g), or a dict
    {"per_group": g} / {"per_tile": g} / {"granularity": name}, each optionally with "pow2_scale": bool (the spelling
    DmxModule.configure takes)"""
    if isinstance(granularity, (tuple, list)) and len(granularity) == 2 and group_size is None:
        granularity, group_size = granularity
    if isinstance(granularity, dict):
        d = dict(granularity)
        if "pow2_scale" in d:
            if pow2_scale:
                raise ValueError(f"set_scaling: pow2_scale given twice, got {granularity!r}")
            pow2_scale = d.pop("pow2_scale")
        if len(d) != 1 or group_size is not None or next(iter(d)) not in ("per_group", "per_tile", "granularity"):
            raise ValueError(f"set_scaling: expected {{'per_group': int}}, {{'per_tile': int}} or {{'granularity': name}}, optionally with "
                             f"'pow2_scale', got {granularity!r}")
        (k, v), = d.items()
        granularity, group_size = (v, None) if k == "granularity" else (k, v)
    if not isinstance(pow2_scale, bool):
        raise ValueError(f"set_scaling: pow2_scale must be a bool, got {pow2_scale!r}")
    if granularity is None or granularity is False:
        if group_size is not None or pow2_scale:
            raise ValueError(f"set_scaling: group_size {group_size!r} / pow2_scale {pow2_scale!r} without a granularity")
        return None
    return granularity, group_size, pow2_scale


_BLOCK_SCALE_KEYS = ("scale_format", "scale_max", "tensor_scale")


def _split_block_scale(setting):
    """set_scaling's dict form -> (the setting without the block-scale keys, None or {those keys}): "scale_format" (the format the
    group scales are quantised to), optionally "scale_max" and "tensor_scale" (ops.block_scaled_float_qdq; ops.NVFP4 is such a dict)"""
    if not isinstance(setting, dict) or not any(k in setting for k in _BLOCK_SCALE_KEYS):
        return setting, None
    d = dict(setting)
    b = {k: d.pop(k) for k in _BLOCK_SCALE_KEYS if k in d}
    if "scale_format" not in b:
        raise ValueError(f"set_scaling: {sorted(b)} only mean something for quantised group scales: add 'scale_format' (the format of "
                         f"the scales, e.g. 'FP[1|4|3,7](_N)') or drop them, got {setting!r}")
    return d, b


class CastTo(HostFlags, torch.nn.Module):
    """Simulated numerical cast to a target format (cast.py:136-162).  Buffers and switches follow
    torch.ao's FakeQuantize, which the reference subclasses: scale, zero_point, fake_quant_enabled,
    observer_enabled, qscheme, ch_axis.  The two switches are read from host mirrors (_flags.py): forward never
    waits for the device."""
    _flag_names = ("fake_quant_enabled", "observer_enabled")
    #: a SAME-format cast returns a COPY, like the reference's Same.cast (`x.clone()`, numerical/format.py:89-90): the
    #: caller may mutate the result in place.  DmxModule switches this off on the casts it owns (their results are
    #: consumed inside the module) and re-establishes the no-alias guarantee once, at the module boundary (nn.py).
    copy_on_same = True
    #: cast a transposed / permuted view IN ITS OWN LAYOUT: the kernels take contiguous tensors, so a dense permuted view is cast through
    #: the permutation that makes it contiguous (the block dimension follows it) and the result is handed back with the input's strides,
    #: instead of being copied to a contiguous tensor first.  Same values; set by modules whose `_forward` takes any strides
    #: (ActActMatMul: q / k^T / v of an attention arrive as transposed views -- k^T blocked along -2 is k blocked along its LAST dim).
    keep_layout = False
    #: None, or (granularity, group_size): scale and zero point are derived from every tensor itself (set_dynamic).  A plain
    #: attribute, not a buffer: the state_dict of a module does not change.
    _dynamic = None
    #: None, or {"k", "outlier_format"} beside a per_group / per_token _dynamic: every segment keeps its k largest magnitudes exact, or in
    #: the per-element float format (ops.outlier_fixed_qdq; DESIGN.md §8 "Outlier-aware dynamic cast").  A plain attribute as well.
    _outliers = None
    #: None, or (granularity, group_size, pow2_scale): a float format is cast with a scale derived from every tensor itself (set_scaling;
    #: DESIGN.md §8).  A plain attribute as well.
    _scaling = None
    #: None, or (scale_format, scale_max, tensor_scale) beside a per_group _scaling: the group scales are quantised to scale_format under
    #: one float32 scale per tensor (ops.block_scaled_float_qdq).  A plain attribute as well.
    _block_scale = None
    #: None, or {"granularity", "group_size", "learn_zero_point", "grad_scale", "init"}: an integer format is cast with a LEARNED scale and
    #: zero point per segment (set_learnable; DESIGN.md §8 "Learned step size").  The two nn.Parameters exist only while this is set.
    _learnable = None
    #: the learned parameters still wait for their data-dependent initial values (filled in place by the first forward): a host flag
    _learnable_pending = False
    #: None, or {"granularity", "group_size", "norm", "name"}: the cast runs ops.codebook_qdq with the float32 buffer `codebook` in place of
    #: the format's arithmetic (set_codebook; DESIGN.md §8 "Codebook casts").  The buffer exists only while this is set.
    _codebook = None
    #: None, or {"granularity", "group_size", "norm", "grid"}: the cast runs ops.vq_qdq with the float32 buffer `vq_codebook` [K, d] in place
    #: of the format's arithmetic (set_vq; DESIGN.md §8 "Vector codebook casts").  The buffers exist only while this is set.
    _vq = None

    def __init__(self, format="SAME", observer=DummyObserver, group_size=None, block_dim=-1,
                 qscheme=torch.per_tensor_affine, ch_axis=-1, **observer_kwargs):
        super().__init__()
        self.set_format(format)
        self.qscheme, self.ch_axis = qscheme, ch_axis
        self.is_per_channel = qscheme in _PER_CHANNEL
        if group_size:
            assert not self.is_per_channel, "group_size must be used with per tensor quantization scheme"
        self.group_size = group_size if group_size else None
        self.activation_post_process = observer(dtype=self.format, qscheme=qscheme, ch_axis=ch_axis, **observer_kwargs)
        self.register_buffer("scale", torch.tensor([1.0], dtype=torch.float))
        self.register_buffer("zero_point", torch.tensor([0], dtype=torch.int64))
        self.register_buffer("fake_quant_enabled", torch.tensor([1], dtype=torch.uint8))
        self.register_buffer("observer_enabled", torch.tensor([0], dtype=torch.uint8))
        self.refresh_flags()
        self.physical_dtype = None
        self.block_dim = block_dim
        self.pre_transform = {}

    # ------------------------------------------------------------------ switches (FakeQuantize API)
    def enable_fake_quant(self, enabled: bool = True):
        self._set_flag("fake_quant_enabled", enabled)

    def disable_fake_quant(self):
        self.enable_fake_quant(False)

    def enable_observer(self, enabled: bool = True):
        self._set_flag("observer_enabled", enabled)

    def disable_observer(self):
        self.enable_observer(False)

    def calculate_qparams(self):
        return self.activation_post_process.calculate_qparams()

    # ------------------------------------------------------------------ configuration
    def set_format(self, format: Union[str, torch.dtype, Format]):
        if isinstance(format, str):
            format = Format.from_shorthand(format)
        if self._dynamic is not None and not isinstance(format, Same):
            ops.dynamic_check(format, *self._dynamic, what="CastTo.set_format on a dynamic cast")
            if self._outliers is not None:
                ops.outlier_check(format, self._dynamic[1], self._outliers["k"], self._outliers["outlier_format"], self._dynamic[0],
                                  what="CastTo.set_format on a dynamic cast with outliers")
        if self._scaling is not None and not isinstance(format, Same):
            ops.dynamic_float_check(format, *self._scaling[:2], what="CastTo.set_format on a scaled cast")
            if self._block_scale is not None:
                ops.block_scaled_check(format, self._scaling[1], *self._block_scale, what="CastTo.set_format on a scaled cast")
        if self._learnable is not None and not isinstance(format, Same):
            f_ = ops.dynamic_check(format, self._learnable["granularity"], self._learnable["group_size"], what="CastTo.set_format on a learnable cast")[0]
            if f_.rounding != "nearest":
                raise ValueError(f"CastTo.set_format on a learnable cast: a learned step size is defined for nearest rounding, got {f_!r}")
        self.format = format
        if hasattr(self, "activation_post_process"):
            self.activation_post_process.dtype = format
            from .observer import get_qmin_qmax
            self.activation_post_process.quant_min, self.activation_post_process.quant_max = get_qmin_qmax(format)

    @property
    def dtype(self):
        return self.format

    def set_pre_transform(self, pre_transform: Dict):
        self.pre_transform = dict(pre_transform)
        if isinstance(self.pre_transform.get("format"), str):
            self.pre_transform["format"] = Format.from_shorthand(self.pre_transform["format"])
        if "hadamard" in self.pre_transform:
            # an orthonormal block-Hadamard rotation along block_dim around the cast (ops.hadamard_qdq): 64, or
            # {"size": 64, "inverse": False} to leave the result in the rotated basis; a bad size raises ValueError here
            self.pre_transform["hadamard"] = _parse_hadamard(self.pre_transform["hadamard"])
            if self._learnable is not None:
                self.pre_transform.pop("hadamard")
                raise ValueError(_LEARNABLE_HADAMARD)
            if self._codebook is not None:
                self.pre_transform.pop("hadamard")
                raise ValueError(_CODEBOOK_HADAMARD)
            if self._vq is not None:
                self.pre_transform.pop("hadamard")
                raise ValueError(_VQ_HADAMARD)

    def set_dynamic(self, granularity=None, group_size=None):
        """Dynamic scales (not in the reference): with fake-quant on and the observer off, an integer format is cast with a
        scale and zero point derived from the tensor itself on every forward (ops.dynamic_fixed_qdq; this cast's qscheme decides symmetric
        or affine) -- one per row of the last dimension ("per_token"; per output channel of an [out, in] weight), per `group_size`
        consecutive elements of it ("per_group", or {"per_group": g}) or for the whole tensor ("per_tensor").  The scale / zero_point
        buffers and the observer are neither read nor written.  None switches back to the stored scales.  While the observer is enabled the
        calibration path runs as ever.  ValueError for an unknown granularity and for a format without an integer range -- here, or in
        set_format when the format comes later (a cast that is still SAME accepts the setting).
        Outliers (DESIGN.md §8 "Outlier-aware dynamic cast"): {"per_group": g, "outliers": k} or {"granularity": "per_token", "outliers": k},
        each optionally with "outlier_format" (None: the value itself; or a per-element FloatingPoint format), keep every segment's k largest
        magnitudes at that precision and derive the scale from the rest (ops.outlier_fixed_qdq); "outliers": 0 is the plain setting."""
        granularity, out = _parse_outliers(granularity)
        dyn = _parse_dynamic(granularity, group_size)
        if dyn is not None and self._codebook is not None:
            raise ValueError("CastTo.set_dynamic: " + _CODEBOOK_EXCLUSIVE)
        if dyn is not None and self._vq is not None:
            raise ValueError("CastTo.set_dynamic: " + _VQ_EXCLUSIVE)
        if dyn is not None and self._learnable is not None:
            raise ValueError("CastTo.set_dynamic: this cast has learned scales (set_learnable), an exclusive source: set_learnable(None) first")
        if dyn is not None:
            if isinstance(self.format, Same):
                ops.dynamic_check("XP[8,0](CSN)", *dyn, what="CastTo.set_dynamic")   # (the granularity alone)
            else:
                ops.dynamic_check(self.format, *dyn, what="CastTo.set_dynamic")
        if out is not None:
            _, _, k_, ofmt_ = ops.outlier_check("XP[8,0](CSN)" if isinstance(self.format, Same) else self.format, dyn[1], out["k"],
                                                   out["outlier_format"], dyn[0], what="CastTo.set_dynamic")
            out = {"k": k_, "outlier_format": ofmt_} if k_ else None
        self._dynamic = dyn
        self._outliers = out

    @property
    def dynamic(self):
        """None, "per_token", "per_tensor" or {"per_group": g} (set_dynamic); with outliers set, the dict {"per_group": g, "outliers": k} or
        {"granularity": "per_token", "outliers": k}, with "outlier_format" (its shorthand) where one is set"""
        dyn = self._dynamic
        if dyn is None:
            return None
        if self._outliers is not None:
            d = {"per_group": dyn[1]} if dyn[0] == "per_group" else {"granularity": dyn[0]}
            d["outliers"] = self._outliers["k"]
            if self._outliers["outlier_format"] is not None:
                d["outlier_format"] = repr(self._outliers["outlier_format"])
            return d
        return {"per_group": dyn[1]} if dyn[0] == "per_group" else dyn[0]

    def _dynamic_cast(self, x, out_dtype):
        g, gs = self._dynamic
        if self._outliers is not None:
            return ops.outlier_fixed_qdq(x, self.format, gs, self._outliers["k"], symmetric_qscheme=self.qscheme in _SYMMETRIC,
                                         outlier_format=self._outliers["outlier_format"], granularity=g, out_dtype=out_dtype)
        return ops.dynamic_fixed_qdq(x, self.format, g, gs, symmetric_qscheme=self.qscheme in _SYMMETRIC, out_dtype=out_dtype)

    # ------------------------------------------------------------------ learned step size (LSQ / LSQ+)
    def set_learnable(self, granularity=None, group_size=None, learn_zero_point: bool = False, grad_scale="lsq", init: str = "minmax",
                      like: Optional[torch.Tensor] = None):
        """Learned step size (LSQ, Esser et al. 2020; LSQ+, Bhalgat et al. 2020; not in the reference): with fake-quant on
        and the observer off, an integer format is cast with a scale and a zero point that are nn.Parameters of this cast --
        `learned_scale` and `learned_zero_point`, float32 [n_segments], the second trained only with learn_zero_point -- through
        ops.lsq_fixed_qdq: the forward is the static affine cast with those values, the backward clips the gradient of x to the
        integer range and gives the parameters theirs (grad_scale: "lsq" = 1 / sqrt(segment * qmax), None, or a float).  Segments as in
        set_dynamic: "per_token" (per output channel of an [out, in] weight), "per_group" with group_size (or {"per_group": g}),
        "per_tensor".  The parameters are registered HERE and nowhere else: an untouched cast keeps its four buffers.
        like: the tensor this cast will see (DmxModule passes its weight): it fixes n_segments.  Without it only "per_tensor" is
        possible -- an activation's per-token or per-group scales have no fixed shape to register: ValueError.
        init: "minmax" -- the (scale, zero point) ops.dynamic_fixed_qdq derives for the tensor, so the first forward equals the dynamic
        cast of the same granularity bit for bit; "lsq" -- s = 2 mean|x| / sqrt(qmax), z = 0.  From `like` at once where it lives on the
        GPU, else from the first tensor the cast sees (in place, under no_grad; a host flag guards it, which loading a state_dict that
        carries the parameters clears).
        Exclusive with set_dynamic and set_scaling, and with a "hadamard" pre_transform, whose fused rotated cast reads the stored
        scale buffers (ValueError in either order).  None removes the parameters and returns to the
        stored scales.  While the observer is enabled the calibration path runs as ever."""
        lrn = _parse_dynamic(granularity, group_size)
        if lrn is None:
            for n in ("learned_scale", "learned_zero_point"):
                if n in self._parameters:
                    del self._parameters[n]
            self._learnable, self._learnable_pending = None, False
            return
        if "hadamard" in self.pre_transform:
            raise ValueError(_LEARNABLE_HADAMARD)
        if self._codebook is not None:
            raise ValueError("CastTo.set_learnable: " + _CODEBOOK_EXCLUSIVE)
        if self._vq is not None:
            raise ValueError("CastTo.set_learnable: " + _VQ_EXCLUSIVE)
        if self._dynamic is not None or self._scaling is not None:
            raise ValueError("CastTo.set_learnable: this cast derives its scales from every tensor (set_dynamic / set_scaling); a learned "
                             "scale is a third, exclusive source: switch that off first")
        fmt = "XP[8,0](CSN)" if isinstance(self.format, Same) else self.format   # (SAME: the granularity alone)
        fmt, g, gs = ops.dynamic_check(fmt, *lrn, what="CastTo.set_learnable")
        if fmt.rounding != "nearest":
            raise ValueError(f"CastTo.set_learnable: a learned step size is defined for nearest rounding, got {fmt!r}")
        if init not in ("minmax", "lsq"):
            raise ValueError(f"CastTo.set_learnable: init must be 'minmax' or 'lsq', got {init!r}")
        if not isinstance(learn_zero_point, bool):
            raise ValueError(f"CastTo.set_learnable: learn_zero_point must be a bool, got {learn_zero_point!r}")
        ops.lsq_grad_factor(grad_scale, 1, 1)   # (ValueError for a bad spelling)
        if like is None:
            if g != "per_tensor":
                raise ValueError(f"CastTo.set_learnable: {g!r} needs like= (the tensor this cast will see, e.g. a weight): the learned scales "
                                 "are parameters of a fixed shape, and a per-token or per-group scale of an activation has none -- "
                                 "activation casts take 'per_tensor' only")
            n_seg, dev = 1, self.scale.device
        else:
            if like.dim() < 1 or like.numel() == 0:
                raise ValueError("CastTo.set_learnable: like must be a non-empty tensor with at least one dimension")
            if g == "per_group" and like.shape[-1] % gs:
                raise ValueError(f"CastTo.set_learnable: the last dimension of like has {like.shape[-1]} elements, not a multiple of the "
                                 f"group size {gs}")
            n_seg = {"per_token": like.numel() // like.shape[-1], "per_group": like.numel() // (gs or 1), "per_tensor": 1}[g]
            dev = like.device
        self._learnable = {"granularity": g, "group_size": gs, "learn_zero_point": learn_zero_point, "grad_scale": grad_scale, "init": init}
        self.register_parameter("learned_scale", torch.nn.Parameter(torch.ones(n_seg, dtype=torch.float32, device=dev)))
        self.register_parameter("learned_zero_point", torch.nn.Parameter(torch.zeros(n_seg, dtype=torch.float32, device=dev),
                                                                         requires_grad=learn_zero_point))
        self._learnable_pending = True
        if like is not None and like.is_cuda and not isinstance(self.format, Same):
            self._learnable_init(like)

    @property
    def learnable(self):
        """None, or the setting: {"granularity": "per_token" | "per_tensor" | {"per_group": g}, "learn_zero_point", "grad_scale", "init"}"""
        lrn = self._learnable
        if lrn is None:
            return None
        g = {"per_group": lrn["group_size"]} if lrn["granularity"] == "per_group" else lrn["granularity"]
        return {"granularity": g, "learn_zero_point": lrn["learn_zero_point"], "grad_scale": lrn["grad_scale"], "init": lrn["init"]}

    def _learnable_init(self, x):
        """fills learned_scale / learned_zero_point in place from the tensor x (set_learnable's init rules); nothing is read back"""
        from .observer import get_qmin_qmax
        lrn = self._learnable
        g, gs = lrn["granularity"], lrn["group_size"]
        with torch.no_grad():
            xd = x.detach()
            if lrn["init"] == "minmax":
                _, sc, zp = ops.dynamic_fixed_qdq(xd, self.format, g, gs, symmetric_qscheme=self.qscheme in _SYMMETRIC, return_qparams=True)
                zp = zp.float()
            else:
                S = {"per_token": xd.shape[-1], "per_group": gs, "per_tensor": xd.numel()}[g]
                sc = xd.reshape(-1, S).float().abs().mean(dim=1) * (2.0 / float(get_qmin_qmax(self.format)[1]) ** 0.5)
                zp = torch.zeros_like(sc)
            if sc.numel() != self.learned_scale.numel():
                raise ValueError(f"CastTo: the learned scales were registered for {self.learned_scale.numel()} segments, this tensor has "
                                 f"{sc.numel()} ({g}, shape {tuple(x.shape)})")
            self.learned_scale.data.copy_(sc.reshape(self.learned_scale.shape))
            self.learned_zero_point.data.copy_(zp.reshape(self.learned_zero_point.shape))
        self._learnable_pending = False

    def _learnable_cast(self, x, out_dtype):
        lrn = self._learnable
        if self._learnable_pending:
            self._learnable_init(x)
        with torch.no_grad():
            self.learned_scale.data.clamp_(min=_LEARNED_SCALE_MIN)
        return ops.lsq_fixed_qdq(x, self.learned_scale, self.learned_zero_point, self.format, lrn["granularity"], lrn["group_size"],
                                 grad_scale=lrn["grad_scale"], out_dtype=out_dtype)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        cb = self._codebook
        if cb is not None and prefix + "codebook" in state_dict:   # (load time: the host copy of the setting follows the loaded values)
            lv = state_dict[prefix + "codebook"].detach().float().cpu()
            if cb["name"] is not None and lv.tolist() != list(ops.codebook_check(cb["name"])[0]):
                cb["name"] = None
            if prefix + "codebook_norm" in state_dict:
                v = float(state_dict[prefix + "codebook_norm"].detach().float().cpu().reshape(-1)[0])
                cb["norm"] = v if v > 0.0 else None
        vq = self._vq
        if vq is not None and prefix + "vq_codebook" in state_dict:   # (the same for a vector codebook: a loaded table is no longer the grid)
            if vq["grid"] is not None and not torch.equal(state_dict[prefix + "vq_codebook"].detach().float().cpu(), ops.vq_grid(*vq["grid"])):
                vq["grid"] = None
            if prefix + "vq_norm" in state_dict:
                v = float(state_dict[prefix + "vq_norm"].detach().float().cpu().reshape(-1)[0])
                vq["norm"] = v if v > 0.0 else None
        if self._learnable is not None and prefix + "learned_scale" in state_dict:
            self._learnable_pending = False   # (the loaded values are the initial values)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def set_scaling(self, granularity=None, group_size=None, pow2_scale: bool = False):
        """Dynamic float scales (not in the reference): with fake-quant on and the observer off, a FloatingPoint format is
        cast as float_q(x / s) * s with s = the segment's absolute maximum over the format's largest value, derived from the tensor
        itself on every forward (ops.dynamic_float_qdq) -- one per row of the last dimension ("per_token"; per output channel of an
        [out, in] weight), per `group_size` consecutive elements of it ("per_group", or {"per_group": g}), per group_size x group_size
        tile of the last two dimensions ("per_tile", or {"per_tile": g}) or for the whole tensor ("per_tensor"); pow2_scale rounds s up
        to a power of two.  A setting of its own beside set_dynamic (the integer formats'): a plain attribute, no buffer, no state_dict
        key; None switches back to the unscaled cast.  ValueError for an unknown granularity and for a format that cannot be scaled (not
        a FloatingPoint, unsigned, 8 exponent bits) -- here, or in set_format when the format comes later (a cast that is still SAME
        accepts the setting).
        Quantised group scales (ops.block_scaled_float_qdq): the dict form {"per_group": g, "scale_format": Sf} with, optionally,
        "scale_max" and "tensor_scale" ("dynamic" -- the default --, None, a float or a one-element tensor) casts every group's scale to
        the float format Sf under one float32 scale per tensor -- ops.NVFP4 is the ready setting for FP[1|2|1,1](_N).  These keys go with
        per_group only and not with pow2_scale: ValueError otherwise."""
        granularity, block = _split_block_scale(granularity)
        sc = _parse_scaling(granularity, group_size, pow2_scale)
        if sc is not None and self._codebook is not None:
            raise ValueError("CastTo.set_scaling: " + _CODEBOOK_EXCLUSIVE)
        if sc is not None and self._vq is not None:
            raise ValueError("CastTo.set_scaling: " + _VQ_EXCLUSIVE)
        if sc is not None and self._learnable is not None:
            raise ValueError("CastTo.set_scaling: this cast has learned scales (set_learnable), an exclusive source: set_learnable(None) first")
        if block is not None:
            if sc is None or sc[0] != "per_group":
                raise ValueError(f"set_scaling: scale_format / scale_max / tensor_scale quantise the scales of GROUPS: give "
                                 f"{{'per_group': g}} with them (got granularity {None if sc is None else sc[0]!r}), or drop them")
            if sc[2]:
                raise ValueError("set_scaling: pow2_scale and scale_format are two different scale rules: drop pow2_scale (a power-of-two "
                                 "scale format is FP[1|e|0,bias]) or drop scale_format")
        if sc is not None:
            fmt = "FP[1|4|3,7](FN)" if isinstance(self.format, Same) else self.format   # (SAME: the granularity alone)
            ops.dynamic_float_check(fmt, *sc[:2], what="CastTo.set_scaling")
            if block is not None:
                _, _, smax = ops.block_scaled_check(fmt, sc[1], block["scale_format"], block.get("scale_max"),
                                                    block.get("tensor_scale", "dynamic"), what="CastTo.set_scaling")
                block = (block["scale_format"], smax, block.get("tensor_scale", "dynamic"))
        self._scaling, self._block_scale = sc, block

    @property
    def scaling(self):
        """None, or the setting in configure's spelling: "per_token", "per_tensor", {"per_group": g} or {"per_tile": g}; as a dict with
        "pow2_scale": True where that is set ({"granularity": "per_token", "pow2_scale": True})"""
        sc = self._scaling
        if sc is None:
            return None
        g, gs, pow2 = sc
        if self._block_scale is not None:
            sf, smax, ts = self._block_scale
            return {"per_group": gs, "scale_format": sf if isinstance(sf, str) else repr(sf), "scale_max": smax, "tensor_scale": ts}
        out = {g: gs} if g in ("per_group", "per_tile") else g
        if pow2:
            out = dict(out, pow2_scale=True) if isinstance(out, dict) else {"granularity": g, "pow2_scale": True}
        return out

    def _scaled_cast(self, x, out_dtype):
        g, gs, pow2 = self._scaling
        if self._block_scale is not None:
            sf, smax, ts = self._block_scale
            return ops.block_scaled_float_qdq(x, self.format, gs, sf, smax, ts, out_dtype=out_dtype)
        return ops.dynamic_float_qdq(x, self.format, g, gs, pow2_scale=pow2, out_dtype=out_dtype)

    # ------------------------------------------------------------------ codebook casts
    def set_codebook(self, setting=None):
        """Codebook cast (not in the reference; DESIGN.md §8 "Codebook casts"): with fake-quant on and the observer off, the tensor is cast
        onto a small table of levels under a per-segment absolute-maximum scale (ops.codebook_qdq) IN PLACE of the format's arithmetic; a
        SAME cast stays the identity.  setting: None, or a dict {"codebook": a name of ops.CODEBOOKS | a list / tensor of levels,
        "per_group": g | "granularity": "per_token" / "per_tensor" / "per_group" (with "group_size"), "norm": None or a positive number} such
        as ops.NF4.  The table is registered HERE as the float32 buffer `codebook` [K], beside `codebook_norm` [1] (the pinned norm, 0 for
        none), so that a fitted table (fit_codebook) is saved and loaded with the module -- into a cast that was given a table of the same
        size; None removes both, and an untouched cast keeps its four buffers.  Exclusive with set_dynamic, set_scaling,
        set_learnable and a "hadamard" pre_transform (ValueError in either order).  ValueError for everything ops.codebook_check refuses."""
        if setting is None:
            for n in ("codebook", "codebook_norm"):
                if n in self._buffers:
                    del self._buffers[n]
            self._codebook = None
            return
        if not isinstance(setting, dict) or "codebook" not in setting or not set(setting) <= {"codebook", "per_group", "granularity", "group_size", "norm"}:
            raise ValueError(f"set_codebook: expected None or a dict with 'codebook' and optionally 'per_group' / 'granularity' / 'group_size' / "
                             f"'norm' (such as ops.NF4), got {setting!r}")
        if "per_group" in setting:
            if setting.get("granularity", "per_group") != "per_group" or "group_size" in setting:
                raise ValueError(f"set_codebook: 'per_group' names the granularity and its group size by itself, got {setting!r}")
            g, gs = "per_group", setting["per_group"]
        else:
            g, gs = setting.get("granularity", "per_group"), setting.get("group_size", 64 if setting.get("granularity", "per_group") == "per_group" else None)
            if g != "per_group" and gs is not None:
                raise ValueError(f"set_codebook: group_size goes with granularity 'per_group', got {setting!r}")
        levels, g, gs, norm = ops.codebook_check(setting["codebook"], g, gs, setting.get("norm"), what="CastTo.set_codebook")
        if self._vq is not None:
            raise ValueError("CastTo.set_codebook: " + _VQ_EXCLUSIVE)
        if self._dynamic is not None or self._scaling is not None or self._learnable is not None:
            raise ValueError("CastTo.set_codebook: this cast already takes its scales from set_dynamic / set_scaling / set_learnable; a codebook "
                             "replaces the format's arithmetic and is exclusive with them: switch that off first")
        if "hadamard" in self.pre_transform:
            raise ValueError(_CODEBOOK_HADAMARD)
        t = levels.detach().to(torch.float32).clone() if isinstance(levels, torch.Tensor) else torch.tensor(levels, dtype=torch.float32)
        for n in ("codebook", "codebook_norm"):
            if n in self._buffers:
                del self._buffers[n]
        self.register_buffer("codebook", t.to(t.device if t.is_cuda else self.scale.device))
        # the pinned norm travels with the table (0: none pinned, the table's own largest magnitude); the cast itself reads the host copy
        self.register_buffer("codebook_norm", torch.tensor([0.0 if norm is None else norm], dtype=torch.float32, device=self.codebook.device))
        self._codebook = {"granularity": g, "group_size": gs, "norm": norm,
                          "name": setting["codebook"] if isinstance(setting["codebook"], str) else None}

    @property
    def codebook_setting(self):
        """None, or the setting in the spelling set_codebook accepts: {"codebook": the name it was set by, or the buffer's levels as a
        list, "per_group": g | "granularity": ..., and "norm" where one is pinned}.  A fitted table reads back as its levels."""
        cb = self._codebook
        if cb is None:
            return None
        out = {"codebook": cb["name"] if cb["name"] is not None else self.codebook.detach().cpu().tolist()}
        out.update({"per_group": cb["group_size"]} if cb["granularity"] == "per_group" else {"granularity": cb["granularity"]})
        if cb["norm"] is not None:
            out["norm"] = cb["norm"]
        return out

    def fit_codebook(self, x, iters: int = 8):
        """replaces the table IN PLACE by ops.codebook_fit's result for the tensor x (or list of tensors), started from the current table,
        and pins the norm the fit used: the cast then reproduces the fitted error.  -> the buffer"""
        if self._codebook is None:
            raise ValueError("CastTo.fit_codebook: no codebook is set (set_codebook first)")
        cb = self._codebook
        first = x[0] if isinstance(x, (list, tuple)) else x
        if self.codebook.device != first.device:
            self.codebook = self.codebook.to(first.device)
        c, norm = ops.codebook_fit(x, self.codebook, cb["granularity"], cb["group_size"], cb["norm"], iters=iters)
        with torch.no_grad():
            self.codebook.copy_(c)
            self.codebook_norm.fill_(norm)
        cb["norm"], cb["name"] = norm, None
        return self.codebook

    def _codebook_cast(self, x, out_dtype):
        cb = self._codebook
        c = self.codebook if self.codebook.device == x.device else self.codebook.to(x.device)
        return ops.codebook_qdq(x, c, cb["granularity"], cb["group_size"], cb["norm"], out_dtype=out_dtype)

    # ------------------------------------------------------------------ vector codebook casts
    def set_vq(self, setting=None):
        """Vector codebook cast (not in the reference; DESIGN.md §8 "Vector codebook casts"): with fake-quant on and the observer off, every
        d consecutive elements of the last dimension are replaced together by one row of a [K, d] table under a per-segment
        absolute-maximum scale (ops.vq_qdq) IN PLACE of the format's arithmetic; a SAME cast stays the identity.  setting: None, or a dict
        {"codebook": a list of rows | a [K, d] tensor | {"grid": levels, "dim": d} (ops.vq_grid), "per_group": g | "granularity":
        "per_token" / "per_tensor" / "per_group" (with "group_size"), "norm": None or a positive number}.  The table is registered HERE as
        the float32 buffer `vq_codebook` [K, d], beside `vq_norm` [1] (the pinned norm, 0 for none), so that a fitted table (fit_vq) is
        saved and loaded with the module -- into a cast that was given a table of the same shape; None removes both.  Exclusive with
        set_codebook, set_dynamic, set_scaling, set_learnable and a "hadamard" pre_transform (ValueError in either order).  ValueError for
        everything ops.vq_check refuses."""
        if setting is None:
            for n in ("vq_codebook", "vq_norm"):
                if n in self._buffers:
                    del self._buffers[n]
            self._vq = None
            return
        if not isinstance(setting, dict) or "codebook" not in setting or not set(setting) <= {"codebook", "per_group", "granularity", "group_size", "norm"}:
            raise ValueError(f"set_vq: expected None or a dict with 'codebook' and optionally 'per_group' / 'granularity' / 'group_size' / "
                             f"'norm', got {setting!r}")
        if "per_group" in setting:
            if setting.get("granularity", "per_group") != "per_group" or "group_size" in setting:
                raise ValueError(f"set_vq: 'per_group' names the granularity and its group size by itself, got {setting!r}")
            g, gs = "per_group", setting["per_group"]
        else:
            g, gs = setting.get("granularity", "per_group"), setting.get("group_size", 64 if setting.get("granularity", "per_group") == "per_group" else None)
            if g != "per_group" and gs is not None:
                raise ValueError(f"set_vq: group_size goes with granularity 'per_group', got {setting!r}")
        table, K, d, g, gs, norm = ops.vq_check(setting["codebook"], None, g, gs, setting.get("norm"), what="CastTo.set_vq")
        if self._codebook is not None:
            raise ValueError("CastTo.set_vq: " + _CODEBOOK_EXCLUSIVE)
        if self._dynamic is not None or self._scaling is not None or self._learnable is not None:
            raise ValueError("CastTo.set_vq: this cast already takes its scales from set_dynamic / set_scaling / set_learnable; a vector "
                             "codebook replaces the format's arithmetic and is exclusive with them: switch that off first")
        if "hadamard" in self.pre_transform:
            raise ValueError(_VQ_HADAMARD)
        t = table.detach().to(torch.float32).clone() if isinstance(table, torch.Tensor) else torch.tensor(table, dtype=torch.float32)
        for n in ("vq_codebook", "vq_norm"):
            if n in self._buffers:
                del self._buffers[n]
        self.register_buffer("vq_codebook", t.to(t.device if t.is_cuda else self.scale.device))
        # the pinned norm travels with the table (0: none pinned, the table's own largest magnitude); the cast itself reads the host copy
        self.register_buffer("vq_norm", torch.tensor([0.0 if norm is None else norm], dtype=torch.float32, device=self.vq_codebook.device))
        grid = setting["codebook"] if isinstance(setting["codebook"], dict) else None
        self._vq = {"granularity": g, "group_size": gs, "norm": norm,
                    "grid": (grid["grid"] if isinstance(grid["grid"], str) else tuple(grid["grid"]), grid["dim"]) if grid is not None else None}

    @property
    def vq_setting(self):
        """None, or the setting in the spelling set_vq accepts: {"codebook": the grid it was set by, or the buffer's rows as a list of
        lists, "per_group": g | "granularity": ..., and "norm" where one is pinned}.  A fitted table reads back as its rows."""
        vq = self._vq
        if vq is None:
            return None
        grid = vq["grid"]
        out = {"codebook": {"grid": grid[0] if isinstance(grid[0], str) else list(grid[0]), "dim": grid[1]} if grid is not None
               else self.vq_codebook.detach().cpu().tolist()}
        out.update({"per_group": vq["group_size"]} if vq["granularity"] == "per_group" else {"granularity": vq["granularity"]})
        if vq["norm"] is not None:
            out["norm"] = vq["norm"]
        return out

    def fit_vq(self, x, iters: int = 8):
        """replaces the table IN PLACE by ops.vq_fit's result for the tensor x (or list of tensors), started from the current table, and
        pins the norm the fit used: the cast then reproduces the fitted error.  -> the buffer"""
        if self._vq is None:
            raise ValueError("CastTo.fit_vq: no vector codebook is set (set_vq first)")
        vq = self._vq
        first = x[0] if isinstance(x, (list, tuple)) else x
        if self.vq_codebook.device != first.device:
            self.vq_codebook = self.vq_codebook.to(first.device)
            self.vq_norm = self.vq_norm.to(first.device)
        c, norm = ops.vq_fit(x, codebook=self.vq_codebook, granularity=vq["granularity"], group_size=vq["group_size"], norm=vq["norm"], iters=iters)
        with torch.no_grad():
            self.vq_codebook.copy_(c)
            self.vq_norm.fill_(norm)
        vq["norm"], vq["grid"] = norm, None
        return self.vq_codebook

    def _vq_cast(self, x, out_dtype):
        vq = self._vq
        c = self.vq_codebook if self.vq_codebook.device == x.device else self.vq_codebook.to(x.device)
        return ops.vq_qdq(x, c, vq["granularity"], vq["group_size"], vq["norm"], out_dtype=out_dtype)

    def enable_calibration(self, state: bool = True, observer_cls: ObserverBase = HistogramObserver,
                           qscheme_to_overload: Optional[torch.qscheme] = None, group_size: int = None,
                           ch_axis: int = None) -> None:
        """cast.py:308-340: install an observer and switch to observe-only, or back to fake-quant."""
        if state:
            if ch_axis is not None:
                self.ch_axis = ch_axis
            if qscheme_to_overload is not None:
                self.qscheme = qscheme_to_overload
                self.is_per_channel = qscheme_to_overload in _PER_CHANNEL
            self.group_size = group_size if group_size else None
            if self.group_size:
                assert not self.is_per_channel, "group quantization is to be used with per tensor quantization"
            self.activation_post_process = observer_cls(dtype=self.format, qscheme=self.qscheme, ch_axis=self.ch_axis)
            self._group_observers = []
            self.disable_fake_quant()
            self.enable_observer()
        else:
            self.enable_fake_quant()
            self.disable_observer()
            if isinstance(self.activation_post_process, HistogramObserver):
                self.activation_post_process.check_finite()   # the device path's delayed raise

    # ------------------------------------------------------------------ forward pieces
    def _observer_step(self, x):
        """cast.py:179-226, all groups in one reduction launch."""
        obs = self.activation_post_process
        obs.ch_axis = self.ch_axis
        obs.qscheme = self.qscheme
        if self.group_size and isinstance(obs, HistogramObserver) and obs.device_path_ok(x, self.group_size):
            # every slab's histogram in one observer and one call (dmxq_hist_observe), the searches in one launch
            obs(x.detach(), self.group_size)
            _scale, _zero_point = obs.calculate_qparams()
        elif self.group_size and not isinstance(obs, (MinMaxObserver, DummyObserver)):
            # per-tensor-only observers (the histogram's host code): one instance per slab, as cast.py:185-213 does for every class
            slabs = torch.split(x.detach(), self.group_size, dim=self.ch_axis)
            if len(getattr(self, "_group_observers", ())) != len(slabs):
                self._group_observers = [obs.__class__(dtype=self.format, qscheme=self.qscheme, ch_axis=self.ch_axis)
                                         for _ in slabs]
            qp = []
            for o, slab in zip(self._group_observers, slabs):
                o(slab)
                qp.append(o.calculate_qparams())
            _scale = torch.cat([s.reshape(1) for s, _ in qp])
            _zero_point = torch.cat([z.reshape(1) for _, z in qp])
            obs.min_val = torch.stack([o.min_val.reshape(()) for o in self._group_observers])
            obs.max_val = torch.stack([o.max_val.reshape(()) for o in self._group_observers])
        else:
            obs(x.detach(), self.group_size) if isinstance(obs, MinMaxObserver) else obs(x.detach())
            _scale, _zero_point = obs.calculate_qparams()
        _scale, _zero_point = _scale.to(x.device), _zero_point.to(x.device)
        if self.scale.shape != _scale.shape or self.scale.device != _scale.device:
            self.scale = torch.zeros_like(_scale)
            self.zero_point = torch.zeros_like(_zero_point)
        self.scale.copy_(_scale)
        self.zero_point.copy_(_zero_point)

    @staticmethod
    def apply_shaping_seq(x, shaping_list):
        """cast.py:239-259: view / permute / flatten sequence and its inverse."""
        inverse = []
        for op, args in shaping_list:
            orig = x.size()
            if op == "view":
                x = x.reshape(*args)
                inverse.append(("view", orig))
            elif op == "permute":
                x = x.permute(*args)
                inverse.append(("permute", torch.LongTensor(list(args)).argsort().tolist()))
            elif op == "flatten":
                x = x.flatten(*args)
                inverse.append(("view", orig))
            else:
                raise Exception(f"unknown shape op {op}")
        return x, inverse[::-1]

    def _quantize(self, x, out_dtype):
        fmt = self.format
        # the autograd wrappers only matter when a gradient will flow (straight-through estimator); inference skips them
        ste = torch.is_grad_enabled() and x.requires_grad
        if self._codebook is not None and not self.__dict__["_h_observer_enabled"]:
            return self._codebook_cast(x, out_dtype)  # (a straight-through estimator under autograd by itself)
        if self._vq is not None and not self.__dict__["_h_observer_enabled"]:
            return self._vq_cast(x, out_dtype)        # (the same)
        if self._dynamic is not None and isinstance(fmt, FixedPoint) and not self.__dict__["_h_observer_enabled"]:
            return self._dynamic_cast(x, out_dtype)   # (a straight-through estimator under autograd by itself)
        if self._scaling is not None and isinstance(fmt, FloatingPoint) and not self.__dict__["_h_observer_enabled"]:
            return self._scaled_cast(x, out_dtype)    # (the same)
        if self._learnable is not None and isinstance(fmt, FixedPoint) and not self.__dict__["_h_observer_enabled"]:
            return self._learnable_cast(x, out_dtype)   # (ops.lsq_fixed_qdq: an autograd Function with the LSQ backward)
        if isinstance(fmt, FixedPoint):
            # per-tensor: one scale; per-channel: scale[c]; per-group: scale[c // group_size] (cast.py:279-293)
            if self.group_size:
                ch_axis, gs = self.ch_axis, self.group_size
            elif self.is_per_channel:
                ch_axis, gs = self.ch_axis, None
            else:
                ch_axis, gs = None, None
            if ste:
                return _FixedAffineCast.apply(x, fmt, self.scale, self.zero_point, ch_axis, gs, out_dtype)
            return ops.fixed_qdq(x, fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=self.scale,
                                 zero_point=self.zero_point, ch_axis=ch_axis, group_size=gs, out_dtype=out_dtype)
        if ste:
            return CastToFormat.apply(x, fmt, self.block_dim, out_dtype)
        if self.keep_layout and x.dim() > 1 and not x.is_contiguous() and not torch.compiler.is_compiling():
            order = sorted(range(x.dim()), key=lambda d: (-x.stride(d), d))
            xp = x.permute(order)
            if xp.is_contiguous():
                y = fmt.cast(xp, order.index(self.block_dim % x.dim()), out_dtype=out_dtype)
                inv = [0] * len(order)
                for i, d in enumerate(order):
                    inv[d] = i
                return y.permute(inv)
        return fmt.cast(x, self.block_dim, out_dtype=out_dtype)

    # ------------------------------------------------------------------ hadamard pre_transform
    def _hadamard_qdq(self, x, had, out_dtype):
        """rotate -> this cast with its current scale / zero point -> [rotate back] as ONE ops.hadamard_qdq call (one launch where the
        fused kernel covers the format)"""
        fmt, kw = self.format, {}
        if isinstance(fmt, FixedPoint):
            kw = {"scale": self.scale, "zero_point": self.zero_point}
            if self.group_size:
                kw.update(ch_axis=self.ch_axis, group_size=self.group_size)
            elif self.is_per_channel:
                if x.dim() == 2 and self.ch_axis % 2 == 0 and self.block_dim % 2 == 1:
                    kw["per_row"] = True   # (per output channel of a [rows, L] weight rotated along its rows: the fused kernel's case)
                else:
                    kw["ch_axis"] = self.ch_axis
        return ops.hadamard_qdq(x, had["size"], fmt, self.block_dim, had["inverse"], out_dtype=out_dtype, **kw)

    def _rotate_observe_cast(self, x, had):
        """forward's steps rotation -> observer step (on the rotated float32 tensor: scales are calibrated in the rotated basis) -> cast
        -> inverse rotation.  With fake-quant off nothing is cast: the input comes back as it is (inverse) or rotated (no inverse)."""
        d = self.__dict__
        fmt = self.format
        r = ops.hadamard(x, had["size"], self.block_dim, out_dtype=torch.float32)
        if d["_h_observer_enabled"] and not isinstance(fmt, Same):
            self._observer_step(r)
        if not d["_h_fake_quant_enabled"]:
            return x if had["inverse"] else r
        if not isinstance(fmt, Format):
            raise TypeError("CastTo with a torch.dtype format is torch.ao's stock FakeQuantize path, "
                            "not part of the accelerated hot path")
        if not had["inverse"]:
            return self._quantize(r, self.physical_dtype)
        return ops.hadamard(self._quantize(r, torch.float32), had["size"], self.block_dim, out_dtype=self.physical_dtype)

    def forward(self, x):
        d = self.__dict__  # (plain attributes: nn.Module.__setattr__ costs several microseconds per assignment)
        d["physical_dtype"] = x.dtype
        fmt, pt = self.format, self.pre_transform
        if not pt:  # the common case: no shaping / shortcut / pre-format
            same = isinstance(fmt, Same)
            if d["_h_observer_enabled"] and not same:
                self._observer_step(x)
            if not d["_h_fake_quant_enabled"]:
                return x
            if same:  # the reference's Same.cast is x.clone() (format.py:89-90): one full copy per no-op cast
                return x.clone() if self.copy_on_same else x
            if not isinstance(fmt, Format):
                raise TypeError("CastTo with a torch.dtype format is torch.ao's stock FakeQuantize path, "
                                "not part of the accelerated hot path")
            return self._quantize(x, x.dtype)
        had = pt.get("hadamard")
        if had is not None and len(pt) == 1 and d["_h_fake_quant_enabled"] and not d["_h_observer_enabled"] and isinstance(fmt, Format) \
                and not isinstance(fmt, Same) and self._dynamic is None and self._scaling is None:   # (a dynamic / scaled cast: the step-by-step route below)
            return self._hadamard_qdq(x, had, x.dtype)   # rotation, cast and inverse rotation: one call
        inverse_shaping = None
        shortcut = None
        if "shaping" in pt:
            x, inverse_shaping = self.apply_shaping_seq(x, pt["shaping"])
        sc_idx = pt.get("noquant_shortcut")
        if isinstance(sc_idx, list):  # the reference indexes with the list itself (a multi-dim index); spelled as a tuple
            sc_idx = tuple(sc_idx)
        if sc_idx is not None:
            shortcut = x[sc_idx].clone()
        if "format" in pt:
            x = CastToFormat.apply(x, pt["format"], self.block_dim, torch.float32)
        if had is not None:
            if had["inverse"] and torch.is_grad_enabled() and x.requires_grad:
                x = _RotatedSTE.apply(x, self, had)
            else:
                x = self._rotate_observe_cast(x, had)   # (no inverse: the gradient is ops.hadamard(grad) through the pieces' own backward)
        elif d["_h_observer_enabled"] and x is not None and not isinstance(fmt, Same):
            self._observer_step(x)
        if d["_h_fake_quant_enabled"] and had is None:
            if isinstance(fmt, Format):
                x = self._quantize(x, self.physical_dtype)
            else:
                raise TypeError("CastTo with a torch.dtype format is torch.ao's stock FakeQuantize path, "
                                "not part of the accelerated hot path")
        if shortcut is not None:
            x = x.clone() if x.dtype == self.physical_dtype else x.to(self.physical_dtype)
            x[sc_idx] = shortcut.to(x.dtype)
        if inverse_shaping is not None:
            x, _ = self.apply_shaping_seq(x, inverse_shaping)
        return x.to(self.physical_dtype)

    # ------------------------------------------------------------------ error of this cast
    def measure_error(self, x):
        """The row [sum_sq_err, sum_sq_ref, max_abs_err, count] (float64 [4] on x's device, ops.error_stats) between x and what this cast
        makes of it: its format along its block_dim with its current scale / zero point.  Neither the observer nor the switches are
        touched, and nothing is read back to the host.  BFP, FloatingPoint and per-tensor FixedPoint casts are measured without
        materialising the cast (ops.cast_error); per-channel / per-group FixedPoint, and the formats cast_error does not fuse, as this
        cast's own launch followed by ops.error_stats.  A cast whose pre_transform is only "hadamard" is measured as the rotated cast
        (ops.hadamard_qdq) followed by ops.error_stats against x; one with any other pre_transform key is not measured."""
        if self.pre_transform and set(self.pre_transform) != {"hadamard"}:
            raise NotImplementedError("CastTo.measure_error: a cast with a pre_transform other than hadamard (shaping / shortcut / pre-format)")
        fmt, x = self.format, x.detach()
        dyn_cast = self._codebook_cast if self._codebook is not None and isinstance(fmt, Format) and not isinstance(fmt, Same) else \
            self._vq_cast if self._vq is not None and isinstance(fmt, Format) and not isinstance(fmt, Same) else \
            self._dynamic_cast if self._dynamic is not None and isinstance(fmt, FixedPoint) else \
            self._scaled_cast if self._scaling is not None and isinstance(fmt, FloatingPoint) else \
            self._learnable_cast if self._learnable is not None and isinstance(fmt, FixedPoint) else None
        if dyn_cast is not None:
            # a dynamic / scaled / learnable cast: the cast itself (between the two rotations of a "hadamard" pre_transform), then ops.error_stats
            with torch.no_grad():
                had = self.pre_transform.get("hadamard")
                if had is None:
                    y = dyn_cast(x, x.dtype)
                else:
                    r = ops.hadamard(x, had["size"], self.block_dim, out_dtype=torch.float32)
                    y = (ops.hadamard(dyn_cast(r, torch.float32), had["size"], self.block_dim, out_dtype=x.dtype)
                         if had["inverse"] else dyn_cast(r, x.dtype))
            return ops.error_stats(x, y)
        if self.pre_transform:
            had = self.pre_transform["hadamard"]
            with torch.no_grad():
                if isinstance(fmt, Format) and not isinstance(fmt, Same):
                    y = self._hadamard_qdq(x, had, x.dtype)
                else:
                    y = ops.hadamard(x, had["size"], self.block_dim)
                    y = ops.hadamard(y, had["size"], self.block_dim) if had["inverse"] else y
            return ops.error_stats(x, y)
        if not isinstance(fmt, Format) or isinstance(fmt, Same):
            return ops.error_stats(x, x)
        if isinstance(fmt, FixedPoint):
            if self.group_size or self.is_per_channel or self.scale.numel() != 1:
                with torch.no_grad():
                    return ops.error_stats(x, self._quantize(x, x.dtype))
            return ops.cast_error(x, [(fmt, self.scale, self.zero_point)], block_dim=self.block_dim)[0]
        return ops.cast_error(x, [fmt], block_dim=self.block_dim)[0]

    # ------------------------------------------------------------------ introspection
    def get_precision(self) -> Optional[float]:
        if isinstance(self.format, Same):
            if self.physical_dtype is not None:
                return float(torch.finfo(self.physical_dtype).bits)
            return None
        return self.format.bit_precision

    def extra_repr(self):
        return f"format = dtype = {self.format!r}, qscheme = {self.qscheme}, ch_axis = {self.ch_axis}, " \
               f"group_size = {self.group_size}, block_dim = {self.block_dim}" \
               + (f", dynamic = {self.dynamic!r}" if self._dynamic is not None else "") \
               + (f", scaling = {self.scaling!r}" if self._scaling is not None else "") \
               + (f", learnable = {self.learnable!r}" if self._learnable is not None else "") \
               + (f", codebook = {self._codebook_repr()}" if self._codebook is not None else "") \
               + (f", vq = {self._vq_repr()}" if self._vq is not None else "")

    def _vq_repr(self):
        vq = self._vq   # (no device read: a table that is no grid shows its shape)
        grid = vq["grid"]
        out = {"codebook": {"grid": grid[0] if isinstance(grid[0], str) else list(grid[0]), "dim": grid[1]} if grid is not None
               else f"<{self.vq_codebook.shape[0]} rows of {self.vq_codebook.shape[1]}>"}
        out.update({"per_group": vq["group_size"]} if vq["granularity"] == "per_group" else {"granularity": vq["granularity"]})
        if vq["norm"] is not None:
            out["norm"] = vq["norm"]
        return repr(out)

    def _codebook_repr(self):
        cb = self._codebook   # (no device read: a table without a name shows its size)
        out = {"codebook": cb["name"] if cb["name"] is not None else f"<{self.codebook.shape[0]} levels>"}
        out.update({"per_group": cb["group_size"]} if cb["granularity"] == "per_group" else {"granularity": cb["granularity"]})
        if cb["norm"] is not None:
            out["norm"] = cb["norm"]
        return repr(out)


class CastToDict(torch.nn.ModuleDict):
    """Keyed collection of CastTo's applied to a module's positional / keyword tensors (cast.py:58-134)."""

    def forward(self, x, *args, output=False, first_done=False, **kwargs):
        """first_done: `x` already went through its cast (the fused input path of DmxModule.forward)."""
        keys = list(self.keys())
        if output:
            if isinstance(x, (tuple, list)):
                return type(x)(self[keys[i]](a) for i, a in enumerate(x))
            return self[keys[0]](x)
        i = 1
        new_args, new_kwargs = [], {}
        for a in args:
            if isinstance(a, torch.Tensor):
                new_args.append(self[keys[i]](a))
                i += 1
            else:
                new_args.append(a)
        for k, v in kwargs.items():
            new_kwargs[k] = self[k + "_cast"](v) if isinstance(v, torch.Tensor) else v
        return (x if first_done else self[keys[0]](x)), new_args, new_kwargs

    def pack_to_dict(self, param):
        keys = list(self.keys())
        if isinstance(param, (tuple, list)):
            param = {keys[i]: (p if p is not None else "SAME") for i, p in enumerate(param)}
        elif not isinstance(param, dict):
            raise ValueError("format needs to be a dict, tuple or list!")
        if len(param) != len(self):
            warnings.warn(f"length of format to set is not equal to length of input_casts, some CastTos might not "
                          f"be set properly!\nlen({param}!={len(self)})")
        return param

    def set_pre_transform(self, pre_transforms):
        for k, t in self.pack_to_dict(pre_transforms).items():
            self[k].set_pre_transform(t)

    def set_dynamic(self, dynamic):
        """one setting (None, "per_token", "per_tensor", {"per_group": g}, or a dict with "outliers" as CastTo.set_dynamic takes it) for every
        cast, or a list / dict of settings over the casts the way set_pre_transform takes them"""
        one = isinstance(dynamic, dict) and (set(dynamic) == {"per_group"} or ("outliers" in dynamic and set(dynamic) <= {
            "per_group", "granularity", *_OUTLIER_KEYS})) and not set(dynamic) & set(self.keys())
        if dynamic is None or isinstance(dynamic, str) or one:
            for c in self.values():
                c.set_dynamic(dynamic)
            return
        if isinstance(dynamic, (tuple, list)):   # (not pack_to_dict: it spells a None entry "SAME", a format)
            if len(dynamic) != len(self):
                raise ValueError(f"set_dynamic: {len(dynamic)} settings for {len(self)} casts")
            dynamic = dict(zip(self.keys(), dynamic))
        elif not isinstance(dynamic, dict):
            raise ValueError(f"set_dynamic: expected a setting, or a list or dict of settings, got {dynamic!r}")
        for k, t in dynamic.items():
            if k not in self.keys():
                raise RuntimeError(f"No CastTo with key {k}!")
            self[k].set_dynamic(t)

    def set_scaling(self, scaling):
        """one setting (None, "per_token", "per_tensor", {"per_group": g}, {"per_tile": g}, each dict optionally with "pow2_scale"; a
        per_group dict also with "scale_format" / "scale_max" / "tensor_scale", such as ops.NVFP4) for every cast, or a list / dict of settings over the casts the way set_dynamic takes them"""
        one = isinstance(scaling, dict) and set(scaling) <= {"per_group", "per_tile", "granularity", "pow2_scale", *_BLOCK_SCALE_KEYS} \
            and not set(scaling) & set(self.keys())
        if scaling is None or isinstance(scaling, str) or one:
            for c in self.values():
                c.set_scaling(scaling)
            return
        if isinstance(scaling, (tuple, list)):
            if len(scaling) != len(self):
                raise ValueError(f"set_scaling: {len(scaling)} settings for {len(self)} casts")
            scaling = dict(zip(self.keys(), scaling))
        elif not isinstance(scaling, dict):
            raise ValueError(f"set_scaling: expected a setting, or a list or dict of settings, got {scaling!r}")
        for k, t in scaling.items():
            if k not in self.keys():
                raise RuntimeError(f"No CastTo with key {k}!")
            self[k].set_scaling(t)

    def set_codebook(self, codebook):
        """one setting (None, or a dict with "codebook" such as ops.NF4) for every cast, or a list / dict of settings over the casts the
        way set_scaling takes them"""
        one = isinstance(codebook, dict) and "codebook" in codebook and not set(codebook) & set(self.keys())
        if codebook is None or one:
            for c in self.values():
                c.set_codebook(codebook)
            return
        if isinstance(codebook, (tuple, list)):
            if len(codebook) != len(self):
                raise ValueError(f"set_codebook: {len(codebook)} settings for {len(self)} casts")
            codebook = dict(zip(self.keys(), codebook))
        elif not isinstance(codebook, dict):
            raise ValueError(f"set_codebook: expected a setting, or a list or dict of settings, got {codebook!r}")
        for k, t in codebook.items():
            if k not in self.keys():
                raise RuntimeError(f"No CastTo with key {k}!")
            self[k].set_codebook(t)

    def set_vq(self, vq):
        """one setting (None, or a dict with "codebook": rows, a [K, d] tensor or {"grid": ..., "dim": d}) for every cast, or a list / dict
        of settings over the casts the way set_codebook takes them"""
        one = isinstance(vq, dict) and "codebook" in vq and not set(vq) & set(self.keys())
        if vq is None or one:
            for c in self.values():
                c.set_vq(vq)
            return
        if isinstance(vq, (tuple, list)):
            if len(vq) != len(self):
                raise ValueError(f"set_vq: {len(vq)} settings for {len(self)} casts")
            vq = dict(zip(self.keys(), vq))
        elif not isinstance(vq, dict):
            raise ValueError(f"set_vq: expected a setting, or a list or dict of settings, got {vq!r}")
        for k, t in vq.items():
            if k not in self.keys():
                raise RuntimeError(f"No CastTo with key {k}!")
            self[k].set_vq(t)

    def set_format(self, format):
        for k, f in self.pack_to_dict(format).items():
            if k not in self.keys():
                raise RuntimeError(f"No CastTo with key {k}!")
            self[k].set_format(f)

    def disable_fake_quant(self):
        for c in self.values():
            c.disable_fake_quant()

    def enable_fake_quant(self):
        for c in self.values():
            c.enable_fake_quant()

    def enable_observer(self):
        for c in self.values():
            c.enable_observer()

    def disable_observer(self):
        for c in self.values():
            c.disable_observer()
