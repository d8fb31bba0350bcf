"""Case table for the module-forward parity fixtures of the activation / normalisation DmxModules.

ONE table drives three users, so that all of them build identical inputs, weights and modules:
  * `oracle/gen_golden_r7.py` runs the REFERENCE's modules (dmx.compressor.modeling.nn, CPU) on it and commits the bit patterns of
    their outputs (tests/golden/approx_modules_{f32,bf16,f16}.npz);
  * `tests/test_approx_modules_host.py` regenerates the inputs and reproduces those bits with the oracle's casts around torch's CPU
    functions (no GPU, no reference);
  * `tests/test_gpu_approx_modules.py` / `tools/accuracy_vs_reference.py` run this repo's mirror (dmx_compressor_amd.nn) on it.
Inputs are never stored: every one is a function of (seed, linear index) through tests/_data.make, and the fixture keeps its SHA-256.

No reference import and no GPU import here.  Row LENGTHS are the ones that select the kernel shapes of csrc/approx.hip (64 / 32 lanes
per row, ragged 197 / 1500, the workgroup-per-row 4096) and stay; row COUNTS are as small as the planted rows allow, to keep the
float32 fixture (whose `raw` values do not compress) within the size of the other fixtures."""
import os
from collections import namedtuple

import numpy as np
import torch

from _data import make

F = torch.nn.functional
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CONFIGS = ("basic", "same")
FLOAT16 = "FP[1|5|10,15](FN)"            # config_rules.BASIC's format on both sides of every module of this table
_T_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_NP_BITS = {torch.float32: np.uint32, torch.bfloat16: np.uint16, torch.float16: np.uint16}

SPECIALS = [0.0, -0.0, 65504.0, 65520.0, -65536.0, 131008.0, 1e30, -3e38, 6.1e-5, 6.0e-5, -6.2e-5, 1e-30, -1e-40, 88.5, -88.5, 11.0, -11.0,
            float("inf"), float("-inf"), float("nan")]


def inputs_with_specials(shape, dtype, seed, scale=3.0, specials=True):
    """scale * normal, with the saturating, flushed, signed-zero and non-finite values and the FLOAT16 thresholds planted at
    elements 1, 4, 7, ... (the `_inputs` of tests/test_gpu_act_cast.py)"""
    x = make("normal", shape, seed=seed) * scale
    if specials:
        flat = x.reshape(-1)
        k = min(len(SPECIALS), flat.numel() // 4)
        flat[torch.arange(k) * 3 + 1] = torch.tensor(SPECIALS[:k])
    return x.to(dtype)


# family: the key of d_ref and of the tolerance; cls: the class name on both sides; args / kwargs: the constructor's
Case = namedtuple("Case", "name family cls args kwargs shape seed")

CASES = [
    Case("softmax_7x64", "softmax", "Softmax", (), {"dim": -1}, (7, 64), 1101),
    Case("softmax_5x197", "softmax", "Softmax", (), {"dim": -1}, (5, 197), 1102),
    Case("softmax_3x1500", "softmax", "Softmax", (), {"dim": -1}, (3, 1500), 1103),
    Case("softmax_2x4096", "softmax", "Softmax", (), {"dim": -1}, (2, 4096), 1104),
    Case("softmax_dim-2_48x40", "softmax", "Softmax", (), {"dim": -2}, (2, 48, 40), 1105),
    Case("layernorm_768", "layernorm", "LayerNorm", (768,), {}, (3, 768), 1201),
    Case("layernorm_4096", "layernorm", "LayerNorm", (4096,), {}, (2, 4096), 1202),
    Case("layernorm_1500", "layernorm", "LayerNorm", (1500,), {}, (2, 1500), 1203),
    Case("layernorm_768_noaffine", "layernorm", "LayerNorm", (768,), {"elementwise_affine": False}, (3, 768), 1204),
    Case("rmsnorm_4096_default_eps", "rmsnorm", "RMSNorm", (4096,), {}, (2, 4096), 1301),
    Case("rmsnorm_768_default_eps", "rmsnorm", "RMSNorm", (768,), {}, (3, 768), 1302),
    Case("rmsnorm_4096_eps1e-6", "rmsnorm", "RMSNorm", (4096,), {"eps": 1e-6}, (2, 4096), 1303),
    Case("rmsnorm_768_eps1e-6", "rmsnorm", "RMSNorm", (768,), {"eps": 1e-6}, (3, 768), 1304),
    Case("gelu", "gelu", "GELU", (), {}, (1, 1024), 1401),
    Case("gelu_approximate_tanh", "gelu_tanh", "GELU", (), {"approximate": "tanh"}, (1, 1024), 1401),   # same input as "gelu"
    Case("silu", "silu", "SiLU", (), {}, (1, 1024), 1403),
    Case("quick_gelu", "quick_gelu", "QuickGELU", (), {}, (1, 1024), 1404),
    Case("exp", "exp", "Exp", (), {}, (1, 1024), 1405),
    Case("new_gelu", "new_gelu", "NewGELU", (), {}, (1, 1024), 1406),
    Case("fast_gelu", "fast_gelu", "FastGELU", (), {}, (1, 1024), 1407),
]
BY_NAME = {c.name: c for c in CASES}
NORMS = ("layernorm", "rmsnorm")


def case_input(case, dtype):
    """the module's input for `case` in `dtype` (CPU)"""
    if case.family == "softmax":
        x = inputs_with_specials(case.shape, dtype, case.seed, scale=2.0, specials=False)
        rows = x.movedim(case.kwargs["dim"], -1)        # a view: rows along the softmax dim
        if rows.numel() // rows.shape[-1] >= 3:         # the attention-mask row: first half -inf (FLOAT16 makes it -131008)
            rows[(0,) * (rows.dim() - 1) + (slice(0, rows.shape[-1] // 2),)] = float("-inf")
        return x
    if case.family in NORMS:
        x = (inputs_with_specials(case.shape, dtype, case.seed, scale=2.0, specials=False).float() + 0.5).to(dtype)
        x[1, 5] = 70000.0 if dtype != torch.float16 else 65504.0        # saturates in FLOAT16
        return x
    return inputs_with_specials(case.shape, dtype, case.seed, scale=3.0)


def case_params(case, dtype):
    """(weight, bias) in `dtype`, None where the module has none"""
    if case.family not in NORMS or case.kwargs.get("elementwise_affine") is False:
        return None, None
    cols = case.args[0]
    w = (make("normal", (cols,), seed=case.seed + 50) * 0.1 + 1).to(dtype)
    b = (make("normal", (cols,), seed=case.seed + 51) * 0.1).to(dtype) if case.family == "layernorm" else None
    return w, b


def build_module(nn, case, dtype, device="cpu"):
    """the module of `case` from the namespace `nn` (the reference's or this repo's), unconfigured, with the seeded parameters"""
    m = getattr(nn, case.cls)(*case.args, **case.kwargs)
    if case.family in NORMS:
        m = m.to(dtype)
    w, b = case_params(case, dtype)
    with torch.no_grad():
        if w is not None:
            m.weight.copy_(w)
        if b is not None:
            m.bias.copy_(b)
    return m.to(device).eval()


def cpu_cast(oracle, config):
    """the module's input / output CastTo on the CPU through the oracle (dtype -> same dtype): FLOAT16 for "basic", a copy for "same" """
    if config == "same":
        return lambda x: x.clone()
    return lambda x: oracle.floating_point_cast(x, 10, 5, 15, True).to(x.dtype)


def _quick_gelu(x):      # transformers.activations.QuickGELUActivation
    return x * torch.sigmoid(1.702 * x)


def _new_gelu(x):        # transformers.activations.NewGELUActivation
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * torch.pow(x, 3.0))))


def _fast_gelu(x):       # transformers.activations.FastGELUActivation
    return 0.5 * x * (1.0 + torch.tanh(x * 0.7978845608 * (1.0 + 0.044715 * x * x)))


def torch_forward(case, c, w, b, eps):
    """the plain torch function the REFERENCE's module evaluates between its casts, on the cast input `c` -- in the dtype of `c`
    (the host test), or in float64 (the truth of d_ref).  Pinned bit for bit to the stored reference outputs by the generator and the
    host test.  `GELU(approximate="tanh")` is F.gelu(x) there: the constructor argument does not reach the function."""
    fam = case.family
    if fam == "softmax":
        return F.softmax(c, dim=case.kwargs["dim"])
    if fam == "layernorm":
        return F.layer_norm(c, tuple(case.args), w, b, eps)
    if fam == "rmsnorm":
        return F.rms_norm(c, tuple(case.args), w, eps)
    return {"gelu": F.gelu, "gelu_tanh": F.gelu, "silu": F.silu, "quick_gelu": _quick_gelu, "exp": torch.exp, "new_gelu": _new_gelu,
            "fast_gelu": _fast_gelu}[fam](c)


def to_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_T_BITS[t.dtype]).numpy().view(_NP_BITS[t.dtype]).copy()


def from_bits(a, dtype):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if dtype == torch.float32 else np.int16).copy()).view(dtype)


def fixture_path(dt_name):
    return os.path.join(GOLD, f"approx_modules_{dt_name}.npz")


class Fixture:
    """tests/golden/approx_modules_<dtype>.npz.  Keys: `<case>/sha256` (of the input bits), `<case>/<config>/{raw,y}` (bit patterns;
    `raw` is the module's `_forward(input_cast(x))`, `y` its full forward; under "same" the two are the same bits and `raw` is stored
    once, as `y`), `<case>/<config>/{eps,dim}` (NaN where the module has none), `d_ref/<family>/<config>`, `cpu_capability`."""

    def __init__(self, dt_name):
        self.dtype = DTYPES[dt_name]
        self.z = np.load(fixture_path(dt_name))
        self.cpu_capability = str(self.z["cpu_capability"])

    def has(self, case):
        return f"{case.name}/sha256" in self.z.files

    def sha256(self, case):
        return str(self.z[f"{case.name}/sha256"])

    def y(self, case, config):
        return from_bits(self.z[f"{case.name}/{config}/y"], self.dtype).reshape(case.shape)

    def raw(self, case, config):
        k = f"{case.name}/{config}/raw"
        return from_bits(self.z[k], self.dtype).reshape(case.shape) if k in self.z.files else self.y(case, config)

    def defect(self, case, config):
        """mask of the elements where the reference's CPU evaluation and the float64 truth disagree on being NaN / Inf (recorded by
        the generator, which admits exactly one kind: torch's vectorised CPU erf-GELU of +Inf is NaN)"""
        m = torch.zeros(case.shape, dtype=torch.bool)
        k = f"{case.name}/{config}/defect_idx"
        if k in self.z.files:
            m.view(-1)[torch.from_numpy(self.z[k].astype(np.int64))] = True
        return m

    def centre(self, case, config):
        """float64 `raw`, with the float64 truth's value at the `defect` elements: what this repo's modules are pinned to"""
        c = self.raw(case, config).double()
        k = f"{case.name}/{config}/defect_idx"
        if k in self.z.files:
            c.view(-1)[torch.from_numpy(self.z[k].astype(np.int64))] = torch.from_numpy(self.z[f"{case.name}/{config}/defect_truth"])
        return c

    def eps(self, case, config):
        v = float(self.z[f"{case.name}/{config}/eps"])
        return None if v != v else v

    def dim(self, case, config):
        v = float(self.z[f"{case.name}/{config}/dim"])
        return None if v != v else int(v)

    def d_ref(self, family, config):
        return float(self.z[f"d_ref/{family}/{config}"])


def distance_to(got, want, dtype, floor=None):
    """how far `got` is from the stored reference output `want` (both of `dtype`): (elements whose bits differ -- any NaN matches any
    NaN --, largest distance over the finite pairs in ulps of `dtype` at |want| or, where larger, at the contract's absolute `floor`
    (the magnitude of the terms that cancel in GELU and LayerNorm: tests/_data.err_in_ulps), how many of the differing elements lie
    above / below `want`; the rest of them differ in the sign of a zero or in being finite).  Reported, never asserted."""
    from _data import ulp_of
    g, t = got.detach().cpu(), want.detach().cpu()
    both_nan = torch.isnan(g) & torch.isnan(t)
    diff = (g.contiguous().view(_T_BITS[dtype]) != t.contiguous().view(_T_BITS[dtype])) & ~both_nan
    gd, td = g.double(), t.double()
    fin = torch.isfinite(gd) & torch.isfinite(td) & diff
    u = ulp_of(td, dtype, floor)
    worst = float(((gd - td).abs()[fin] / u[fin]).max()) if bool(fin.any()) else 0.0
    return int(diff.sum()), worst, int((diff & (gd > td)).sum()), int((diff & (gd < td)).sum())
