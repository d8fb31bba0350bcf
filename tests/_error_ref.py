"""The float64 restatement of the error statistics (include/dmxq.h "error statistics") and the seeded cases of
tests/golden/error_stats.npz.  Shared by tools/gen_golden_error.py (which runs the REFERENCE's compute_error on these cases), the host
test and the GPU test; imports neither the library nor the reference.

One row per tensor pair (r, t): [sum_sq_err, sum_sq_ref, max_abs_err, count] with d = float(r) - float(t), one fp32 subtraction;
sum_sq_err = sum d^2 and sum_sq_ref = sum float(r)^2 with every square formed in float64 (exact) and summed in float64;
max_abs_err = torch's own (r - t).float().abs().max(): the difference rounded to the promoted dtype of the pair."""
import json
from collections import OrderedDict

import torch

from _data import make

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def error_row_ref(r: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """float64 [4] on the CPU"""
    r, t = r.detach().cpu().reshape(-1), t.detach().cpu().reshape(-1)
    n = r.numel()
    if n == 0:
        return torch.zeros(4, dtype=torch.float64)
    d = r.float() - t.float()
    sse = (d.double() * d.double()).sum()
    ssr = (r.double() * r.double()).sum()
    mx = (r - t).float().abs().max().double()
    return torch.stack([sse, ssr, mx, torch.tensor(float(n), dtype=torch.float64)])


def sum_bound(n: int) -> float:
    """relative bound between an fp64 sum of n non-negative terms in ANY order and the float64 restatement: each is within
    (n - 1) 2^-53 of the exact sum"""
    return n * 2.0 ** -52


def gather(c):
    if isinstance(c, torch.Tensor):
        return [c]
    if isinstance(c, (tuple, list)):
        return [t for x in c for t in gather(x)]
    if isinstance(c, dict):
        return [t for v in c.values() for t in gather(v)]
    return []


def compute_error_ref(out1, out2):
    """compute_error (utils/benchmark.py:392-410) from the rows: sum of the pairs' mse, max of the pairs' maxdelta"""
    rows = [error_row_ref(x, y) for x, y in zip(gather(out1), gather(out2))]
    return {"mse": sum(float(r[0] / r[3]) for r in rows), "maxdelta": max([float(r[2]) for r in rows] + [0]), "n": [int(r[3]) for r in rows]}


# ---------------------------------------------------------------------------------------------------- the fixture's cases
# a leaf: ("T", kind of tests/_data.py make, shape, dtype of the reference side, dtype of the test side, seed, noise): the reference side
# is make(kind, shape, seed) in its dtype, the test side is the float32 values plus noise * make("normal", shape, seed + 500) in its
# dtype.  Everything else is structure; None and numbers are the non-tensor entries a model output carries.
def T(kind, shape, dr, dt, seed, noise):
    return ["T", kind, list(shape), dr, dt, seed, noise]


CASES = OrderedDict([
    ("f32_pair", T("normal", (64, 96), "f32", "f32", 11, 0.01)),
    ("bf16_pair", T("normal", (32, 128), "bf16", "bf16", 12, 0.02)),
    ("f16_pair", T("normal", (48, 40), "f16", "f16", 13, 0.005)),
    ("mixed_f32_bf16", T("normal", (40, 64), "f32", "bf16", 14, 0.0)),
    ("mixed_f16_bf16", T("normal", (24, 72), "f16", "bf16", 15, 0.01)),
    ("heavy_f32", T("heavy", (128, 33), "f32", "f32", 16, 0.5)),
    ("one_element", T("normal", (1,), "bf16", "bf16", 17, 0.25)),
    ("list_of_three", [T("normal", (16, 64), "f32", "f32", 18, 0.01), T("normal", (8, 24), "bf16", "bf16", 19, 0.03),
                       T("outlier", (4, 160), "f16", "f16", 20, 0.01)]),
    ("nested", {"logits": T("normal", (2, 7, 50), "f32", "f32", 21, 0.02),
                "hidden": (T("normal", (2, 7, 32), "bf16", "bf16", 22, 0.02), T("normal", (2, 7, 32), "bf16", "bf16", 23, 0.04)),
                "past": [{"k": T("normal", (2, 2, 7, 16), "f16", "f16", 24, 0.01), "v": T("normal", (2, 2, 7, 16), "f16", "f16", 25, 0.01)}],
                "loss": None, "steps": 3}),
    ("tuple_with_others", (T("ties", (32, 32), "f32", "f32", 26, 0.0039062), None, 5, [T("normal", (9,), "f32", "f16", 27, 0.0)])),
    ("empty_list", []),
])


def case_table_json() -> str:
    return json.dumps(CASES, sort_keys=False)


def _build(node, side):
    if isinstance(node, list) and node and node[0] == "T":
        _, kind, shape, dr, dt, seed, noise = node
        ref = make(kind, tuple(shape), seed=seed)
        if side == 0:
            return ref.to(DTYPES[dr])
        return (ref + noise * make("normal", tuple(shape), seed=seed + 500)).to(DTYPES[dt])
    if isinstance(node, dict):
        return {k: _build(v, side) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return type(node)(_build(v, side) for v in node)
    return node


def build_case(name):
    """(reference collection, test collection) of CPU tensors"""
    return _build(CASES[name], 0), _build(CASES[name], 1)
