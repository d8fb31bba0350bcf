"""Error measurement: what a cast, a layer or a whole configuration costs -- the mirror of the reference's `utils/benchmark.py:320-530`
(gather_tensors, compute_mse_error, compute_maxdelta_error, compute_error, measure_model_error), plus `format_sweep`.

The numbers come from ONE measuring stick, `ops.error_stats` / `ops.cast_error` (csrc/error_stats.hip): rows of
[sum_sq_err, sum_sq_ref, max_abs_err, count] in float64 that stay on the device.  Where the reference pays one `mse_loss`, one
`abs().max()` and two `.item()` synchronisations per tensor pair, a call here reads the host ONCE, whatever the number of pairs.  Tensors
on the CPU keep the reference's torch expressions.
"""
from collections import OrderedDict
from contextlib import ExitStack
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import ops

__all__ = ["gather_tensors", "compute_mse_error", "compute_maxdelta_error", "compute_error", "measure_model_error", "format_sweep",
           "mse_of", "sqnr_db_of", "ModelErrorReport"]

TensorCollection = Union[torch.Tensor, List[Any], Tuple[Any, ...], Dict[str, Any]]


def mse_of(rows: torch.Tensor) -> torch.Tensor:
    """mean squared error of error_stats rows ([4] or [K, 4]), on the rows' device"""
    return rows[..., 0] / rows[..., 3]


def sqnr_db_of(rows: torch.Tensor) -> torch.Tensor:
    """signal to quantization-noise ratio in dB of error_stats rows, on the rows' device: 10 log10(sum_sq_ref / sum_sq_err)"""
    return 10.0 * torch.log10(rows[..., 1] / rows[..., 0])


def gather_tensors(tensor_collection: TensorCollection) -> List[torch.Tensor]:
    """every tensor of a nested structure of lists, tuples and dicts (a HuggingFace model output, say), in order"""
    if isinstance(tensor_collection, torch.Tensor):
        return [tensor_collection]
    if isinstance(tensor_collection, (tuple, list)):
        return [t for x in tensor_collection for t in gather_tensors(x)]
    if isinstance(tensor_collection, dict):
        return [t for v in tensor_collection.values() for t in gather_tensors(v)]
    return []


_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)   # what dmxq_error_stats reads


def _torch_pair(x: torch.Tensor, y: torch.Tensor, want_mse: bool, want_max: bool) -> torch.Tensor:
    """[mse, maxdelta] of one pair by the reference's torch expressions, as a float64 [2] tensor on the pair's device: any dtype torch
    can subtract (token ids, position ids, float64, ...).  torch has no bool subtraction: masks are compared as 0 / 1."""
    if x.dtype == torch.bool or y.dtype == torch.bool:
        x, y = x.float(), y.float()
    mse = torch.nn.functional.mse_loss(x.float(), y.float()) if want_mse else torch.zeros((), device=x.device)
    mx = (x - y).float().abs().max() if want_max else torch.zeros((), device=x.device)
    return torch.stack([mse.double(), mx.double()])


def _pair_stats(t_list1: Sequence[torch.Tensor], t_list2: Sequence[torch.Tensor], want_mse: bool, want_max: bool):
    """per pair (mse, maxdelta) as Python floats.  Pairs on a GPU: float32 / float16 / bfloat16 through ops.error_stats, every other
    dtype through the reference's expressions on the device, and ONE host read for all of them (per device).  Pairs on the CPU: the
    reference's expressions."""
    pairs = list(zip(t_list1, t_list2))
    res: List[Optional[Tuple[float, float]]] = [None] * len(pairs)
    on_gpu: Dict[torch.device, List[int]] = OrderedDict()
    for i, (x, y) in enumerate(pairs):
        if x.is_cuda and y.is_cuda and x.device == y.device:
            on_gpu.setdefault(x.device, []).append(i)
        else:
            res[i] = tuple(_torch_pair(x, y, want_mse, want_max).tolist())
    for dev, idx in on_gpu.items():
        fused = [i for i in idx if pairs[i][0].dtype in _KERNEL_DTYPES and pairs[i][1].dtype in _KERNEL_DTYPES]
        other = [i for i in idx if i not in fused]
        vals = []
        if fused:
            rows = torch.empty((len(fused), 4), dtype=torch.float64, device=dev)
            for j, i in enumerate(fused):
                ops.error_stats(pairs[i][0], pairs[i][1], out=rows[j])
            vals.append(torch.stack([mse_of(rows), rows[:, 2]], dim=1))
        if other:
            vals.append(torch.stack([_torch_pair(pairs[i][0].detach(), pairs[i][1].detach(), want_mse, want_max) for i in other]))
        host = torch.cat(vals).cpu().tolist()   # the one host read
        for (mse, mx), i in zip(host, fused + other):
            res[i] = (mse, mx)
    return res


def compute_mse_error(t_list1: Sequence[torch.Tensor], t_list2: Sequence[torch.Tensor]) -> float:
    """sum of the mean squared errors of corresponding pairs"""
    return sum(r[0] for r in _pair_stats(t_list1, t_list2, True, False))


def compute_maxdelta_error(t_list1: Sequence[torch.Tensor], t_list2: Sequence[torch.Tensor]) -> float:
    """largest element-wise difference over all pairs (0 without pairs)"""
    return max([r[1] for r in _pair_stats(t_list1, t_list2, False, True)] + [0])


def compute_error(out1: TensorCollection, out2: TensorCollection) -> Dict[str, float]:
    """{"mse": sum over the pairs of their mean squared error, "maxdelta": max over the pairs of their largest difference} between the
    tensors of two collections of the same structure"""
    res = _pair_stats(gather_tensors(out1), gather_tensors(out2), True, True)
    return {"mse": sum(r[0] for r in res), "maxdelta": max([r[1] for r in res] + [0])}


# ---------------------------------------------------------------------------------------------------- per-layer errors of a model
class ModelErrorReport(dict):
    """measure_model_error's result: {name of the tested model: {"cumulative" | "per_layer" | "input": {layer: {"mse", "maxdelta"}},
    "final_output_error": {"mse", "maxdelta"}}}; `.table` (and str()) is the plain-text table the reference prints"""
    table: str = ""

    def __str__(self):
        return self.table


def _dmx_modules(model: torch.nn.Module, names: Optional[Sequence[str]] = None):
    from .nn import DmxModule
    mods = OrderedDict((n, m) for n, m in model.named_modules() if isinstance(m, DmxModule))
    if names is None:
        return mods
    missing = [n for n in names if n not in mods]
    if missing:
        raise AttributeError(f"submodules {missing} not found among the model's DmxModules")
    return OrderedDict((n, mods[n]) for n in dict.fromkeys(names))


def _collect(model, runner, names):
    mods = _dmx_modules(model, names)
    records = {n: [] for n in mods}
    with ExitStack() as stack, torch.no_grad():
        for n, m in mods.items():
            stack.enter_context(m.monitoring(records[n]))
        final = runner(model)
    return mods, records, final


def _plain_table(columns: "OrderedDict[str, list]") -> str:
    try:
        from tabulate import tabulate
        return tabulate(columns, headers="keys", tablefmt="github")
    except ImportError:
        pass
    heads = list(columns)
    n = max(len(v) for v in columns.values())
    cells = [[str(columns[h][r]) if r < len(columns[h]) else "" for h in heads] for r in range(n)]
    width = [max([len(h)] + [len(row[c]) for row in cells]) for c, h in enumerate(heads)]
    line = lambda row: "| " + " | ".join(v.ljust(w) for v, w in zip(row, width)) + " |"   # noqa: E731
    return "\n".join([line(heads), "|" + "|".join("-" * (w + 2) for w in width) + "|"] + [line(r) for r in cells])


def measure_model_error(reference_model: torch.nn.Module, models: Dict[str, torch.nn.Module], runner: Callable[[torch.nn.Module], Any],
                        modules: Optional[Sequence[str]] = None) -> ModelErrorReport:
    """The error at every DmxModule of each model in `models` against the same module of `reference_model` (utils/benchmark.py:413-531).
    runner(model) runs one forward on the SAME data for every model and returns its output; modules: names as in named_modules()
    (default: every DmxModule of the tested model).  Per tested model and layer, summed over the forwards the layer saw:
      "input"       its inputs against the reference's inputs;
      "cumulative"  its output against the reference's output -- its own error and everything upstream;
      "per_layer"   its output when RE-RUN on the reference's recorded inputs against the reference's output -- its own error alone;
    and "final_output_error" between the models' outputs."""
    ref_names = None if modules is None else list(modules)
    _, ref_records, ref_final = _collect(reference_model, runner, ref_names)
    report = ModelErrorReport()
    table_layers: List[str] = []
    for name, model in models.items():
        mods, records, final = _collect(model, runner, ref_names)
        cum, per, inp = OrderedDict(), OrderedDict(), OrderedDict()
        for layer, mod in mods.items():
            if layer not in ref_records:
                continue
            assert len(records[layer]) == len(ref_records[layer]), f"{layer}: the models ran it a different number of times"
            cum[layer], per[layer], inp[layer] = ({"mse": 0.0, "maxdelta": 0.0} for _ in range(3))
            for d_ref, d_test in zip(ref_records[layer], records[layer]):
                with torch.no_grad():
                    clean = mod(*d_ref["input"][0], **d_ref["input"][1])
                for acc, err in ((inp[layer], compute_error(d_ref["input"], d_test["input"])),
                                 (cum[layer], compute_error(d_ref["output"], d_test["output"])),
                                 (per[layer], compute_error(d_ref["output"], clean))):
                    for metric, val in err.items():
                        acc[metric] += val
        report[name] = {"cumulative": cum, "per_layer": per, "input": inp, "final_output_error": compute_error(final, ref_final)}
        if len(cum) > len(table_layers):
            table_layers = list(cum)

    def cell(e):
        return f'{e["mse"]:.2g}({e["maxdelta"]:.2g})'

    columns = OrderedDict({"error relative to the reference": ["error_format", "final_output_error"] + table_layers})
    for name, r in report.items():
        for kind in ("per_layer", "cumulative", "input"):
            columns[f"{name}({kind})"] = ["mse(max delta)", cell(r["final_output_error"])] + [cell(r[kind][l]) if l in r[kind] else "" for l in table_layers]
    report.table = _plain_table(columns)
    return report


# ---------------------------------------------------------------------------------------------------- format sweep
def _labels(formats):
    from .format import Format
    out = []
    for f in formats:
        f = f[0] if isinstance(f, (tuple, list)) else f
        out.append(f if isinstance(f, str) else repr(Format.from_shorthand(f)))
    return out


def _sweep_rows(x, formats, block_dim, hadamard):
    """the error_stats rows [len(hadamard) * K, 4] of x against its cast to each of K formats, per rotation entry (None: no rotation:
    ops.cast_error; a size: the rotated cast ops.hadamard_qdq(x, size, format) -- rotate, cast, rotate back -- then ops.error_stats)"""
    rows = []
    for h in hadamard:
        if h is None:
            rows.append(ops.cast_error(x, formats, block_dim=block_dim))
            continue
        r = torch.empty((len(formats), 4), dtype=torch.float64, device=x.device)
        for k, entry in enumerate(formats):
            fmt, scale, zp = ops.cast_error_entry(entry)
            with torch.no_grad():
                y = ops.hadamard_qdq(x.detach(), h, fmt, block_dim=block_dim, scale=scale, zero_point=zp)
            ops.error_stats(x, y, out=r[k])
        rows.append(r)
    return torch.cat(rows)


def _sweep_labels(formats, hadamard):
    """(rotation entries, result keys) of format_sweep: "<format>" for the entry None, "<format> @H<size>" for a rotation size, entry by
    entry in the order given"""
    entries = list(hadamard) if isinstance(hadamard, (list, tuple)) else [hadamard]
    if not entries:
        raise ValueError("format_sweep: hadamard is a size, or a non-empty list of sizes and None")
    for h in entries:
        if h is not None:
            ops.hadamard_check_size(h, "format_sweep")
    return entries, [l if h is None else f"{l} @H{h}" for h in entries for l in _labels(formats)]


def format_sweep(model_or_tensor, formats, block_dim: Optional[int] = None, hadamard=None):
    """SQNR in dB of every candidate format, from one read of each tensor per 8 formats (ops.cast_error).
    A tensor -> {format: dB}; a model -> {module name: {format: dB}} over the weight of every weighted DmxModule, blocks along the module's
    `weight_cast.block_dim` (or block_dim when given).  formats as in ops.cast_error; the keys are the shorthands given (repr() of Format
    objects).  All rows stay on the device until ONE host read at the end.  An exact cast shows as inf.
    hadamard: a rotation size, or a list of sizes that may include None -- every format is measured once per entry, None as it stands
    and a size wrapped in the orthonormal block-Hadamard rotation of that width along the blocked dimension (ops.hadamard_qdq: rotate,
    cast, rotate back; a FixedPoint entry's scale applies to the ROTATED tensor).  Keys: "<format>" for None, "<format> @H<size>"
    otherwise, in the order of `hadamard`."""
    formats = list(formats)
    entries, labels = _sweep_labels(formats, hadamard)
    if isinstance(model_or_tensor, torch.Tensor):
        db = sqnr_db_of(_sweep_rows(model_or_tensor, formats, -1 if block_dim is None else block_dim, entries)).cpu().tolist()
        return dict(zip(labels, db))
    names, rows = [], []
    for n, m in _dmx_modules(model_or_tensor).items():
        w = getattr(m, "weight", None)
        if w is None or m.weight_cast is None or not w.is_floating_point():
            continue
        names.append(n)
        rows.append(sqnr_db_of(_sweep_rows(w, formats, m.weight_cast.block_dim if block_dim is None else block_dim, entries)))
    if not names:
        return {}
    host: Dict[torch.device, list] = {}
    for dev in dict.fromkeys(r.device for r in rows):
        host[dev] = torch.stack([r for r in rows if r.device == dev]).cpu().tolist()
    return {n: dict(zip(labels, host[r.device].pop(0))) for n, r in zip(names, rows)}
