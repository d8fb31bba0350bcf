#!/usr/bin/env python3
"""oracle/gen_golden_r7.py — BUILD-CONTAINER ONLY (the earlier generators are unchanged so that their fixtures stay byte-identical).

Runs the REFERENCE's activation / normalisation DmxModules (dmx.compressor.modeling.nn through oracle/ref_shim.py, CPU) on the case
table of tests/_approx_cases.py and writes

  tests/golden/approx_modules_{f32,bf16,f16}.npz

Per case and configuration ("basic": the reference's own config_rules.BASIC, FLOAT16 on both sides; "same": the unconfigured module):
the bit patterns of `raw` = the module's `_forward(input_cast(x))` and of `y` = its full forward, the SHA-256 of the input bits, the
module's effective eps / dim; per family and configuration `d_ref`, the largest distance of `raw` from the float64 truth of the
function the reference ACTUALLY evaluates on input_cast(x), in ulps of the tensor dtype with the absolute floors of the existing
contract (tests/test_gpu_act_cast.py UNARY / _ln_truth), measured by tests/_data.err_in_ulps -- on the reference alone; and this
machine's torch CPU capability.  Recorded results, numbers and names only.

Asserted along the way: the oracle's casts around the plain torch CPU function reproduce `raw` and `y` bit for bit (this pins the
generator and tests/_approx_cases.torch_forward), and `GELU(approximate="tanh")` gives the bits of `GELU()`: the reference's
constructor argument never reaches its function.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_r7.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O  # noqa: E402
import ref_shim  # noqa: E402
from _approx_cases import CASES, CONFIGS, DTYPES, FLOAT16, NORMS, build_module, case_input, case_params, cpu_cast, fixture_path, to_bits, torch_forward  # noqa: E402
from _data import err_in_ulps, round_once, sha256_bits  # noqa: E402
from test_gpu_act_cast import UNARY, _ln_truth, _rms_truth  # noqa: E402  (the truths and floors of the existing contract, not restated)

ref = ref_shim.load_reference()
from dmx.compressor.modeling import nn as rnn  # noqa: E402

GELU_FAMILY = ("gelu", "gelu_tanh", "quick_gelu", "new_gelu", "fast_gelu")


def configure(m, config):
    """ "basic": the reference's own rule for the module's type; the GELU family gets the same two FLOAT16 formats explicitly"""
    if config == "same":
        return m
    hit = False
    for r in ref.config_rules.BASIC:
        if isinstance(m, r.module_types):
            m.configure(r.module_config)
            hit = True
    if not hit or isinstance(m, rnn.GELUBase):
        m.configure(dict(input_formats=[FLOAT16], output_formats=[FLOAT16]))
    fi, fo = m.input_casts.input_cast.format, m.output_casts.output_cast.format
    assert repr(fi) == FLOAT16 and repr(fo) == FLOAT16, (type(m).__name__, repr(fi), repr(fo))
    return m


def truth_and_floor(case, cin, w, b, eps):
    """float64 truth of the function the reference evaluates, and the absolute floor the contract counts ulps against"""
    fam = case.family
    if fam == "softmax":
        return torch.nn.functional.softmax(cin.double(), case.kwargs["dim"]), None
    if fam == "layernorm":
        return _ln_truth(cin, case.args[0], w, b, eps)
    if fam == "rmsnorm":
        return _rms_truth(cin, case.args[0], w, eps), None
    if fam in ("new_gelu", "fast_gelu"):
        return torch_forward(case, cin.double(), None, None, None), cin.double().abs() / 2
    f64, floor_fn, _ = UNARY["gelu" if fam == "gelu_tanh" else fam]      # approximate="tanh" IS erf in the reference
    return f64(cin, cin.dtype), None if floor_fn is None else floor_fn(cin)


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    both_nan = (torch.isnan(a.float()) & torch.isnan(b.float())).numpy()
    return bool(((to_bits(a) == to_bits(b)) | both_nan).all())


def save_npz(path, store):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(store[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    checked = 0
    for dt_name, dtype in DTYPES.items():
        store = {"cpu_capability": np.array(torch.backends.cpu.get_cpu_capability())}
        d_ref = {}
        ys = {}
        for case in CASES:
            if not hasattr(rnn, case.cls):
                print(f"[{dt_name}] {case.name}: the reference has no {case.cls}; left out")
                continue
            x = case_input(case, dtype)
            w, b = case_params(case, dtype)
            store[f"{case.name}/sha256"] = np.array(sha256_bits(x))
            for config in CONFIGS:
                m = configure(build_module(rnn, case, dtype), config)
                with torch.no_grad():
                    cin, _, _ = m.input_casts(x.clone())
                    raw = m._forward(cin)
                    y = m(x.clone())
                assert raw.dtype == dtype and y.dtype == dtype and tuple(y.shape) == case.shape, (case.name, raw.dtype, y.dtype, y.shape)
                eps, dim = getattr(m, "eps", None), getattr(m, "dim", None)
                # the generator's own restatement: oracle casts around the plain torch function
                cast = cpu_cast(O, config)
                c0 = cast(x)
                assert same_bits(c0, cin), f"ORACLE != REFERENCE: input cast of {case.name} {dt_name} {config}"
                r0 = torch_forward(case, c0, w, b, eps)
                assert same_bits(r0, raw), f"torch function != REFERENCE `_forward`: {case.name} {dt_name} {config}"
                assert same_bits(cast(r0), y), f"ORACLE casts around torch != REFERENCE forward: {case.name} {dt_name} {config}"
                checked += 3
                key = f"{case.name}/{config}"
                store[f"{key}/y"] = to_bits(y)
                if config == "same":
                    assert same_bits(raw, y), f"{key}: an unconfigured module's forward is its `_forward`"
                else:
                    store[f"{key}/raw"] = to_bits(raw)
                store[f"{key}/eps"] = np.array(float("nan") if eps is None else float(eps))
                store[f"{key}/dim"] = np.array(float("nan") if dim is None else float(dim))
                ys[key] = y
                truth, floor = truth_and_floor(case, cin, w, b, eps)
                # elements where the reference's CPU evaluation and the float64 truth disagree on being NaN / Inf are no rounding
                # distance: each is a finding of its own.  The one known: torch's vectorised CPU erf-GELU of +Inf is
                # NaN (float64, and torch on a GPU: +Inf).  They are recorded with the truth's value and left out of d_ref; anything
                # else stops the generator.
                rd, td = raw.double(), round_once(truth.double(), dtype).double()      # (the comparison err_in_ulps makes)
                defect = (torch.isnan(rd) ^ torch.isnan(td)) | ((torch.isinf(td) | torch.isinf(rd)) & ~torch.isnan(rd) & ~torch.isnan(td) & (rd != td))
                if bool(defect.any()):
                    assert case.family in ("gelu", "gelu_tanh") and bool((cin.double()[defect] == float("inf")).all()) \
                        and bool(torch.isnan(rd[defect]).all()) and bool((td[defect] == float("inf")).all()), \
                        f"{key}: the reference and the float64 truth disagree on NaN / Inf at {int(defect.sum())} elements"
                    store[f"{key}/defect_idx"] = defect.reshape(-1).nonzero().reshape(-1).numpy().astype(np.int32)
                    store[f"{key}/defect_truth"] = td[defect].numpy().astype(np.float64)
                    print(f"[{dt_name}] {key}: NaN where the float64 truth is +Inf at {int(defect.sum())} elements (input +Inf)")
                d = err_in_ulps(torch.where(defect, td.to(dtype), raw), truth, dtype, floor)
                d_ref[(case.family, config)] = max(d_ref.get((case.family, config), 0.0), d)
        for config in CONFIGS:   # the finding, as a recorded fact
            assert same_bits(ys[f"gelu_approximate_tanh/{config}"], ys[f"gelu/{config}"]), "GELU(approximate='tanh') != GELU() in the reference"
            checked += 1
        for (fam, config), d in sorted(d_ref.items()):
            assert d == d and d != float("inf"), (fam, config, d)
            store[f"d_ref/{fam}/{config}"] = np.array(d)
            print(f"[{dt_name}] d_ref {fam:11s} {config:5s} {d:.3f} ulp")
        save_npz(fixture_path(dt_name), store)
        print(f"[{dt_name}] {fixture_path(dt_name)}: {os.path.getsize(fixture_path(dt_name))} bytes")
    print(f"oracle / torch == reference on {checked} comparisons")


if __name__ == "__main__":
    main()
