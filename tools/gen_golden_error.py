"""tests/golden/error_stats.npz: the reference's own compute_error (utils/benchmark.py:392-410: gather_tensors, compute_mse_error,
compute_maxdelta_error) on the seeded cases of tests/_error_ref.py.

Build container only: loads the reference read-only through oracle/ref_shim.py, which stands in for the third-party modules this image
lacks; `tabulate` (imported by utils/benchmark.py for its table, never called here) gets a stand-in the same way when it is absent.
Nothing of the reference's arithmetic is replaced: mse is its sum of torch.nn.functional.mse_loss(x.float(), y.float()).item(),
maxdelta its max of (x - y).float().abs().max().item().

The fixture keeps the case table (kinds, shapes, dtypes, seeds, noise: tests/_data.py `make` rebuilds the tensors anywhere), the
reference's two numbers per case as float64, and the torch version that computed them (the mse is bit-exact only on the same build:
ATen leaves the order of its float32 sum open).
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ref_shim  # noqa: E402
from _error_ref import CASES, build_case, case_table_json, compute_error_ref  # noqa: E402

try:
    import tabulate  # noqa: F401
except ImportError:
    sys.modules["tabulate"] = types.SimpleNamespace(tabulate=lambda *a, **k: "")
ref_shim.load_reference()
from dmx.compressor.utils.benchmark import compute_error  # noqa: E402


def main():
    out = {"case_table": np.array(case_table_json()), "torch_version": np.array(torch.__version__), "names": np.array(list(CASES))}
    for name in CASES:
        a, b = build_case(name)
        e = compute_error(a, b)
        r = compute_error_ref(a, b)
        out[f"{name}_mse"] = np.float64(e["mse"])
        out[f"{name}_maxdelta"] = np.float64(e["maxdelta"])
        rel = abs(r["mse"] - e["mse"]) / e["mse"] if e["mse"] else 0.0
        print(f"{name}: reference mse {e['mse']:.9g} maxdelta {e['maxdelta']:.9g} | float64 restatement mse {r['mse']:.9g} (rel {rel:.2g}) "
              f"maxdelta {r['maxdelta']:.9g} n {r['n']}", flush=True)
        assert r["maxdelta"] == e["maxdelta"], name
    path = os.path.join(ROOT, "tests", "golden", "error_stats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
