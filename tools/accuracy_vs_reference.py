"""How far this repo's activation / normalisation modules land from the REFERENCE's own forward outputs, measured on the GPU against
tests/golden/approx_modules_{f32,bf16,f16}.npz (oracle/gen_golden_r7.py) -- fixtures only, no reference needed.  Per module family,
dtype and configuration: element count, elements whose bits differ from the reference's `y`, the largest distance in ulps of the
tensor dtype, the sign balance of the differing elements (this library above / below the reference), `d_ref` (how far the reference's
own value sits from the float64 truth) and `N` (what tests/test_gpu_act_cast.py grants the kernel): the bracket
tests/test_gpu_approx_modules.py asserts is N + d_ref.  `GELU(approximate="tanh")` is listed against the reference too -- there the
distance is the documented divergence (the reference evaluates erf for it), not an error.

Second table: the SmoothQuant scale vector of every Linear of the Whisper-small encoder layer (tests/_model_shapes.py), which
tests/test_gpu_model_shapes.py compares within 4 fp32 ulp of the reference's vector (tests/golden/model_scales.npz): how many entries
differ at all, and by how much.

Writes profiles/r14_accuracy_vs_reference.txt, first line tools/stamp.py --header (`--no-write`: print only)."""
import os
import subprocess
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import dmx_compressor_amd as d  # noqa: E402
import oracle as O  # noqa: E402
from _approx_cases import CASES, CONFIGS, DTYPES, Fixture, distance_to  # noqa: E402
from _data import ulp_of  # noqa: E402
from _model_shapes import STAGES, make_api  # noqa: E402
from test_gpu_approx_modules import run_case  # noqa: E402


def module_table(dev):
    lines = [f"{'family':11s} {'dtype':5s} {'config':6s} {'elements':>9s} {'differ':>7s} {'max ulp':>10s} {'above':>6s} {'below':>6s} {'d_ref':>7s} {'N':>4s}"]
    for dt_name in DTYPES:
        fx = Fixture(dt_name)
        rows = OrderedDict()
        for case in CASES:
            for config in CONFIGS:
                r = run_case(d, O, dev, fx, case, config)
                differ, worst, above, below = distance_to(r["got"], r["y"], fx.dtype, r["floor"])
                acc = rows.setdefault((case.family, config), [0, 0, 0.0, 0, 0, r["d_ref"], r["n"]])
                acc[0] += r["got"].numel()
                acc[1] += differ
                acc[2] = max(acc[2], worst)
                acc[3] += above
                acc[4] += below
        for (fam, config), (n, differ, worst, above, below, d_ref, N) in rows.items():
            lines.append(f"{fam:11s} {dt_name:5s} {config:6s} {n:9d} {differ:7d} {worst:10.2f} {above:6d} {below:6d} {d_ref:7.3f} {N:4d}")
    return lines


def smoothquant_table(dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "model_scales.npz"))
    ref = {k: torch.from_numpy(np.ascontiguousarray(z[k]).view(np.int32).copy()).view(torch.float32) for k in z.files}
    stages = STAGES["config5_whisper_small_encoder_layer"](make_api(d.nn, d), None, dev, scales_in=ref)
    lines = [f"{'linear':9s} {'entries':>8s} {'differ':>7s} {'max ulp':>8s}"]
    for name, t in stages:
        if name.endswith("~"):
            lin = name.split("/")[0]
            want = ref[f"whisper/{lin}"]
            differ = int((t.view(torch.int32) != want.view(torch.int32)).sum())
            worst = float(((t.double() - want.double()).abs() / ulp_of(want.double(), torch.float32)).max())
            lines.append(f"{lin:9s} {t.numel():8d} {differ:7d} {worst:8.2f}")
    return lines


def main():
    dev = torch.device("cuda:0")
    header = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip()
    lines = [header,
             f"# tools/accuracy_vs_reference.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
             f"{time.strftime('%Y-%m-%d')}; reference outputs recorded on a CPU with torch capability {Fixture('f32').cpu_capability}",
             "# module forward vs the reference's forward (bits of `y`); ulps of the tensor dtype (at the contract's floor where the result cancels: GELU, LayerNorm); above / below: this library's value "
             "above / below the reference's; the asserted bracket is N + d_ref"]
    lines += module_table(dev)
    lines += ["", "# SmoothQuant scale vectors, Whisper-small encoder layer (asserted: within 4 fp32 ulp)"]
    lines += smoothquant_table(dev)
    print("\n".join(lines), flush=True)
    if "--no-write" not in sys.argv:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r14_accuracy_vs_reference.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
