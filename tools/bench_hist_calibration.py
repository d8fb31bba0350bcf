"""One HistogramObserver calibration step of a CastTo (observe every group + range search + qparams, cast.py _observer_step) on the
GPU: the device path (csrc/hist_observer.hip) against the host code (DMXQ_HIST_HOST=1: per-slab observers, .cpu() reads, the Python
search), in the same process, alternating, device events around a step that ends in a synchronise, medians of 5 steps each after
one warm-up step.  Writes profiles/r08_hist_calibration.txt (first line: tools/stamp.py --header).
Kernel times and launches per step: `rocprofv3 --kernel-trace --stats -- python tools/bench_hist_calibration.py --quick` (device path
only, 10 steps per row, nothing written)."""
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dmx_compressor_amd as d  # noqa: E402

ROWS = [((4096, 4096), torch.bfloat16, None), ((2048, 768), torch.float32, 128), ((2048, 4096), torch.bfloat16, 128)]
FMTS = ["XP[8,0](CSN)", "XP[4,0](CSN)"]


def _cast(fmt, gs, host):
    os.environ["DMXQ_HIST_HOST"] = "1" if host else "0"
    c = d.CastTo(format=fmt).cuda()
    c.enable_calibration(True, d.HistogramObserver, torch.per_tensor_affine, **(dict(group_size=gs, ch_axis=-1) if gs else {}))
    return c


def _step(c, x, host):
    os.environ["DMXQ_HIST_HOST"] = "1" if host else "0"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    c(x)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), 1000 * (time.perf_counter() - t0)


def _batch(shape, dtype, k, gen):
    # the same distribution each step, a slightly wider spread every time: most steps re-bin onto a wider range
    return (torch.randn(shape, generator=gen, device="cuda") * (1.0 + 0.05 * k)).to(dtype)


def main():
    quick = "--quick" in sys.argv
    reps = 10 if quick else 5
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = []
    if not quick:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
        lines.append(f"# tools/bench_hist_calibration.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                     f"{time.strftime('%Y-%m-%d')}; one CastTo calibration step (observe + search + qparams), medians of {reps} steps per "
                     f"path after one warm-up step, device and host (DMXQ_HIST_HOST=1) alternating; device events, wall clock in brackets")
    for shape, dtype, gs in ROWS:
        for fmt in FMTS:
            dev_c = _cast(fmt, gs, False)
            host_c = None if quick else _cast(fmt, gs, True)
            _step(dev_c, _batch(shape, dtype, 0, gen), False)
            if host_c is not None:
                _step(host_c, _batch(shape, dtype, 0, gen), True)
            td, th = [], []
            for k in range(1, reps + 1):
                x = _batch(shape, dtype, k, gen)
                td.append(_step(dev_c, x, False))
                if host_c is not None:
                    th.append(_step(host_c, x, True))
            med = lambda v, i: sorted(t[i] for t in v)[len(v) // 2]
            G = -(-shape[-1] // gs) if gs else 1
            line = (f"{list(shape)} {str(dtype).replace('torch.', '')} {'group ' + str(gs) if gs else 'per tensor'} ({G} groups) {fmt}: "
                    f"device {med(td, 0):.3f} ms [{med(td, 1):.3f}]")
            if th:
                line += f", host {med(th, 0):.3f} ms [{med(th, 1):.3f}], speed-up {med(th, 0) / med(td, 0):.1f}x"
            print(line, flush=True)
            lines.append(line)
    os.environ.pop("DMXQ_HIST_HOST", None)
    if not quick:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r08_hist_calibration.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
