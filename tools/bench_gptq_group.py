"""GPTQ apply() with dynamic per-group scales on the GPU: a 4096 x 4096 Linear, XP[4,0](CSN), weight_dynamic per_group 128, microblock
1, block 128 -- the fused kernel (csrc/gptq_dynamic.hip), the torch loop of the same definition (`fuse_gptq = False`) and, as the
yardstick, the existing fused path with a static per-row scale (csrc/gptq.hip, DMXQ_GPTQ_FIXED).  Same process, alternating, device
events around each apply() after a warm-up; medians.  Every apply() carries the same factorisation (cholesky -> cholesky_inverse ->
upper cholesky), weight copy, diagonal inverses and trailing GEMMs, which pull the ratio of the two fused paths towards 1, so the
in-block launches alone -- what the two kernels differ in -- are timed apart on the same factor.  Writes profiles/r13_gptq_group.txt,
first line tools/stamp.py --header (`--quick`: a 1024 x 1024 layer, one run each, nothing written)."""
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dmx_compressor_amd as d  # noqa: E402
from dmx_compressor_amd.layer_reconstruction import OptimalBrainCompressor  # noqa: E402

FMT, GROUP, MB, BLOCK = "XP[4,0](CSN)", 128, 1, 128


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    quick = "--quick" in sys.argv
    n, reps, loop_reps = (1024, 1, 1) if quick else (4096, 5, 2)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    W0 = torch.randn(n, n, device=dev) * 0.02
    X = torch.randn(2048, n, device=dev)

    def module(dynamic):
        m = d.nn.Linear(n, n, bias=False).to(dev)
        m.configure({"weight_format": FMT, "weight_dynamic": dynamic})
        if dynamic is None:   # static per-output-channel scales, as a MinMax calibration of the weight leaves them
            hp = d.DmxModuleQuantizerCalibrationHyperparams(weight=d.DmxQuantizerCalibrationHyperparams(
                observer_cls=d.MinMaxObserver, qscheme_to_overload=torch.per_channel_symmetric, ch_axis=0))
            with torch.no_grad():
                m.weight.copy_(W0)
                with m.calibrating_quantizers(hp):
                    m(X[:8])
        return m

    dyn, static = module({"per_group": GROUP}), module(None)
    dyn.weight_cast.qscheme = torch.per_tensor_symmetric   # (symmetric scales on both sides, as the static calibration's)
    obc = OptimalBrainCompressor(dyn)
    obc.measure_hessian(X.unsqueeze(0))
    H0 = obc.H.clone()

    def apply(m, fuse):
        def f():
            m.fuse_gptq = fuse
            with torch.no_grad():
                m.weight.copy_(W0)
            m.weight_cast.enable_fake_quant()   # (apply() switches a dynamic cast off)
            o = OptimalBrainCompressor(m)
            o.H = H0.clone()
            o.apply(microblock_size=MB, block_size=BLOCK)
        return f

    runs = {"fused dynamic per_group 128": (apply(dyn, True), reps), "torch loop dynamic per_group 128": (apply(dyn, False), loop_reps),
            "fused static per-row": (apply(static, True), reps)}
    for f, _ in runs.values():   # warm-up
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for i in range(max(reps, loop_reps)):   # alternating
        for k, (f, r) in runs.items():
            if i < r:
                times[k].append(_timed(f))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    # the column loop alone: one launch per 128-column block on the same Hinv, no trailing GEMMs (timing only: the blocks' inputs are W0's)
    H = H0.clone()
    H[range(n), range(n)] += 0.01 * torch.mean(torch.diag(H))
    Hinv = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True).contiguous()
    invd = OptimalBrainCompressor._inv_diag(Hinv, MB)
    W, Q, E = W0.float().clone(), torch.empty(n, n, device=dev), torch.empty(n, BLOCK, device=dev)
    fmt = d.Format.from_shorthand(FMT)
    S = torch.empty(n, n // GROUP, device=dev)
    Z = torch.empty(n, n // GROUP, dtype=torch.int64, device=dev)
    sc, zp = static.weight_cast.scale.detach().float().contiguous(), static.weight_cast.zero_point.detach().to(torch.int64).contiguous()
    fields = d.ops.gptq_fields(fmt, True)

    def blocks(dynamic):
        def f():
            for i1 in range(0, n, BLOCK):
                i2 = i1 + BLOCK
                if dynamic:
                    d.ops.gptq_block_dynamic(W[:, i1:i2], Hinv[i1:i2, i1:i2], invd[i1:i2], Q[:, i1:i2], E, S[:, i1 // GROUP:i2 // GROUP],
                                             Z[:, i1 // GROUP:i2 // GROUP], MB, GROUP, fmt, True)
                else:
                    d.ops.gptq_block(W[:, i1:i2], Hinv[i1:i2, i1:i2], invd[i1:i2], Q[:, i1:i2], E, MB, fields, sc, zp)
        return f

    loops = {}
    for name, f in (("dynamic per_group 128", blocks(True)), ("static per-row", blocks(False))):
        f()
        torch.cuda.synchronize()
        ts = sorted(_timed(f) for _ in range(reps))
        loops[name] = ts[len(ts) // 2]
    header = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip()
    lines = [header,
             f"# tools/bench_gptq_group.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
             f"{time.strftime('%Y-%m-%d')}; apply() on a [{n},{n}] Linear, {FMT}, microblock {MB}, block {BLOCK}; medians of device-event "
             f"timings, fused {reps} runs / loop {loop_reps} runs, alternating"]
    lines += [f"apply(), {k}: {v:.2f} ms" for k, v in med.items()]
    ks = list(med)
    lines.append(f"apply(), fused dynamic / fused static: {med[ks[0]] / med[ks[2]]:.3f}; torch loop / fused dynamic: {med[ks[1]] / med[ks[0]]:.1f}x "
                 f"(every apply() includes the same factorisation, weight copy, diagonal inverses and trailing GEMMs)")
    nblk = n // BLOCK
    lines += [f"column loop alone ({nblk} launches, one per {BLOCK}-column block), {k}: {v:.2f} ms ({1000 * v / nblk:.1f} us per block)"
              for k, v in loops.items()]
    lines.append(f"column loop alone, dynamic / static: {loops['dynamic per_group 128'] / loops['static per-row']:.3f}")
    print("\n".join(lines), flush=True)
    if not quick:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r13_gptq_group.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
