"""GPTQ apply() on the GPU: the fused column kernel (csrc/gptq.hip) against the reference-shaped loop (`fuse_gptq = False`), in the
same process, alternating, device events around each apply() after a warm-up; then the fused path's split into factorisation
(cholesky -> cholesky_inverse -> upper cholesky), in-block kernel launches and trailing GEMMs, each timed on its own.
Writes profiles/r07_gptq.txt.  The kernel's own time: `rocprofv3 --kernel-trace --stats -- python tools/bench_gptq.py --quick`."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dmx_compressor_amd as d  # noqa: E402
from dmx_compressor_amd.layer_reconstruction import OptimalBrainCompressor  # noqa: E402


def _events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def run(rows, cols, fmt, mb, reps, loop_reps):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = d.nn.Linear(cols, rows, bias=False).to(dev)
    m.configure({"weight_format": fmt})
    W0 = m.weight.detach().clone()
    X = torch.randn(2048, cols, device=dev)
    obc = OptimalBrainCompressor(m)
    obc.measure_hessian(X.unsqueeze(0))
    H0 = obc.H.clone()

    def apply(fuse):
        def f():
            m.fuse_gptq = fuse
            with torch.no_grad():
                m.weight.copy_(W0)
            o = OptimalBrainCompressor(m)
            o.H = H0.clone()
            o.apply(microblock_size=mb, block_size=128)
        return f

    apply(True)()
    apply(False)()
    torch.cuda.synchronize()
    fused, loop = [], []
    for _ in range(max(reps, loop_reps)):   # alternating
        if len(fused) < reps:
            fused.append(_events(apply(True), 1))
        if len(loop) < loop_reps:
            loop.append(_events(apply(False), 1))
    tf, tl = sorted(fused)[len(fused) // 2], sorted(loop)[len(loop) // 2]
    # the fused path's pieces, each on its own
    H = H0.clone()
    damp = 0.01 * torch.mean(torch.diag(H))
    H[range(cols), range(cols)] += damp

    def factor():
        Hc = torch.linalg.cholesky(H)
        Hc = torch.cholesky_inverse(Hc)
        return torch.linalg.cholesky(Hc, upper=True).contiguous()

    t_fact = _events(factor, reps)
    Hinv = factor()
    fields = d.ops.gptq_fields(d.Format.from_shorthand(fmt))
    W = W0.float().clone()
    Q = torch.empty_like(W)
    E = torch.empty(rows, 128, device=dev)
    invd = OptimalBrainCompressor._inv_diag(Hinv, mb)

    def kernels():
        for i1 in range(0, cols, 128):
            i2 = min(i1 + 128, cols)
            dblk = invd[i1:i2] if mb == 1 else invd[i1 // mb:-(-i2 // mb)]
            d.ops.gptq_block(W[:, i1:i2], Hinv[i1:i2, i1:i2], dblk, Q[:, i1:i2], E[:, :i2 - i1], mb, fields)

    def gemms():
        for i1 in range(0, cols, 128):
            i2 = min(i1 + 128, cols)
            if i2 < cols:
                W[:, i2:].addmm_(E[:, :i2 - i1], Hinv[i1:i2, i2:], alpha=-1)

    t_kern, t_gemm = _events(kernels, reps), _events(gemms, reps)
    t_inv = _events(lambda: OptimalBrainCompressor._inv_diag(Hinv, mb), reps)
    nblk = -(-cols // 128)
    return (f"[{rows},{cols}] {fmt} mb {mb}: apply() fused {tf:.2f} ms, loop {tl:.2f} ms, speed-up {tl / tf:.1f}x | fused split: "
            f"factorisation {t_fact:.2f} ms, in-block kernel {t_kern:.2f} ms ({1000 * t_kern / nblk:.1f} us per 128-column block), "
            f"trailing GEMMs {t_gemm:.2f} ms, diagonal-block inverses (one batched call) {t_inv:.2f} ms")


def main():
    quick = "--quick" in sys.argv
    shapes = [(4096, 4096), (14336, 4096)]
    fmts = [("FP[1|4|3,7](_N)", 1), ("BFP[8|8]{64}(SN)", 64)]
    reps, loop_reps = (1, 1) if quick else (5, 2)
    lines = [f"# tools/bench_gptq.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
             f"{time.strftime('%Y-%m-%d')}; medians of device-event timings, fused {reps} runs / loop {loop_reps} runs, alternating"]
    for rows, cols in shapes[:1] if quick else shapes:
        for fmt, mb in fmts:
            line = run(rows, cols, fmt, mb, reps, loop_reps)
            print(line, flush=True)
            lines.append(line)
    if not quick:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r07_gptq.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
