"""AdaRound on the GPU: ops.adaround_qdq and ops.adaround_backward in ONE pass each (csrc/adaround.hip) beside the chain of torch
operations that spells the same definition, on the same buffers, and one whole AdaRoundCalibrator.apply().  Writes
profiles/r24_adaround.txt (first line: tools/stamp.py --header).

Byte counts only say which way it should go: per bf16 element with a float32 output the forward moves 2 + 4 + 4 = 10 B and the backward
2 + 4 + 4 + 4 = 14 B (the float32 gradient in, dV out); the chain makes 10 to 25 elementwise passes over float32 temporaries.  Whether
the kernels are bound by HBM or by the VALU (expf, powf) is what this table shows.  What decides the default route is this table: a
class (ops.adaround_class) goes to the kernel by default only where it is FASTER than the chain here; a row where it is not is
marked, the exit status is 1, and the class belongs in ops.ADAROUND_CHAIN_BY_DEFAULT.

Method (tools/bench_lsq.py's): each side's calls over a ring of (w, V, g) triples larger than the 256 MiB last-level cache are captured
into ONE graph per side (every call keeps its own outputs); the two graphs of a row are replayed in turn, device events around every
replay; per side the median over the replays of (replay time / calls) and the spread.

    python tools/bench_adaround.py                  # the full table, written to profiles/
    python tools/bench_adaround.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
PEAK = 8e12                       # HBM3E of an MI355X, bytes per second
FORMAT = "XP[4,0](C_N)"
BETA, REG_WEIGHT = 8.0, 0.01      # a mid-schedule step: the regulariser's powf runs


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="4096x4096,14336x4096,2048x768", help="comma-separated ROWSxCOLS (bf16); a shape whose COLS are no multiple of the group size is not measured per group")
    ap.add_argument("--group", type=int, default=128, help="the per_group size")
    ap.add_argument("--replays", type=int, default=11, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--apply-shape", default="4096x4096", help="the Linear (OUTxIN) whose whole apply() is timed; empty: none")
    ap.add_argument("--apply-steps", type=int, default=100, help="Adam steps of the timed apply()")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_adaround.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    a.shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",") if s]
    a.apply_shape = tuple(int(v) for v in a.apply_shape.lower().split("x")) if a.apply_shape else None
    for s in a.shapes + ([a.apply_shape] if a.apply_shape else []):
        if len(s) != 2 or min(s) < 1 or s[1] % 8:
            ap.error(f"shape {s}: ROWSxCOLS with COLS a multiple of 8")
    if a.replays < 3 or a.warmup < 1 or a.apply_steps < 1:
        ap.error("at least 3 timed replays, 1 warm-up replay and 1 step")
    return a


def plan(args):
    """[(shape, granularity, group size, ring)] -- shared by the dry run and the timed run"""
    rows = []
    for shape in args.shapes:
        nbytes = shape[0] * shape[1] * (2 + 4 + 4)   # w, V and the float32 gradient
        ring = min(32, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache (at most 32 triples)
        for granularity, g in (("per_group", args.group), ("per_token", None), ("per_tensor", None)):
            if g is not None and shape[1] % g:
                continue
            rows.append((shape, granularity, g, ring))
    return rows


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, granularity, g, ring in rows:
            print(f"{FORMAT} {granularity}{'' if g is None else ' ' + str(g)} {list(shape)} bf16, float32 output and gradient: ring of {ring} "
                  f"(w, V, g) triples ({ring * shape[0] * shape[1] * 10 / 2**20:.0f} MiB) per graph; forward and backward, fused and chain; "
                  f"{args.warmup} + {args.replays} replays per side")
        if args.apply_shape:
            print(f"apply(): a {list(args.apply_shape)} bf16 Linear, weight_dynamic per group {args.group}, {args.apply_steps} Adam steps; "
                  f"the same count of forward + backward launches and of float32 GEMMs timed on their own")
        return 0

    import torch
    import dmx_compressor_amd as d

    dev = torch.device("cuda:0")
    bf16, f32 = torch.bfloat16, torch.float32
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_adaround.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the two graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; "
                 f"% = 10 B (forward) or 14 B (backward) per bf16 element / median / 8 TB/s; bf16 weight, float32 output and gradient (the "
                 f"module path); forward = ops.adaround_qdq soft; backward = ops.adaround_backward with beta {BETA}, reg_weight {REG_WEIGHT} "
                 f"and the regulariser's sum (two launches); fused=True against fused=False (the definition in torch operations); class = "
                 f"ops.adaround_class of the row.  Not measured: f16 / f32 weights, other group sizes, hard mode")

    def graph_of(fn, ring):
        for p in ring[:2]:
            fn(*p)                      # eager warm-up: code objects, allocator
        torch.cuda.synchronize()
        g, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            for p in ring:
                keep.append(fn(*p))     # (every call's outputs stay alive)
        return g, keep

    def replay_ms(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def med(v):
        return sorted(v)[len(v) // 2]

    slower = []
    gen = torch.Generator(device=dev).manual_seed(0)
    ring_shape, ring = None, None
    fmt = d.Format.from_shorthand(FORMAT)
    for shape, granularity, g, ring_n in rows:
        if shape != ring_shape:
            ring = None
            ring = [((torch.randn(shape, generator=gen, device=dev) * 0.7).to(bf16), torch.rand(shape, generator=gen, device=dev) * 8.0 - 4.0,
                     torch.randn(shape, generator=gen, device=dev)) for _ in range(ring_n)]
            ring_shape = shape
        S = {"per_group": g, "per_token": shape[1], "per_tensor": shape[0] * shape[1]}[granularity]
        n_seg = shape[0] * shape[1] // S
        s = (torch.rand(n_seg, generator=gen, device=dev) + 0.5) * (1.4 / 7)   # (a good share of the elements is clipped)
        z = torch.randint(-3, 4, (n_seg,), generator=gen, device=dev).float()
        cls = d.ops.adaround_class(S, bf16, granularity)
        for what, per_elem, make in (
                ("forward", 10, lambda fused: (lambda w, V, gr: d.ops.adaround_qdq(w, V, s, z, fmt, granularity, g, out_dtype=f32, fused=fused))),
                ("backward", 14, lambda fused: (lambda w, V, gr: d.ops.adaround_backward(w, V, gr, s, z, fmt, granularity, g, beta=BETA,
                                                                                           reg_weight=REG_WEIGHT, fused=fused)))):
            graphs = [(label,) + graph_of(make(fused), ring) for label, fused in (("fused", True), ("chain", False))]
            for _ in range(args.warmup):
                for _, gr, _ in graphs:
                    replay_ms(gr)
            times = {label: [] for label, _, _ in graphs}
            for _ in range(args.replays):
                for label, gr, _ in graphs:
                    times[label].append(1000.0 * replay_ms(gr) / len(ring))
            nbytes = per_elem * shape[0] * shape[1]
            m = {k: med(v) for k, v in times.items()}
            line = f"{FORMAT} {granularity}{'' if g is None else ' ' + str(g)} {list(shape)} bf16 {what} (class {cls}):"
            for label in ("fused", "chain"):
                t = times[label]
                line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}], {100.0 * nbytes / (m[label] * 1e-6) / PEAK:.0f} %;"
            line += f" chain / fused {m['chain'] / m['fused']:.2f}x"
            if m["fused"] >= m["chain"]:
                line += " ** NOT FASTER THAN THE CHAIN **"
                slower.append((cls, what, granularity, shape))
            print(line, flush=True)
            lines.append(line)
            del graphs
    ring = None

    if args.apply_shape:
        out_f, in_f = args.apply_shape
        steps = args.apply_steps
        torch.manual_seed(0)
        lin = d.nn.Linear(in_f, out_f).to(dev).to(bf16)
        lin.configure({"weight_format": FORMAT, "weight_dynamic": {"per_group": args.group}})
        x = torch.randn(2048, in_f, device=dev, dtype=bf16)
        hp = d.DmxAdaRoundHyperparams(iters=steps)

        def timed(fn):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        with torch.no_grad():
            lin.enable_adaround(True, hp)
            lin(x)
            rounder, lin.adarounder = lin.adarounder, None
            W = lin.weight.detach().clone()
            rounder.apply()                       # warm-up
            lin.weight.copy_(W)
            lin.weight_cast.enable_fake_quant()
            t_apply = []
            for _ in range(3):
                t_apply.append(timed(rounder.apply))
                lin.weight.copy_(W)
                lin.weight_cast.enable_fake_quant()
            sc, zp = rounder.qparams(W)
            zf = zp.float()
            V = d.ops.adaround_init(W, sc, zp, fmt, "per_group", args.group)
            gD = torch.randn(out_f, in_f, device=dev)
            G = rounder.gram

            def kernels():
                for _ in range(steps):
                    d.ops.adaround_qdq(W, V, sc, zf, fmt, "per_group", args.group, out_dtype=f32)
                    d.ops.adaround_backward(W, V, gD, sc, zf, fmt, "per_group", args.group, beta=BETA, reg_weight=REG_WEIGHT, want_reg=False)

            def gemms():
                with d.ops._front._full_fp32_matmul():
                    for _ in range(steps):
                        gD @ G

            kernels(), gemms()
            t_k = med([timed(kernels) for _ in range(3)])
            t_g = med([timed(gemms) for _ in range(3)])
        t_a = med(t_apply)
        line = (f"apply() of a [{out_f}, {in_f}] bf16 Linear, weight_dynamic per group {args.group}, {steps} Adam steps, 2048 tokens observed: "
                f"{t_a:.1f} ms [{min(t_apply):.1f} .. {max(t_apply):.1f}]; on their own, {steps} forward + backward launches {t_k:.1f} ms "
                f"({100.0 * t_k / t_a:.0f} %), {steps} float32 [{out_f}, {in_f}] x [{in_f}, {in_f}] GEMMs {t_g:.1f} ms ({100.0 * t_g / t_a:.0f} %); "
                f"the rest is the subtraction, the scaling of the gradient, Adam and the two loss evaluations")
        print(line, flush=True)
        lines.append(line)

    lines.append("# every fused row is faster than its chain" if not slower else f"# NOT FASTER THAN THE CHAIN: {slower}")
    print(lines[-1], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
