"""AWQ on the GPU: ops.awq_scaled_error in ONE launch (csrc/awq.hip) beside the four-launch chain that defines it
(scale_channels -> dynamic_fixed_qdq -> scale_channels to float32 -> the subtraction) on the same buffers, ops.channel_sumabs beside
torch's x.float().abs().sum(0), and the whole AWQCalibrator.apply() of one Linear split into its elementwise and its GEMM time.
Writes profiles/r17_awq.txt (first line: tools/stamp.py --header).

What decides the default route of awq_scaled_error is this table: a group size goes to the kernel by default only where it is FASTER
than the chain here; a row where it is not is marked, the exit status is 1, and the group size belongs in ops.AWQ_CHAIN_BY_DEFAULT.

Method (tools/bench_wanda.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are captured
into ONE graph per side (every call keeps its own output), so that a replay is back-to-back kernels without the host in between; the
graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of (replay time / calls)
and the spread.  apply() is timed eagerly as a whole, device events around the call and a synchronisation after it.

    python tools/bench_awq.py                  # the full table, written to profiles/
    python tools/bench_awq.py --dry-run        # no GPU: the plan, nothing timed or written
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
WEIGHT_SHAPES = "4096x4096,14336x4096,4096x14336"
SUMABS_SHAPES = "8192x4096,2048x768"
FMT, GROUP = "XP[4,0](CSN)", 128


def _shapes(ap, text, what, multiple):
    out = []
    for r in text.split(","):
        if not r:
            continue
        shape = tuple(int(v) for v in r.lower().split("x"))
        if len(shape) != 2 or min(shape) < 1 or shape[1] % multiple:
            ap.error(f"{what} {r}: ROWSxCOLS with COLS a multiple of {multiple}")
        out.append(shape)
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--weights", default=WEIGHT_SHAPES, help="comma-separated ROWSxCOLS of the weights (bf16)")
    ap.add_argument("--sumabs", default=SUMABS_SHAPES, help="comma-separated ROWSxCOLS of the activations (bf16)")
    ap.add_argument("--apply", default="4096x4096", help="OUTxIN of the Linear whose apply() is timed ('' to skip)")
    ap.add_argument("--n-grid", type=int, default=20, help="candidates of the timed apply()")
    ap.add_argument("--tokens", type=int, default=2048, help="calibration tokens of the timed apply()")
    ap.add_argument("--replays", type=int, default=15, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=3, help="untimed replays per side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_awq.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    a.weights, a.sumabs = _shapes(ap, a.weights, "weight", GROUP), _shapes(ap, a.sumabs, "activation", 1)
    a.apply = _shapes(ap, a.apply, "apply", GROUP)
    if a.replays < 3 or a.warmup < 1 or a.n_grid < 1 or a.tokens < 1:
        ap.error("at least 3 timed replays, 1 warm-up replay, 1 candidate and 1 token")
    return a


def ring_of(shape):
    """the ring holds 1.5 x the last-level cache (at most 160 inputs)"""
    return min(160, max(2, -(-(LLC_BYTES * 3 // 2) // (shape[0] * shape[1] * 2))))


def main(argv=None):
    args = parse_args(argv)
    if args.dry_run:
        for shape in args.weights:
            print(f"awq_scaled_error {FMT} g{GROUP} {list(shape)} bf16: ring of {ring_of(shape)} weights "
                  f"({ring_of(shape) * shape[0] * shape[1] * 2 / 2**20:.0f} MiB); fused and chain; {args.warmup} + {args.replays} replays per side")
        for shape in args.sumabs:
            print(f"channel_sumabs {list(shape)} bf16: ring of {ring_of(shape)} inputs; kernel and torch; {args.warmup} + {args.replays} replays per side")
        for shape in args.apply:
            print(f"apply() of a Linear({shape[1]}, {shape[0]}) bf16, {FMT} g{GROUP}, n_grid {args.n_grid}, {args.tokens} tokens: whole, "
                  f"elementwise part and GEMM part, 3 timed runs each after one warm-up")
        return 0

    import torch
    import dmx_compressor_amd as d

    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_awq.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events.  "
                 f"awq_scaled_error ({FMT}, groups of {GROUP}, affine scheme): fused = one dmxq_awq_group_error launch writing the float32 "
                 f"error alone (% = 6 B per bf16 element / median / 8 TB/s), chain = scale_channels (bf16) -> dynamic_fixed_qdq (its kernel) -> "
                 f"scale_channels (divide, float32) -> torch's subtraction of w.float() (% = the same 6 B: what the result needs, not what "
                 f"the chain moves).  channel_sumabs: kernel = ops.channel_sumabs into one float64 [C] vector (two launches), torch = "
                 f"x.float().abs().sum(0) (float32 sums: NOT the definition); % = 2 B per bf16 element / median / 8 TB/s.  apply(): "
                 f"AWQCalibrator.apply() of one Linear, eager, ms per call")

    def graph_of(fn, ring):
        for x in ring[:2]:
            fn(x)                       # eager warm-up: code objects, allocator
        torch.cuda.synchronize()
        g, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            for x in ring:
                keep.append(fn(x))      # (every call's output stays alive: as many output buffers as inputs)
        return g, keep

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def med(v):
        return sorted(v)[len(v) // 2]

    def measure(sides, ring):
        graphs = [(label,) + graph_of(fn, ring) for label, fn in sides]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                event_ms(gr.replay)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * event_ms(gr.replay) / len(ring))
        del graphs
        return times

    def cell(label, t, nbytes):
        m = med(t)
        return f" {label} {m:.1f} us [{min(t):.1f} .. {max(t):.1f}], {100.0 * nbytes / (m * 1e-6) / PEAK:.0f} %;"

    gen = torch.Generator(device=dev).manual_seed(0)
    slower = []
    for shape in args.weights:
        ring = [(torch.randn(shape, generator=gen, device=dev) * 0.05).to(bf16) for _ in range(ring_of(shape))]
        s = d.ops.awq_candidate_scales(torch.rand(shape[1], generator=gen, device=dev) * 3 + 0.1, 4)[2]
        n = shape[0] * shape[1]
        t = measure([("fused", lambda w: d.ops.awq_scaled_error(w, s, FMT, GROUP, fused=True)),
                     ("chain", lambda w: d.ops.awq_scaled_error(w, s, FMT, GROUP, fused=False))], ring)
        line = f"awq_scaled_error g{GROUP} {list(shape)} bf16:" + cell("fused", t["fused"], 6 * n) + cell("chain", t["chain"], 6 * n)
        line += f" chain / fused {med(t['chain']) / med(t['fused']):.2f}x"
        if med(t["fused"]) >= med(t["chain"]):
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((GROUP, shape))
        print(line, flush=True)
        lines.append(line)
        del ring

    for shape in args.sumabs:
        ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(bf16) for _ in range(ring_of(shape))]
        acc = torch.zeros(shape[1], dtype=torch.float64, device=dev)
        t = measure([("kernel", lambda x: d.ops.channel_sumabs(x, out=acc)), ("torch", lambda x: x.float().abs().sum(0))], ring)
        nbytes = 2 * shape[0] * shape[1]
        line = f"channel_sumabs {list(shape)} bf16:" + cell("kernel", t["kernel"], nbytes) + cell("torch", t["torch"], nbytes)
        line += f" torch / kernel {med(t['torch']) / med(t['kernel']):.2f}x"
        print(line, flush=True)
        lines.append(line)
        del ring

    for out_f, in_f in args.apply:
        m = d.nn.Linear(in_f, out_f).to(dev, bf16).eval()
        m.configure({"weight_format": FMT, "weight_dynamic": {"per_group": GROUP}})
        x = (torch.randn(args.tokens, in_f, generator=gen, device=dev) * 0.7).to(bf16)
        x[:, ::97] *= 30.0
        hp = d.DmxAWQHyperparams(n_grid=args.n_grid)
        with torch.no_grad():
            with m.awq_scaling(hp):
                m(x)                                  # (the first apply(), on leaving: the warm-up)
            whole = []
            for _ in range(3):
                m.smoothquant.disable()
                m.enable_awq(True, d.DmxAWQHyperparams(n_grid=args.n_grid, reset=False))   # the same statistics again
                whole.append(event_ms(lambda: m.enable_awq(False, hp)))
            w, gram = m.weight.detach(), m.awq_gram
            scales = d.ops.awq_candidate_scales(m.awq_x_mean, args.n_grid, m.smoothquant.scale_cast)
            errs = [d.ops.awq_scaled_error(w, scales[k], FMT, GROUP) for k in range(2)]
            ew, mm = [], []
            for _ in range(3):
                ew.append(event_ms(lambda: [d.ops.awq_scaled_error(w, scales[k], FMT, GROUP) for k in range(args.n_grid)]))
                with d.ops._front._full_fp32_matmul():
                    mm.append(event_ms(lambda: [((errs[k % 2] @ gram) * errs[k % 2]).sum(dtype=torch.float64) for k in range(args.n_grid)]))
        line = (f"apply() Linear({in_f}, {out_f}) bf16 {FMT} g{GROUP}, n_grid {args.n_grid}, {args.tokens} tokens: whole {med(whole):.2f} ms "
                f"[{min(whole):.2f} .. {max(whole):.2f}]; its {args.n_grid} awq_scaled_error calls alone {med(ew):.2f} ms "
                f"[{min(ew):.2f} .. {max(ew):.2f}]; its {args.n_grid} float32 GEMMs with the product and the float64 sum alone {med(mm):.2f} ms "
                f"[{min(mm):.2f} .. {max(mm):.2f}]: elementwise {100 * med(ew) / med(whole):.0f} %, GEMM {100 * med(mm) / med(whole):.0f} % of the whole")
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
