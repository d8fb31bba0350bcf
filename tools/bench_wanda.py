"""Wanda on the GPU: ops.channel_sumsq beside torch's x.float().pow(2).sum(0), and ops.wanda_nm_sparsify in ONE pass
over the weight (csrc/wanda.hip) beside the chain that defines it (ops.wanda_score, then ops.nm_sparsify) and beside ops.nm_sparsify
on a READY float32 score, on the same buffers.  Writes profiles/r16_wanda.txt (first line: tools/stamp.py --header).

What decides the default route of wanda_nm_sparsify is this table: a group size goes to the kernel by default only where it is FASTER
than the chain here; a row where it is not is marked, the exit status is 1, and the group size belongs in ops.WANDA_CHAIN_BY_DEFAULT.
channel_sumsq accumulates in float64 by definition; how far that leaves it from the plain read of the input (2 B per bf16 element over
8 TB/s) is recorded, not asserted.

Method (tools/bench_dynamic_float.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are
captured into ONE graph per side (every call keeps its own output), so that a replay is back-to-back kernels without the host in
between; the graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of
(replay time / calls) and the spread.

    python tools/bench_wanda.py                  # the full table, written to profiles/
    python tools/bench_wanda.py --dry-run        # no GPU: the plan, nothing timed or written
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
SUMSQ_SHAPES = "8192x4096,8192x14336,2048x768"
WANDA_SHAPES = "4096x4096,14336x4096"
PATTERNS = "2:4,4:8"


def _shapes(ap, text, what):
    out = []
    for r in text.split(","):
        if not r:
            continue
        shape = tuple(int(v) for v in r.lower().split("x"))
        if len(shape) != 2 or min(shape) < 1 or shape[1] % 16:
            ap.error(f"{what} {r}: ROWSxCOLS with COLS a multiple of 16")
        out.append(shape)
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sumsq", default=SUMSQ_SHAPES, help="comma-separated ROWSxCOLS of the activations (bf16)")
    ap.add_argument("--weights", default=WANDA_SHAPES, help="comma-separated ROWSxCOLS of the weights (bf16)")
    ap.add_argument("--patterns", default=PATTERNS, help="comma-separated K:M")
    ap.add_argument("--replays", type=int, default=15, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=3, help="untimed replays per side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_wanda.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    a.sumsq, a.weights = _shapes(ap, a.sumsq, "activation"), _shapes(ap, a.weights, "weight")
    pats = []
    for p in a.patterns.split(","):
        k, _, m = p.partition(":")
        if not (k.isdigit() and m.isdigit() and int(m) in (4, 8, 16) and 1 <= int(k) <= int(m)):
            ap.error(f"pattern {p}: K:M with M in 4, 8, 16")
        pats.append((int(k), int(m)))
    a.patterns = pats
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def ring_of(shape):
    """the ring holds 1.5 x the last-level cache (at most 160 inputs)"""
    return min(160, max(2, -(-(LLC_BYTES * 3 // 2) // (shape[0] * shape[1] * 2))))


def main(argv=None):
    args = parse_args(argv)
    if args.dry_run:
        for shape in args.sumsq:
            print(f"channel_sumsq {list(shape)} bf16: ring of {ring_of(shape)} inputs ({ring_of(shape) * shape[0] * shape[1] * 2 / 2**20:.0f} MiB); "
                  f"kernel and torch; {args.warmup} + {args.replays} replays per side")
        for shape in args.weights:
            for K, M in args.patterns:
                print(f"wanda_nm_sparsify {K}:{M} {list(shape)} bf16: ring of {ring_of(shape)} weights; y only and score + mask: fused, chain "
                      f"and nm_sparsify on a ready score; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_wanda.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events.  "
                 f"channel_sumsq: kernel = ops.channel_sumsq into one float64 [C] vector (two launches: slab partials, fold), torch = "
                 f"x.float().pow(2).sum(0) (float32 sums: NOT the definition, the nearest thing torch has at this cost); % = 2 B per bf16 "
                 f"element / median / 8 TB/s.  wanda_nm_sparsify: fused = one dmxq_wanda_nm launch, chain = ops.wanda_score (fused) then "
                 f"ops.nm_sparsify on the stored score, ready = ops.nm_sparsify on a float32 score that already exists (what a forward "
                 f"pays after calibration); 'y' = W * mask alone in bf16 (% = 4 B per element / median / 8 TB/s), 'score+mask' = the float32 "
                 f"score and mask the context writes (% = 10 B per element)")

    def graph_of(fn, ring):
        for x in ring[:2]:
            fn(x)                       # eager warm-up: code objects, allocator
        torch.cuda.synchronize()
        g, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            for x in ring:
                keep.append(fn(x))      # (every call's output stays alive: as many output buffers as inputs)
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

    def measure(sides, ring):
        graphs = [(label,) + graph_of(fn, ring) for label, fn in sides]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / len(ring))
        del graphs
        return times

    def cell(label, t, nbytes):
        m = med(t)
        return f" {label} {m:.1f} us [{min(t):.1f} .. {max(t):.1f}], {100.0 * nbytes / (m * 1e-6) / PEAK:.0f} %;"

    gen = torch.Generator(device=dev).manual_seed(0)
    for shape in args.sumsq:
        ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(ring_of(shape))]
        acc = torch.zeros(shape[1], dtype=torch.float64, device=dev)
        times = measure([("kernel", lambda x: d.ops.channel_sumsq(x, out=acc)), ("torch", lambda x: x.float().pow(2).sum(0))], ring)
        nbytes = 2 * shape[0] * shape[1]
        line = f"channel_sumsq {list(shape)} bf16:" + cell("kernel", times["kernel"], nbytes) + cell("torch", times["torch"], nbytes)
        line += f" torch / kernel {med(times['torch']) / med(times['kernel']):.2f}x"
        print(line, flush=True)
        lines.append(line)
        del ring

    slower = []
    for shape in args.weights:
        ring = [(torch.randn(shape, generator=gen, device=dev) * 0.05).to(torch.bfloat16) for _ in range(ring_of(shape))]
        an = torch.rand(shape[1], generator=gen, device=dev) * 3 + 0.1
        ready = d.ops.wanda_score(ring[0], an)
        n = shape[0] * shape[1]
        for K, M in args.patterns:
            bf16 = torch.bfloat16
            t = measure([("fused", lambda w: d.ops.wanda_nm_sparsify(w, an, K, M, fused=True, out_dtype=bf16)),
                         ("chain", lambda w: d.ops.nm_sparsify(w, d.ops.wanda_score(w, an), K, M, out_dtype=bf16)),
                         ("ready", lambda w: d.ops.nm_sparsify(w, ready, K, M, out_dtype=bf16))], ring)
            line = f"wanda_nm_sparsify {K}:{M} {list(shape)} bf16, y:" + "".join(cell(k, t[k], 4 * n) for k in ("fused", "chain", "ready"))
            line += f" chain / fused {med(t['chain']) / med(t['fused']):.2f}x, fused / ready {med(t['fused']) / med(t['ready']):.2f}x"
            if med(t["fused"]) >= med(t["chain"]):
                line += " ** NOT FASTER THAN THE CHAIN **"
                slower.append((M, "y", shape))
            print(line, flush=True)
            lines.append(line)
            t = measure([("fused", lambda w: d.ops.wanda_nm_sparsify(w, an, K, M, return_mask=True, return_score=True, return_y=False, fused=True)),
                         ("chain", lambda w: (lambda s: (d.ops.nm_mask(s, K, M), s))(d.ops.wanda_score(w, an))),
                         ("ready", lambda w: d.ops.nm_mask(ready, K, M))], ring)
            line = f"wanda_nm_sparsify {K}:{M} {list(shape)} bf16, score+mask:" + cell("fused", t["fused"], 10 * n) + cell("chain", t["chain"], 10 * n)
            line += f" nm_mask on a ready score {med(t['ready']):.1f} us; chain / fused {med(t['chain']) / med(t['fused']):.2f}x"
            if med(t["fused"]) >= med(t["chain"]):
                line += " ** NOT FASTER THAN THE CHAIN **"
                slower.append((M, "score+mask", shape))
            print(line, flush=True)
            lines.append(line)
        del ring, ready
    lines.append("# every fused row is faster than its chain" if not slower else f"# NOT FASTER THAN THE CHAIN: {slower}")
    print(lines[-1], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
