"""HQQ on the GPU: ops.hqq_qdq in ONE launch (csrc/hqq.hip) beside the chain of torch operations that defines it (fused=False), at
iters = 20 and at iters = 0, and beside ops.dynamic_fixed_qdq per group of the same size -- the single-pass floor the kernel at
iters = 0 should sit near -- all on the same buffers.  Writes profiles/r21_hqq.txt (first line: tools/stamp.py --header).

What decides the default route is this table: the class (ops.hqq_class) goes to the kernel by default only where it is FASTER than the
chain here; a row where it is not is marked, the exit status is 1, and the class belongs in ops.HQQ_CHAIN_BY_DEFAULT.  The kernel's time
per iteration, (iters=20 - iters=0) / 20, and the ratio to the dynamic cast are recorded, not asserted.

Method (tools/bench_codebook.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are
captured into ONE graph per side (every call keeps its own output), so that a replay is back-to-back kernels without the host in
between; the graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of
(replay time / calls) and the spread.

    python tools/bench_hqq.py                  # the full table, written to profiles/
    python tools/bench_hqq.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
ROWS = "4096x4096:64,4096x4096:128,14336x4096:64,14336x4096:128,2048x768:64,2048x768:128"
SIDES = ("fused20", "chain20", "fused0", "chain0", "dynamic")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default=ROWS, help="comma-separated ROWSxCOLS:GROUP (bf16)")
    ap.add_argument("--format", default="XP[4,0](CSN)", help="the integer format")
    ap.add_argument("--lp-norm", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20, help="the iteration count of the fused20 / chain20 sides")
    ap.add_argument("--replays", type=int, default=9, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--max-ring", type=int, default=160, help="the most inputs of a ring (the chain at 20 iterations is some 300 passes per call)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_hqq.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    rows = []
    for r in a.rows.split(","):
        if not r:
            continue
        shape, _, g = r.partition(":")
        shape = tuple(int(v) for v in shape.lower().split("x"))
        if len(shape) != 2 or min(shape) < 1 or not g.isdigit() or int(g) < 1 or shape[1] % int(g):
            ap.error(f"row {r}: ROWSxCOLS:GROUP with GROUP dividing COLS")
        rows.append((shape, int(g)))
    a.rows = rows
    if a.replays < 3 or a.warmup < 1 or a.iters < 1:
        ap.error("at least 3 timed replays, 1 warm-up replay and 1 iteration")
    return a


def plan(args):
    """[(shape, group size, ring)] -- shared by the dry run and the timed run"""
    out = []
    for shape, g in args.rows:
        nbytes = shape[0] * shape[1] * 2
        ring = min(args.max_ring, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache where max-ring allows
        out.append((shape, g, ring))
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, g, ring in rows:
            print(f"{args.format} g {g} {list(shape)} bf16: ring of {ring} inputs ({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB) and as many "
                  f"outputs per graph; {', '.join(SIDES)}; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    ops = d.ops
    dev = torch.device("cuda:0")
    fmt, lp, it = args.format, args.lp_norm, args.iters
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_hqq.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; rings of at most "
                 f"{args.max_ring} inputs; fused20 / fused0 = ops.hqq_qdq(fused=True) at iters = {it} / 0 (one launch), chain20 / chain0 = the same "
                 f"with fused=False (the definition in torch operations; on more than 65535 groups on pieces of 32768 joined with torch.cat), "
                 f"dynamic = ops.dynamic_fixed_qdq per_group of the same size (one launch, the single-pass floor); format {fmt}, lp_norm {lp}, "
                 f"beta 10, kappa 1.01; per iteration = (fused20 - fused0) / {it}; class = ops.hqq_class of the row")

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

    slower = []
    gen = torch.Generator(device=dev).manual_seed(0)
    ring_shape, ring = None, None
    for shape, g, ring_n in rows:
        if shape != ring_shape:
            ring = None
            ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(ring_n)]
            ring_shape = shape
        cls = ops.hqq_class(g, torch.bfloat16)
        sides = [("fused20", lambda x: ops.hqq_qdq(x, fmt, g, lp, iters=it, fused=True)),
                 ("chain20", lambda x: ops.hqq_qdq(x, fmt, g, lp, iters=it, fused=False)),
                 ("fused0", lambda x: ops.hqq_qdq(x, fmt, g, lp, iters=0, fused=True)),
                 ("chain0", lambda x: ops.hqq_qdq(x, fmt, g, lp, iters=0, fused=False)),
                 ("dynamic", lambda x: ops.dynamic_fixed_qdq(x, fmt, "per_group", g, fused=True))]
        graphs = [(label,) + graph_of(fn, ring) for label, fn in sides]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / len(ring))
        m = {k: med(v) for k, v in times.items()}
        line = f"{fmt} g {g} {list(shape)} bf16 (class {cls}, ring {len(ring)}):"
        for label in SIDES:
            t = times[label]
            line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}];"
        line += (f" chain20 / fused20 {m['chain20'] / m['fused20']:.1f}x, chain0 / fused0 {m['chain0'] / m['fused0']:.1f}x, "
                 f"fused0 / dynamic {m['fused0'] / m['dynamic']:.2f}x, per iteration {(m['fused20'] - m['fused0']) / it:.2f} us")
        if m["fused20"] >= m["chain20"] or m["fused0"] >= m["chain0"]:
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((cls, g, shape))
        print(line, flush=True)
        lines.append(line)
        del graphs
    lines.append("# every fused row is faster than its chain" if not slower else f"# NOT FASTER THAN THE CHAIN: {slower}")
    print(lines[-1], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
