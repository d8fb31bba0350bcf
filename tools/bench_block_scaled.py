"""The two-level block-scaled float cast on the GPU: ops.block_scaled_float_qdq with its group pass in ONE launch
(csrc/block_scaled_float.hip) beside the chain of launches that defines it (group_minmax -> the divisions by fmax and t -> float_qdq
with the scale format -> minimum, multiply, where -> scale_channels -> float_qdq -> scale_channels), beside ops.dynamic_float_qdq per
group of the same size (the float32-scale cast: the difference is the cost of the quantised scale) and beside the STATIC float_qdq of
the same tensor, on the same buffers.  Writes profiles/r18_block_scaled.txt (first line: tools/stamp.py --header).

Two settings per shape -- E2M1 in groups of 16 and E4M3 in groups of 128, both with an E4M3 scale capped at 448 -- each with a dynamic
and a static tensor scale t.  The dynamic-t figure is REDUCTION PLUS CAST: ops.group_minmax over the whole tensor as one group (the
flat reduction of csrc/reduce.hip), two one-element divisions and the rule t = 1 in torch, then the kernel; the static-t figure is the
kernel alone (t is a device tensor the kernel reads).

What decides the default route is this table: the class (ops.block_scaled_float_class) goes to the kernel by default only where it is
FASTER than the chain here; a row where it is not is marked, the exit status is 1, and the class belongs in
ops.BLOCK_SCALED_CHAIN_BY_DEFAULT.  The other two ratios are recorded, not asserted.

Method (tools/bench_dynamic_float.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are
captured into ONE graph per side (every call keeps its own output), so that a replay is back-to-back kernels without the host in
between; the graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of
(replay time / calls) and the spread.  % of 8 TB/s: the 4 B per element a one-pass cast must move, over the median.

    python tools/bench_block_scaled.py                  # the full table, written to profiles/
    python tools/bench_block_scaled.py --dry-run        # no GPU: the plan, nothing timed or written
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
SCALE_FORMAT, SCALE_MAX = "FP[1|4|3,7](_N)", 448.0
SETTINGS = {"e2m1g16": ("FP[1|2|1,1](_N)", 16), "e4m3g128": ("FP[1|4|3,7](_N)", 128)}
SHAPES = "8192x4096,8192x14336,2048x768"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated ROWSxCOLS (bf16)")
    ap.add_argument("--settings", default=",".join(SETTINGS), help=f"comma-separated, of {sorted(SETTINGS)}")
    ap.add_argument("--replays", type=int, default=11, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_block_scaled.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    shapes = []
    for r in a.shapes.split(","):
        if not r:
            continue
        shape = tuple(int(v) for v in r.lower().split("x"))
        if len(shape) != 2 or min(shape) < 1 or shape[1] % 128:
            ap.error(f"shape {r}: ROWSxCOLS with COLS a multiple of 128")
        shapes.append(shape)
    a.shapes = shapes
    a.settings = [s for s in a.settings.split(",") if s]
    for s in a.settings:
        if s not in SETTINGS:
            ap.error(f"setting {s}: one of {sorted(SETTINGS)}")
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def plan(args):
    """[(shape, setting, tensor scale kind, ring)] -- shared by the dry run and the timed run"""
    out = []
    for shape in args.shapes:
        nbytes = shape[0] * shape[1] * 2
        ring = min(160, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache (at most 160 inputs)
        for s in args.settings:
            for t in ("dynamic", "static"):
                out.append((shape, s, t, ring))
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, s, t, ring in rows:
            fmt, g = SETTINGS[s]
            print(f"{fmt} g{g}, {SCALE_FORMAT} scale <= {SCALE_MAX:g}, {t} t, {list(shape)} bf16: ring of {ring} inputs "
                  f"({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB) and as many outputs per graph; fused, chain, float32-scale cast and "
                  f"static cast; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_block_scaled.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; "
                 f"% = 4 B per bf16 element / median / 8 TB/s; scale format {SCALE_FORMAT} capped at {SCALE_MAX:g}; fused = "
                 f"ops.block_scaled_float_qdq(fused=True): with a static t (a device tensor) ONE launch, with a dynamic t the reduction "
                 f"(ops.group_minmax over the whole tensor as one group), two one-element divisions and the t = 1 rule in torch, then that "
                 f"launch -- reduction plus cast; chain = the same with fused=False (the same t, then group_minmax, two scale_channels "
                 f"divisions, float_qdq with the scale format, minimum, multiply, where, scale_channels, float_qdq, scale_channels, the "
                 f"signed-zero select; on more than 65535 groups on pieces of 32768 groups joined with torch.cat); dynf = "
                 f"ops.dynamic_float_qdq per group of the same size (one launch, float32 scales); static = ops.float_qdq (one launch, no "
                 f"reduction, no scale)")

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
    for shape, s, tk, ring_n in rows:
        if shape != ring_shape:
            ring = None
            ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(ring_n)]
            ring_shape = shape
        fmt, g = d.Format.from_shorthand(SETTINGS[s][0]), SETTINGS[s][1]
        cls = d.ops.block_scaled_float_class(g, torch.bfloat16)
        t = "dynamic" if tk == "dynamic" else d.ops.block_scaled_tensor_scale(ring[0], fmt, SCALE_FORMAT, SCALE_MAX)
        sides = [("fused", lambda x: d.ops.block_scaled_float_qdq(x, fmt, g, SCALE_FORMAT, SCALE_MAX, t, fused=True)),
                 ("chain", lambda x: d.ops.block_scaled_float_qdq(x, fmt, g, SCALE_FORMAT, SCALE_MAX, t, fused=False)),
                 ("dynf", lambda x: d.ops.dynamic_float_qdq(x, fmt, "per_group", g, fused=True)),
                 ("static", lambda x: d.ops.float_qdq(x, fmt.mantissa, fmt.exponent, fmt.bias, fmt.flush_subnormal))]
        graphs = [(label,) + graph_of(fn, ring) for label, fn in sides]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / len(ring))
        nbytes = 4 * shape[0] * shape[1]
        m = {k: med(v) for k, v in times.items()}
        line = f"{SETTINGS[s][0]} g{g} {tk} t {list(shape)} bf16 (class {cls}):"
        for label in ("fused", "chain", "dynf", "static"):
            v = times[label]
            line += f" {label} {m[label]:.1f} us [{min(v):.1f} .. {max(v):.1f}], {100.0 * nbytes / (m[label] * 1e-6) / PEAK:.0f} %;"
        line += f" chain / fused {m['chain'] / m['fused']:.2f}x, fused / dynf {m['fused'] / m['dynf']:.2f}x, fused / static {m['fused'] / m['static']:.2f}x"
        if m["fused"] >= m["chain"]:
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((cls, s, tk, shape))
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
