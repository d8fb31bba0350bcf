"""The dynamic casts along a non-last dimension on the GPU: ops.dynamic_fixed_qdq / ops.dynamic_float_qdq with dim != -1 in ONE launch
(csrc/dynamic_cols.hip, fused=True) beside the transposing route that defines them (fused=False: movedim().contiguous() -> the last-dim
kernel -> movedim().contiguous()) and beside the last-dim kernel on a tensor of the same size (the 4 B per bf16 element bound), all on
the same buffers.  Writes profiles/r27_dynamic_cols.txt (first line: tools/stamp.py --header).

What decides the default route is this table: a class (ops.dynamic_cols_class) goes to the kernel by default only where it is FASTER
than the transposing route here; a row where it is not is marked, the exit status is 1, and the class belongs in
ops.DYNAMIC_COLS_CHAIN_BY_DEFAULT.

Method (tools/bench_outlier.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are captured
into ONE graph per side (every call keeps its own output); the graphs of a row are replayed in turn, device events around every
replay; per side the median over the replays of (replay time / calls) and the spread.

    python tools/bench_dynamic_cols.py                  # the full table, written to profiles/
    python tools/bench_dynamic_cols.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
INT4, E4M3 = "XP[4,0](C_N)", "FP[1|4|3,7](FN)"
# (name, shape, dtype, format, group size, dim): the issue's rows, and one row per remaining class / depth so that none stays unmeasured
ROWS = [("keys", (8, 32, 4096, 128), "bf16", INT4, 32, -2), ("keys", (8, 32, 4096, 128), "bf16", INT4, 128, -2),
        ("conv1d weight", (4096, 4096), "bf16", INT4, 128, 0), ("activations", (8192, 4096), "bf16", E4M3, 128, 0),
        ("small", (2048, 768), "bf16", INT4, 128, 0), ("small", (2048, 768), "bf16", E4M3, 128, 0),
        ("weight g16", (4096, 4096), "bf16", INT4, 16, 0), ("weight g64", (4096, 4096), "bf16", INT4, 64, 0),
        ("weight f32 g256", (4096, 4096), "f32", INT4, 256, 0), ("weight g256", (4096, 4096), "bf16", INT4, 256, 0)]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--replays", type=int, default=9, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--max-ring", type=int, default=64, help="the most inputs of a ring")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_dynamic_cols.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def plan(args):
    out = []
    for name, shape, dt, fmt, g, dim in ROWS:
        n = 1
        for v in shape:
            n *= v
        nbytes = n * (4 if dt == "f32" else 2)
        ring = min(args.max_ring, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # 1.5 x the last-level cache where max-ring allows
        out.append((name, shape, dt, fmt, g, dim, ring, nbytes))
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for name, shape, dt, fmt, g, dim, ring, nbytes in rows:
            print(f"{name} {list(shape)} {dt} {fmt} g {g} dim {dim}: ring of {ring} inputs ({ring * nbytes / 2**20:.0f} MiB); cols, transpose, "
                  f"lastdim; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    ops = d.ops
    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_dynamic_cols.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; cols = the op "
                 f"with dim and fused=True (one launch), transpose = the same with fused=False (movedim().contiguous() -> the last-dim "
                 f"kernel -> movedim().contiguous()), lastdim = the last-dim kernel per_group of the same size on the same tensor (the "
                 f"one-read one-write bound); GB/s = 2 x tensor bytes / cols time; class = ops.dynamic_cols_class of the row")
    lines.append("# not measured: f16 inputs, f32 inputs other than the g256 row, the symmetric scheme, E2M1, pow2_scale, per_token columns")

    def graph_of(fn, ring):
        for x in ring[:2]:
            fn(x)
        torch.cuda.synchronize()
        g, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            for x in ring:
                keep.append(fn(x))
        return g, keep

    def replay_ms(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    slower = []
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, shape, dt, fmt, g, dim, ring_n, nbytes in rows:
        dtype = torch.float32 if dt == "f32" else torch.bfloat16
        ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(dtype) for _ in range(ring_n)]
        op = ops.dynamic_float_qdq if fmt == E4M3 else ops.dynamic_fixed_qdq
        inner = 1
        for v in shape[len(shape) + dim + 1 if dim < 0 else dim + 1:]:
            inner *= v
        cls = ops.dynamic_cols_class(g, dtype, inner)
        fns = [("cols", lambda x: op(x, fmt, "per_group", g, fused=True, dim=dim)),
               ("transpose", lambda x: op(x, fmt, "per_group", g, fused=False, dim=dim)),
               ("lastdim", lambda x: op(x, fmt, "per_group", g, fused=True))]
        graphs = [(label,) + graph_of(fn, ring) for label, fn in fns]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / len(ring))
        m = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        line = f"{name} {list(shape)} {dt} {fmt} g {g} dim {dim} (class {cls}, ring {len(ring)}):"
        for label, _ in fns:
            t = times[label]
            line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}];"
        line += f" cols {2 * nbytes / m['cols'] / 1e3:.0f} GB/s; transpose / cols {m['transpose'] / m['cols']:.2f}x; cols / lastdim {m['cols'] / m['lastdim']:.2f}x"
        if m["cols"] >= m["transpose"]:
            line += " ** NOT FASTER THAN THE TRANSPOSING ROUTE **"
            slower.append((cls, name, g))
        print(line, flush=True)
        lines.append(line)
        del graphs, ring
        torch.cuda.empty_cache()
    lines.append("# every cols row is faster than its transposing route" if not slower else f"# NOT FASTER THAN THE TRANSPOSING ROUTE: {slower}")
    print(lines[-1], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
