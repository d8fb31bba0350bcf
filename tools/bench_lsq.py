"""The learned step size backward on the GPU: ops.lsq_backward in ONE pass (csrc/lsq.hip) beside the chain of torch operations that
spells the same definition, on the same buffers.  Writes profiles/r19_lsq.txt (first line: tools/stamp.py --header).

Byte counts only say which way it should go: the kernel reads x and g once and writes dx once (6 B per bf16 element); the chain makes
about ten elementwise passes and two reductions over float32 temporaries of the tensor's size.  What decides the default route is
this table: a launch geometry (ops.lsq_class) goes to the kernel by default only where it is FASTER than the chain here; a row where
it is not is marked, the exit status is 1, and the class belongs in ops.LSQ_CHAIN_BY_DEFAULT.

Method (tools/bench_dynamic_quant.py's): each side's calls over a ring of (x, g) pairs larger than the 256 MiB last-level cache are
captured into ONE graph per side (every call keeps its own outputs), so that a replay is back-to-back kernels without the host in
between; the two graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of
(replay time / calls) and the spread.  % of 8 TB/s: the 6 B per element a one-pass backward must move, over the median.

    python tools/bench_lsq.py                  # the full table, written to profiles/
    python tools/bench_lsq.py --dry-run        # no GPU: the plan, nothing timed or written
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


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="8192x4096,8192x14336,2048x768,60000x48", help="comma-separated ROWSxCOLS (bf16); a shape whose COLS are no multiple of the group size is not measured per group (60000x48: rows of 6 vectors, the short_row geometry)")
    ap.add_argument("--group", type=int, default=128, help="the per_group size")
    ap.add_argument("--replays", type=int, default=11, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_lsq.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    a.shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",") if s]
    for s in a.shapes:
        if len(s) != 2 or min(s) < 1 or s[1] % 8:
            ap.error(f"shape {s}: ROWSxCOLS with COLS a multiple of 8")
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def plan(args):
    """[(shape, granularity, group size, ring)] -- shared by the dry run and the timed run"""
    rows = []
    for shape in args.shapes:
        nbytes = shape[0] * shape[1] * 2 * 2   # x and g
        ring = min(32, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache (at most 32 pairs)
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
            print(f"{FORMAT} {granularity}{'' if g is None else ' ' + str(g)} {list(shape)} bf16: ring of {ring} (x, g) pairs "
                  f"({ring * shape[0] * shape[1] * 4 / 2**20:.0f} MiB) per graph; fused and chain; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_lsq.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the two graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; "
                 f"% = 6 B per bf16 element / median / 8 TB/s; fused = ops.lsq_backward(fused=True) (one launch; per_tensor: two), chain = "
                 f"the same with fused=False (the definition in torch operations on float32 temporaries); affine zero points, want_dz; "
                 f"class = ops.lsq_class of the row.  Not measured: f16 / f32, other group sizes, training end to end")

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
            ring = [((torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16),
                     torch.randn(shape, generator=gen, device=dev).to(torch.bfloat16)) for _ in range(ring_n)]
            ring_shape = shape
        S = {"per_group": g, "per_token": shape[1], "per_tensor": shape[0] * shape[1]}[granularity]
        n_seg = shape[0] * shape[1] // S
        s = (torch.rand(n_seg, generator=gen, device=dev) + 0.5) * (1.4 / 7)   # (a good share of the elements is clipped)
        z = torch.randint(-3, 4, (n_seg,), generator=gen, device=dev).float()
        cls = d.ops.lsq_class(S, torch.bfloat16, granularity)
        sides = [("fused", lambda x, gr: d.ops.lsq_backward(x, gr, s, z, fmt, granularity, g, grad_factor=0.01, fused=True)),
                 ("chain", lambda x, gr: d.ops.lsq_backward(x, gr, s, z, fmt, granularity, g, grad_factor=0.01, fused=False))]
        graphs = [(label,) + graph_of(fn, ring) for label, fn in sides]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / len(ring))
        nbytes = 6 * shape[0] * shape[1]
        m = {k: med(v) for k, v in times.items()}
        line = f"{FORMAT} {granularity}{'' if g is None else ' ' + str(g)} {list(shape)} bf16 (class {cls}):"
        for label in ("fused", "chain"):
            t = times[label]
            line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}], {100.0 * nbytes / (m[label] * 1e-6) / PEAK:.0f} %;"
        line += f" chain / fused {m['chain'] / m['fused']:.2f}x"
        if m["fused"] >= m["chain"]:
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((cls, granularity, shape))
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
