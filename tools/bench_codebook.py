"""The codebook cast on the GPU: ops.codebook_qdq in ONE launch (csrc/codebook.hip) beside the chain of launches that defines it
(group_minmax -> the scale rule -> scale_channels -> torch.bucketize -> gather -> scale_channels) and beside ops.dynamic_float_qdq
E2M1 of the same segment (the 4-bit float cast under the same kind of scale), and ops.codebook_accumulate (one pass plus a fold
launch) beside its torch index_add_ form, all on the same buffers.  Writes profiles/r20_codebook.txt (first line: tools/stamp.py
--header).

What decides the default route is this table: a launch geometry (ops.codebook_class) goes to the kernel by default only where it is
FASTER than the chain here; a row where it is not is marked, the exit status is 1, and the class belongs in
ops.CODEBOOK_CHAIN_BY_DEFAULT.  The ratio to the E2M1 kernel is recorded, not asserted.

Method (tools/bench_dynamic_float.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are
captured into ONE graph per side (every call keeps its own output), so that a replay is back-to-back kernels without the host in
between; the graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of
(replay time / calls) and the spread.  % of 8 TB/s: the bytes a one-pass form must move (the cast: 4 B per bf16 element; the
statistics: 2 B), over the median.

    python tools/bench_codebook.py                  # the full table, written to profiles/
    python tools/bench_codebook.py --dry-run        # no GPU: the plan, nothing timed or written
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
E2M1 = "FP[1|2|1,1](_N)"
ROWS = "8192x4096:per_group,8192x4096:per_token,8192x14336:per_group,8192x14336:per_token,2048x768:per_group,2048x768:per_token"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default=ROWS, help="comma-separated ROWSxCOLS:GRANULARITY (bf16)")
    ap.add_argument("--codebook", default="nf4", help="a name of ops.CODEBOOKS")
    ap.add_argument("--group", type=int, default=64, help="the per_group size")
    ap.add_argument("--replays", type=int, default=15, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=3, help="untimed replays per side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_codebook.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    rows = []
    for r in a.rows.split(","):
        if not r:
            continue
        shape, _, gran = r.partition(":")
        shape = tuple(int(v) for v in shape.lower().split("x"))
        if len(shape) != 2 or min(shape) < 1 or shape[1] % 8 or gran not in ("per_token", "per_group"):
            ap.error(f"row {r}: ROWSxCOLS:per_token|per_group with COLS a multiple of 8")
        if gran == "per_group" and shape[1] % a.group:
            ap.error(f"row {r}: the group size {a.group} does not divide the shape")
        rows.append((shape, gran))
    a.rows = rows
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def plan(args):
    """[(shape, granularity, group size, ring)] -- shared by the dry run and the timed run"""
    out = []
    for shape, gran in args.rows:
        nbytes = shape[0] * shape[1] * 2
        ring = min(160, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache (at most 160 inputs)
        out.append((shape, gran, None if gran == "per_token" else args.group, ring))
    return out


SIDES = ("fused", "chain", "e2m1", "acc", "acc_chain")


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, gran, g, ring in rows:
            print(f"{args.codebook} {gran}{'' if g is None else ' ' + str(g)} {list(shape)} bf16: ring of {ring} inputs "
                  f"({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB) and as many outputs per graph; {', '.join(SIDES)}; "
                  f"{args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    ops = d.ops
    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_codebook.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; "
                 f"% = bytes a one-pass form moves (cast: 4 B per bf16 element, statistics: 2 B) / median / 8 TB/s; fused = "
                 f"ops.codebook_qdq(fused=True) (one launch), chain = the same with fused=False (group_minmax, the scale rule in torch, "
                 f"scale_channels, torch.bucketize, gather, scale_channels; on more than 65535 segments on pieces of 32768 segments joined "
                 f"with torch.cat), e2m1 = ops.dynamic_float_qdq {E2M1} of the same segments (one launch), acc = ops.codebook_accumulate "
                 f"(fused=True: one pass and a fold launch), acc_chain = the same with fused=False (the chain's scale, quotient and index, "
                 f"then torch index_add_); table {args.codebook!r}; class = ops.codebook_class of the row")

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
    table = torch.tensor(ops.CODEBOOKS[args.codebook], dtype=torch.float32, device=dev)
    e2m1 = d.Format.from_shorthand(E2M1)
    for shape, gran, g, ring_n in rows:
        if shape != ring_shape:
            ring = None
            ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(ring_n)]
            ring_shape = shape
        cls = ops.codebook_class(shape[1] if g is None else g, torch.bfloat16, g is None)
        sides = [("fused", lambda x: ops.codebook_qdq(x, table, gran, g, fused=True)),
                 ("chain", lambda x: ops.codebook_qdq(x, table, gran, g, fused=False)),
                 ("e2m1", lambda x: ops.dynamic_float_qdq(x, e2m1, gran, g, fused=True)),
                 ("acc", lambda x: ops.codebook_accumulate(x, table, gran, g, fused=True)),
                 ("acc_chain", lambda x: ops.codebook_accumulate(x, table, gran, g, fused=False))]
        graphs = [(label,) + graph_of(fn, ring) for label, fn in sides]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / len(ring))
        n = shape[0] * shape[1]
        m = {k: med(v) for k, v in times.items()}
        line = f"{args.codebook} {gran}{'' if g is None else ' ' + str(g)} {list(shape)} bf16 (class {cls}):"
        for label in SIDES:
            t = times[label]
            nbytes = (2 if label.startswith("acc") else 4) * n
            line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}], {100.0 * nbytes / (m[label] * 1e-6) / PEAK:.0f} %;"
        line += (f" chain / fused {m['chain'] / m['fused']:.2f}x, fused / e2m1 {m['fused'] / m['e2m1']:.2f}x, "
                 f"acc_chain / acc {m['acc_chain'] / m['acc']:.2f}x")
        if m["fused"] >= m["chain"]:
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((cls, gran, shape))
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
