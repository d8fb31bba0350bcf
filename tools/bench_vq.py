"""The vector codebook cast on the GPU: ops.vq_qdq in ONE launch (csrc/vq.hip) beside the chain of torch operations that defines it
(group_minmax -> the scale rule -> scale_channels -> per-component subtract / multiply / add into a [vectors, K] distance tensor ->
argmin with the NaN and +Inf overrides -> gather -> scale_channels), ops.vq_accumulate (one pass plus a fold launch) beside its torch
index_add_ form, and one whole ops.vq_fit iteration (statistics and the table update), all on the same buffers.  Writes
profiles/r25_vq.txt (first line: tools/stamp.py --header).

What decides the default route is this table: a launch geometry (ops.vq_class) goes to the kernel by default only where it is FASTER
than the chain here; a row where it is not is marked, the exit status is 1, and the class belongs in ops.VQ_CHAIN_BY_DEFAULT.

Method (tools/bench_codebook.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are
captured into ONE graph per side (every call keeps its own output), so that a replay is back-to-back kernels without the host in
between; the graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of
(replay time / calls) and the spread.  The two chain sides take milliseconds per call and far more memory traffic than the cache
holds, so their graphs hold the first --chain-calls inputs of the ring only.  The search is VALU-bound, not HBM-bound: beside the time
stands the rate of lane operations, K (3 d + 2) per d-vector (d subtracts, d multiplies, d - 1 adds, a compare and two selects).

    python tools/bench_vq.py                  # the full table, written to profiles/
    python tools/bench_vq.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
ROWS = "4096x4096:per_group,4096x4096:per_token,14336x4096:per_group,14336x4096:per_token,2048x768:per_group,2048x768:per_token"
TABLES = "2x16,2x256,4x256,8x256"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default=ROWS, help="comma-separated ROWSxCOLS:GRANULARITY (bf16)")
    ap.add_argument("--tables", default=TABLES, help="comma-separated DxK table shapes")
    ap.add_argument("--group", type=int, default=64, help="the per_group size")
    ap.add_argument("--replays", type=int, default=9, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--chain-calls", type=int, default=2, help="calls in a chain side's graph")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_vq.txt"), help="where the table is written")
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
    tables = []
    for t in a.tables.split(","):
        d, _, K = t.lower().partition("x")
        if not (d.isdigit() and K.isdigit() and int(d) in (2, 4, 8) and 2 <= int(K) <= 256):
            ap.error(f"table {t}: DxK with D in 2, 4, 8 and K from 2 to 256")
        tables.append((int(d), int(K)))
    a.tables = tables
    if a.replays < 3 or a.warmup < 1 or a.chain_calls < 1:
        ap.error("at least 3 timed replays, 1 warm-up replay and 1 chain call")
    return a


def plan(args):
    """[(shape, granularity, group size, ring, d, K)] -- shared by the dry run and the timed run"""
    out = []
    for shape, gran in args.rows:
        nbytes = shape[0] * shape[1] * 2
        ring = min(160, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache (at most 160 inputs)
        for d, K in args.tables:
            out.append((shape, gran, None if gran == "per_token" else args.group, ring, d, K))
    return out


SIDES = ("fused", "chain", "acc", "acc_chain", "fit_iter")


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, gran, g, ring, d, K in rows:
            print(f"[{K}, {d}] {gran}{'' if g is None else ' ' + str(g)} {list(shape)} bf16: ring of {ring} inputs "
                  f"({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB) and as many outputs per graph, {min(ring, args.chain_calls)} for the "
                  f"chain sides; {', '.join(SIDES)}; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as dmx

    ops = dmx.ops
    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_vq.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; Glop/s = "
                 f"K (3 d + 2) lane operations per d-vector / median; fused = ops.vq_qdq(fused=True) (one launch), chain = the same with "
                 f"fused=False (group_minmax, the scale rule in torch, scale_channels, per-component distances, argmin, gather, "
                 f"scale_channels; on pieces of at most {ops.VQ_CHAIN_PIECE_ENTRIES} distance entries), acc = ops.vq_accumulate (fused=True: "
                 f"one pass and a fold launch), acc_chain = the same with fused=False (the chain's scale, quotient and index, then torch "
                 f"index_add_), fit_iter = ops.vq_fit(iters=1, fused=True): the statistics and the table update; the fused sides over the "
                 f"whole ring, chain and acc_chain over its first {args.chain_calls} inputs; tables: normal rows (seed 0); class = "
                 f"ops.vq_class of the row")

    def graph_of(fn, ring):
        for x in ring[:2]:
            fn(x)                       # eager warm-up: code objects, allocator
        torch.cuda.synchronize()
        g, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            for x in ring:
                keep.append(fn(x))      # (every call's output stays alive: as many output buffers as inputs)
        return g, keep, len(ring)

    def replay_ms(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def med(v):
        return sorted(v)[len(v) // 2]

    slower, seen = [], set()
    gen = torch.Generator(device=dev).manual_seed(0)
    ring_shape, ring = None, None
    for shape, gran, g, ring_n, d, K in rows:
        if shape != ring_shape:
            ring = None
            ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(ring_n)]
            ring_shape = shape
        table = torch.randn((K, d), generator=gen, device=dev)
        cls = ops.vq_class(shape[1] if g is None else g, torch.bfloat16, d, K, g is None)
        seen.add(cls)
        short = ring[:args.chain_calls]
        sides = [("fused", lambda x: ops.vq_qdq(x, table, gran, g, fused=True), ring),
                 ("chain", lambda x: ops.vq_qdq(x, table, gran, g, fused=False), short),
                 ("acc", lambda x: ops.vq_accumulate(x, table, gran, g, fused=True), ring),
                 ("acc_chain", lambda x: ops.vq_accumulate(x, table, gran, g, fused=False), short),
                 ("fit_iter", lambda x: ops.vq_fit(x, codebook=table, granularity=gran, group_size=g, norm=1.0, iters=1, fused=True)[0], ring)]
        graphs = [(label,) + graph_of(fn, r) for label, fn, r in sides]
        for _ in range(args.warmup):
            for _, gr, _, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _, calls in graphs:
                times[label].append(1000.0 * replay_ms(gr) / calls)
        n = shape[0] * shape[1]
        lane_ops = K * (3 * d + 2) * (n // d)
        m = {k: med(v) for k, v in times.items()}
        line = f"[{K}, {d}] {gran}{'' if g is None else ' ' + str(g)} {list(shape)} bf16 (class {cls}):"
        for label in SIDES:
            t = times[label]
            line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}]"
            line += f", {lane_ops / (m[label] * 1e-6) / 1e9:.0f} Glop/s;" if label == "fused" else ";"
        line += f" chain / fused {m['chain'] / m['fused']:.2f}x, acc_chain / acc {m['acc_chain'] / m['acc']:.2f}x"
        if m["fused"] >= m["chain"]:
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((cls, gran, shape, d, K))
        print(line, flush=True)
        lines.append(line)
        del graphs
        torch.cuda.empty_cache()
    lines.append("# every fused row is faster than its chain" if not slower else f"# NOT FASTER THAN THE CHAIN: {slower}")
    missing = sorted({"group", "short_row", "wave_row", "block_row"} - seen)
    lines.append("# not measured: f16 / f32, group sizes other than the one above, K between the listed ones"
                 + (f"; classes {', '.join(missing)}" if missing else ""))
    print(lines[-2], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
