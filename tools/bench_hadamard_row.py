"""The full-row Hadamard rotation on the GPU: ops.hadamard_row and ops.hadamard_row_dynamic_qdq in ONE launch (csrc/hadamard_row.hip)
beside (a) the same-bits chain of torch operations (fused=False), (b) what users do today -- x @ H as a bf16 torch.matmul with a
resident dense [n, n] matrix (the rotation alone: the cast would come on top) -- and (c) the plain ops.dynamic_fixed_qdq, all on the
same buffers.  Writes profiles/r26_hadamard_row.txt (first line: tools/stamp.py --header).

What decides the default route is this table: a class (ops.hadamard_row_class) goes to the kernel by default only where it is FASTER
than its chain here; a row where it is not is marked, the exit status is 1, and the class belongs in ops.HADAMARD_ROW_CHAIN_BY_DEFAULT.

Method (tools/bench_vq.py's): the fused, matmul and plain-cast calls over a ring of input tensors larger than the 256 MiB last-level
cache are captured into ONE graph per side (every call keeps its own output) and the graphs of a row replayed in turn, device events
around every replay; per side the median over the replays of (replay time / calls).  The chain takes hundreds of torch launches and
milliseconds per call: it is timed eagerly on the ring's first input, device events around the call.

    python tools/bench_hadamard_row.py                  # the full table, written to profiles/
    python tools/bench_hadamard_row.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
SHAPES = "8192x4096,8192x14336,8192x5120,2048x768"
INT4 = "XP[4,0](CSN)"
# (label, granularity, group size, inverse); granularity None: the rotation alone
VARIANTS = [("rotate", None, None, False), ("int4 per_token inverse", "per_token", None, True), ("int4 per_token", "per_token", None, False),
            ("int4 per_group 128 inverse", "per_group", 128, True), ("int4 per_group 128", "per_group", 128, False)]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated ROWSxCOLS (bf16)")
    ap.add_argument("--replays", type=int, default=7, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--chain-reps", type=int, default=3, help="timed eager calls of the chain")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_hadamard_row.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    a.shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",") if s]
    if a.replays < 3 or a.warmup < 1 or a.chain_reps < 1:
        ap.error("at least 3 timed replays, 1 warm-up replay and 1 chain call")
    return a


def plan(args):
    """[(shape, ring, label, granularity, group size, inverse)] -- shared by the dry run and the timed run; a group that does not divide
    the row's 2^k is not a case of the op and is left out"""
    out = []
    for shape in args.shapes:
        n = shape[1]
        odd = n
        while odd % 2 == 0:
            odd //= 2
        P = n // (1 if odd == 1 else 4 * odd)
        ring = min(160, max(2, -(-(LLC_BYTES * 3 // 2) // (shape[0] * n * 2))))
        for label, gran, g, inv in VARIANTS:
            if g is None or P % g == 0:
                out.append((shape, ring, label, gran, g, inv))
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, ring, label, _, _, _ in rows:
            print(f"{label} {list(shape)} bf16: ring of {ring} inputs ({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB); fused, "
                  f"matmul (rotate only), plain cast, chain; {args.warmup} + {args.replays} replays, {args.chain_reps} chain calls")
        return 0

    import torch
    import dmx_compressor_amd as dmx

    ops = dmx.ops
    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_hadamard_row.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; bf16; us per call; fused / matmul / plain = graph replay time / calls in the graph over a "
                 f"ring of inputs, median of {args.replays} replays [min .. max] after {args.warmup} warm-up replays, the graphs of a row "
                 f"replayed in turn; chain = the same call with fused=False, eager, median of {args.chain_reps} calls on the ring's first "
                 f"input; device events; fused = ops.hadamard_row / ops.hadamard_row_dynamic_qdq(fused=True), ONE launch; matmul = x @ H, "
                 f"a bf16 torch.matmul with the resident dense [n, n] matrix (the rotation ALONE, whatever the row's cast); plain = "
                 f"ops.dynamic_fixed_qdq of the unrotated tensor (the cast ALONE); % of 8 TB/s = 4 B per element / fused time; class = "
                 f"ops.hadamard_row_class of the row")

    def graph_of(fn, ring):
        for x in ring[:2]:
            fn(x)
        torch.cuda.synchronize()
        g, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            for x in ring:
                keep.append(fn(x))
        return g, keep, len(ring)

    def timed_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def med(v):
        return sorted(v)[len(v) // 2]

    slower = []
    gen = torch.Generator(device=dev).manual_seed(0)
    cur, ring, H = None, None, None
    for shape, ring_n, label, gran, g, inv in rows:
        n = shape[1]
        if shape != cur:
            ring = H = None
            torch.cuda.empty_cache()
            ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(ring_n)]
            H = ops.hadamard_row(torch.eye(n, device=dev), transpose=True).to(torch.bfloat16)   # row i = R^T e_i: x @ H = R(x)
            cur = shape
        cls = ops.hadamard_row_class(n, torch.bfloat16, g)
        if gran is None:
            sides = [("fused", lambda x: ops.hadamard_row(x, fused=True)), ("matmul", lambda x: torch.matmul(x, H))]
            chain = lambda: ops.hadamard_row(ring[0], fused=False)   # noqa: E731
        else:
            sides = [("fused", lambda x: ops.hadamard_row_dynamic_qdq(x, INT4, gran, g, inverse=inv, fused=True)),
                     ("plain", lambda x: ops.dynamic_fixed_qdq(x, INT4, gran, g))]
            chain = lambda: ops.hadamard_row_dynamic_qdq(ring[0], INT4, gran, g, inverse=inv, fused=False)   # noqa: E731
        graphs = [(name,) + graph_of(fn, ring) for name, fn in sides]
        for _ in range(args.warmup):
            for _, gr, _, _ in graphs:
                timed_ms(gr.replay)
        times = {name: [] for name, _, _, _ in graphs}
        for _ in range(args.replays):
            for name, gr, _, calls in graphs:
                times[name].append(1000.0 * timed_ms(gr.replay) / calls)
        chain()
        times["chain"] = [1000.0 * timed_ms(chain) for _ in range(args.chain_reps)]
        m = {k: med(v) for k, v in times.items()}
        line = f"{label} {list(shape)} (class {cls}):"
        for name, t in times.items():
            line += f" {name} {m[name]:.1f} us [{min(t):.1f} .. {max(t):.1f}]"
            line += f", {100.0 * 4 * shape[0] * n / (m[name] * 1e-6) / 8e12:.0f} % of 8 TB/s;" if name == "fused" else ";"
        line += f" chain / fused {m['chain'] / m['fused']:.1f}x"
        if m["fused"] >= m["chain"]:
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((cls, label, shape))
        print(line, flush=True)
        lines.append(line)
        del graphs
        torch.cuda.empty_cache()
    lines.append("# every fused row is faster than its chain" if not slower else f"# NOT FASTER THAN THE CHAIN: {slower}")
    lines.append("# not measured: f16 / f32, group sizes other than 128, INT8, transpose=True; per_group 128 on [2048, 768] is no case "
                 "(768 = 12 * 64: 128 does not divide 2^k)")
    print(lines[-2], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
