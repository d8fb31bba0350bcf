"""AWQ weight clipping on the GPU: ops.awq_clip in ONE launch (csrc/awq_clip.hip) beside the pinned chain of torch operations that
defines it (fused=False) and beside a plain torch.bmm form of the same search, all on the same buffers.  Writes
profiles/r23_awq_clip.txt (first line: tools/stamp.py --header).

What decides the default route is this table: a group size goes to the kernel by default only where it is FASTER than the pinned chain
here; a row where it is not is marked, the exit status is 1, and the group size belongs in ops.AWQ_CLIP_CHAIN_BY_DEFAULT.  The bmm form
lives in this tool only: its sums are whatever order the GEMM takes, so it is an honest speed comparator and no parity partner; its
ratio to the kernel is recorded as measured, not asserted.

Method (tools/bench_hqq.py's): each side's calls over a ring of input tensors are captured into ONE graph per side (every call keeps
its own output), so that a replay is back-to-back kernels without the host in between; the graphs of a row are replayed in turn, device
events around every replay; per side the median over the replays of (replay time / calls) and the spread.  The kernel's ring is larger
than the 256 MiB last-level cache; the chain and the bmm form make hundreds to thousands of passes over float32 temporaries per call,
so their rings are two inputs (--slow-ring) -- the cache state of the input does not show in them.

    python tools/bench_awq_clip.py                  # the full table, written to profiles/
    python tools/bench_awq_clip.py --dry-run        # no GPU: the plan, nothing timed or written
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
SIDES = ("fused", "chain", "bmm")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default=ROWS, help="comma-separated ROWSxCOLS:GROUP (bf16)")
    ap.add_argument("--format", default="XP[4,0](C_N)", help="the integer format (the default is affine)")
    ap.add_argument("--n-grid", type=int, default=20)
    ap.add_argument("--max-shrink", type=float, default=0.5)
    ap.add_argument("--replays", type=int, default=5, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=1, help="untimed replays per side")
    ap.add_argument("--max-ring", type=int, default=160, help="the most inputs of the kernel's ring")
    ap.add_argument("--slow-ring", type=int, default=2, help="the inputs of the chain's and the bmm form's rings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_awq_clip.txt"), help="where the table is written")
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
    if a.replays < 3 or a.warmup < 1 or a.slow_ring < 1:
        ap.error("at least 3 timed replays, 1 warm-up replay and 1 input per ring")
    return a


def plan(args):
    """[(shape, group size, the kernel's ring)] -- shared by the dry run and the timed run"""
    out = []
    for shape, g in args.rows:
        nbytes = shape[0] * shape[1] * 2
        out.append((shape, g, min(args.max_ring, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))))
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, g, ring in rows:
            print(f"{args.format} g {g} {list(shape)} bf16: the kernel over a ring of {ring} inputs ({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB), "
                  f"the chain and the bmm form over {args.slow_ring}; {', '.join(SIDES)}; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    ops = d.ops
    dev = torch.device("cuda:0")
    fmt = args.format
    ratios = ops.awq_clip_ratios(args.n_grid, args.max_shrink)
    n = ratios.numel()
    r_dev = ratios.to(dev)
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_awq_clip.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; fused = "
                 f"ops.awq_clip(fused=True) (one launch; y only) over a ring of at most {args.max_ring} inputs, chain = the same with fused=False "
                 f"(the definition in torch operations: the sum over l in index order, the slicing tree) and bmm = the same search with "
                 f"torch.bmm for d B and torch.sum (sums not pinned: a speed comparator, no parity partner), both over rings of "
                 f"{args.slow_ring}; format {fmt}, {n} ratios (n_grid {args.n_grid}, max_shrink {args.max_shrink}); blocks of a random "
                 f"second moment; MAC = rows x L x g x {n} multiply-adds of the quadratic forms")

    def bmm_form(w, blocks, g):
        """the same search, its quadratic form through torch.bmm: any summation order"""
        rows_, L = w.shape
        G = L // g
        W = w.float().reshape(rows_, G, g)
        a = W.abs().amax(dim=-1, keepdim=True)
        y, best_loss = w.reshape(rows_, G, g), torch.full_like(a, float("inf"))
        Bt = blocks.transpose(1, 2)
        for i in range(n):
            c = (a * r_dev[i]).to(w.dtype).float()
            v = torch.where(W > c, c, torch.where(W < -c, -c, W)).to(w.dtype)
            dq = ops.dynamic_fixed_qdq(v.reshape(rows_, L), fmt, "per_group", g).float().reshape(rows_, G, g) - W
            t = torch.bmm(dq.transpose(0, 1), Bt).transpose(0, 1)
            loss = (dq * t).sum(-1, keepdim=True)
            better = torch.isfinite(loss) & (loss < best_loss)
            best_loss = torch.where(better, loss, best_loss)
            y = torch.where(better, v, y)
        return y.reshape(rows_, L)

    def graph_of(fn, ring):
        fn(ring[0])                     # eager warm-up: code objects, allocator
        torch.cuda.synchronize()
        g, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            for x in ring:
                keep.append(fn(x))      # (every call's output stays alive)
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
            ring = [(torch.randn(shape, generator=gen, device=dev) * 0.05).to(torch.bfloat16) for _ in range(ring_n)]
            ring_shape = shape
        L = shape[1]
        x = torch.randn(512, L, generator=gen, device=dev) * (1.0 + 3.0 * torch.rand(L, generator=gen, device=dev))
        xg = x.reshape(512, L // g, g).transpose(0, 1)
        blocks = (xg.transpose(1, 2) @ xg / 512).contiguous()
        sides = [("fused", lambda w: ops.awq_clip(w, blocks, fmt, g, ratios, fused=True), ring),
                 ("chain", lambda w: ops.awq_clip(w, blocks, fmt, g, ratios, fused=False), ring[:args.slow_ring]),
                 ("bmm", lambda w: bmm_form(w, blocks, g), ring[:args.slow_ring])]
        graphs = [(label, len(r_)) + graph_of(fn, r_) for label, fn, r_ in sides]
        for _ in range(args.warmup):
            for _, _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _, _ in graphs}
        for _ in range(args.replays):
            for label, calls, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / calls)
        m = {k: med(v) for k, v in times.items()}
        macs = shape[0] * L * g * n
        line = f"{fmt} g {g} {list(shape)} bf16 (ring {len(ring)}):"
        for label in SIDES:
            t = times[label]
            line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}];"
        line += (f" chain / fused {m['chain'] / m['fused']:.1f}x, bmm / fused {m['bmm'] / m['fused']:.2f}x, "
                 f"fused {macs / m['fused'] / 1e6:.2f} T multiply-adds per second")
        if m["fused"] >= m["chain"]:
            line += " ** NOT FASTER THAN THE CHAIN **"
            slower.append((g, shape))
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
