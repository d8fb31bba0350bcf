"""The error probe on the GPU: ops.cast_error (one read of the tensor for K formats, csrc/error_stats.hip) against the unfused composition
it replaces -- K library casts, each followed by torch's mse_loss(x.float(), y.float()) and (x - y).float().abs().max() --, and
ops.error_stats against the same two torch reductions on a given pair.  Writes profiles/r10_error_probe.txt (first line:
tools/stamp.py --header).

Method: each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are captured into ONE graph per side, so
that a replay is back-to-back kernels without the host in between (neither side reads anything back: the reference's .item() calls are
left out, in its favour); the two graphs are replayed alternately, device events around every replay; per side the median over the
replays of (replay time / calls), and the spread (min .. max).  Bytes: what the algorithm must read (the tensor once for the fused
call; for error_stats both tensors); share: that rate over the read ceiling of profiles/r01_directional_ceilings.txt.

    python tools/bench_error_probe.py                  # the full table, written to profiles/
    python tools/bench_error_probe.py --dry-run        # no GPU: the plan (shapes, formats, ring sizes, bytes), nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_CEILING_GBS = 5385.8   # profiles/r01_directional_ceilings.txt: read 32 MiB (512x16)
LLC_BYTES = 256 << 20
# BFP16_16-class candidates: what a per-layer format choice compares
FORMATS = ["BFP[8|8]{16}(SN)", "BFP[8|8]{32}(SN)", "BFP[8|8]{64}(SN)", "BFP[8|8]{128}(SN)", "BFP[6|8]{16}(SN)", "BFP[6|8]{32}(SN)",
           "BFP[4|8]{16}(SN)", "BFP[4|8]{32}(SN)"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="4096x4096,14336x4096", help="comma-separated ROWSxCOLS (bf16)")
    ap.add_argument("--ks", default="1,4,8", help="numbers of formats per cast_error call")
    ap.add_argument("--replays", type=int, default=15, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=3, help="untimed replays per side")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write profiles/r10_error_probe.txt")
    a = ap.parse_args(argv)
    a.shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",") if s]
    a.ks = [int(k) for k in a.ks.split(",") if k]
    for s in a.shapes:
        if len(s) != 2 or min(s) < 1 or s[1] % 128:
            ap.error(f"shape {s}: ROWSxCOLS with COLS a multiple of 128 (the largest block size timed)")
    for k in a.ks:
        if not 1 <= k <= len(FORMATS):
            ap.error(f"K = {k}: between 1 and {len(FORMATS)}")
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def plan(args):
    """[(what, shape, K, ring, bytes read per call by the fused side)] -- shared by the dry run and the timed run"""
    rows = []
    for shape in args.shapes:
        nbytes = shape[0] * shape[1] * 2
        ring = min(64, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache (at most 64 inputs)
        for k in args.ks:
            rows.append(("cast_error", shape, k, ring, nbytes))
        rows.append(("error_stats", shape, 1, max(2, -(-ring // 2)), 2 * nbytes))
    return rows


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for what, shape, k, ring, nbytes in rows:
            print(f"{what} {list(shape)} bf16 K={k}: ring of {ring} inputs ({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB), {nbytes / 2**20:.0f} MiB read "
                  f"per fused call, {args.warmup} + {args.replays} replays per side; formats {FORMATS[:k] if what == 'cast_error' else '-'}")
        return 0

    import torch
    import dmx_compressor_amd as d

    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_error_probe.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], fused and unfused graphs replayed alternately after {args.warmup} warm-up replays each; device events; "
                 f"GB/s = bytes the algorithm reads / median; share of the {READ_CEILING_GBS} GB/s read ceiling "
                 f"(profiles/r01_directional_ceilings.txt)")

    def graph_of(fn, ring):
        for x in ring[:2]:
            fn(x)                       # eager warm-up: code objects, allocator
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for x in ring:
                fn(x)
        return g

    def replay_ms(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def race(g_fused, g_unfused, calls):
        for _ in range(args.warmup):
            replay_ms(g_fused), replay_ms(g_unfused)
        tf, tu = [], []
        for _ in range(args.replays):
            tf.append(1000.0 * replay_ms(g_fused) / calls)
            tu.append(1000.0 * replay_ms(g_unfused) / calls)
        med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
        return (med(tf), min(tf), max(tf)), (med(tu), min(tu), max(tu))

    slower = []
    gen = torch.Generator(device=dev).manual_seed(0)
    rings = {}
    for what, shape, k, ring_n, nbytes in rows:
        if shape not in rings:
            rings.clear()
            rings[shape] = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(max(r[3] for r in rows if r[1] == shape))]
        xs = rings[shape][:ring_n]
        if what == "cast_error":
            fmts = [d.Format.from_shorthand(f) for f in FORMATS[:k]]
            out = torch.zeros(k, 4, dtype=torch.float64, device=dev)
            keep = []

            def fused(x):
                d.ops.cast_error(x, fmts, out=out)

            def unfused(x):
                for f in fmts:
                    y = f.cast(x, -1, out_dtype=x.dtype)
                    keep[:] = [torch.nn.functional.mse_loss(x.float(), y.float()), (x - y).float().abs().max()]
        else:
            ys = {id(x): d.Format.from_shorthand(FORMATS[0]).cast(x, -1, out_dtype=x.dtype) for x in xs}
            out = torch.zeros(4, dtype=torch.float64, device=dev)
            keep = []

            def fused(x):
                d.ops.error_stats(x, ys[id(x)], out=out)

            def unfused(x):
                y = ys[id(x)]
                keep[:] = [torch.nn.functional.mse_loss(x.float(), y.float()), (x - y).float().abs().max()]
        gf, gu = graph_of(fused, xs), graph_of(unfused, xs)
        (mf, lf, hf), (mu, lu, hu) = race(gf, gu, len(xs))
        gbs = nbytes / (mf * 1e-6) / 1e9
        line = (f"{what} {list(shape)} bf16 K={k}: fused {mf:.1f} us [{lf:.1f} .. {hf:.1f}], {gbs:.0f} GB/s = {100 * gbs / READ_CEILING_GBS:.0f} % of the "
                f"read ceiling; unfused {mu:.1f} us [{lu:.1f} .. {hu:.1f}]; unfused / fused {mu / mf:.1f}x")
        if mf > mu:
            line += "  ** FUSED SLOWER **"
            slower.append(line)
        print(line, flush=True)
        lines.append(line)
        del gf, gu
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r10_error_probe.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
