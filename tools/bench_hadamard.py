"""The fused rotated cast on the GPU: ops.hadamard_qdq (rotate -> quantize -> rotate back in ONE launch, csrc/hadamard.hip) beside the
library's PLAIN cast of the same format on the same buffers -- the yardstick: the plain casts are what they were before the rotation
existed.  Writes profiles/r11_hadamard.txt (first line: tools/stamp.py --header).

The one condition that follows from byte counts: the fused call moves 4 B per bf16 element (one read, one write), the three-launch
chain it replaces (rotation to float32, cast in float32, rotation back) 20 B, so the fused call has to come in under 5 x the plain
cast's time; a row that does not is marked and the exit status is 1.

Method: each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are captured into ONE graph per side
(every call keeps its own output: the outputs rotate with the inputs), so that a replay is back-to-back kernels without the host in
between; the graphs of one (shape, format) -- the plain cast and the fused call at every rotation size -- are replayed in turn, device
events around every replay; per side the median over the replays of (replay time / calls), and the spread (min .. max).  GB/s: the
4 B per element the call must move over the median.

    python tools/bench_hadamard.py                  # the full table, written to profiles/
    python tools/bench_hadamard.py --dry-run        # no GPU: the plan (shapes, formats, sizes, ring sizes), nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
FORMATS = ["BFP[8|8]{16}(SN)", "MXFP4[E2M1]{32}", "XP[8,0](CSN)"]   # XP: per tensor, one scale
XP_SCALE = 0.02
LIMIT = 5.0   # fused / plain: 20 B per element for the chain over 4 B for the fused call


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="4096x4096,14336x4096", help="comma-separated ROWSxCOLS (bf16)")
    ap.add_argument("--sizes", default="32,64,128", help="rotation sizes")
    ap.add_argument("--replays", type=int, default=15, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=3, help="untimed replays per side")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write profiles/r11_hadamard.txt")
    a = ap.parse_args(argv)
    a.shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",") if s]
    a.sizes = [int(v) for v in a.sizes.split(",") if v]
    for s in a.shapes:
        if len(s) != 2 or min(s) < 1 or s[1] % 256:
            ap.error(f"shape {s}: ROWSxCOLS with COLS a multiple of 256 (the largest rotation size)")
    for h in a.sizes:
        if h not in (32, 64, 128, 256):
            ap.error(f"size {h}: one of 32, 64, 128, 256 (every format's block divides it)")
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def plan(args):
    """[(shape, format, ring, bytes moved per call)] -- shared by the dry run and the timed run"""
    rows = []
    for shape in args.shapes:
        nbytes = shape[0] * shape[1] * 2
        ring = min(64, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache (at most 64 inputs)
        for fmt in FORMATS:
            rows.append((shape, fmt, ring, 2 * nbytes))
    return rows


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for shape, fmt, ring, nbytes in rows:
            print(f"{fmt} {list(shape)} bf16: ring of {ring} inputs ({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB) and as many outputs per graph, "
                  f"{nbytes / 2**20:.0f} MiB moved per call; plain cast and fused at H = {args.sizes}; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_hadamard.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; GB/s = 4 B per "
                 f"bf16 element / median; fused = ops.hadamard_qdq(x, H, format, fused=True) (rotate, cast, rotate back: one launch), plain = "
                 f"the library's cast of the same format; the fused call must stay under {LIMIT:.0f} x plain (20 B per element for the "
                 f"three-launch chain over 4 B)")

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

    over = []
    gen = torch.Generator(device=dev).manual_seed(0)
    ring_shape, ring = None, None
    scale = torch.full((1,), XP_SCALE, dtype=torch.float32, device=dev)
    zp = torch.zeros(1, dtype=torch.int64, device=dev)
    for shape, name, ring_n, nbytes in rows:
        if shape != ring_shape:
            ring = None
            ring = [(torch.randn(shape, generator=gen, device=dev) * 0.7).to(torch.bfloat16) for _ in range(ring_n)]
            ring_shape = shape
        fmt = d.Format.from_shorthand(name)
        fixed = isinstance(fmt, d.FixedPoint)
        kw = {"scale": scale, "zero_point": zp} if fixed else {}
        if fixed:
            def plain(x):
                return d.ops.fixed_qdq(x, fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=scale, zero_point=zp)
        else:
            def plain(x):
                return fmt.cast(x, -1, out_dtype=x.dtype)
        sides = [("plain", plain)] + [(f"H={h}", (lambda x, h=h: d.ops.hadamard_qdq(x, h, fmt, fused=True, **kw))) for h in args.sizes]
        graphs = [(label,) + graph_of(fn, ring) for label, fn in sides]
        for _ in range(args.warmup):
            for _, g, _ in graphs:
                replay_ms(g)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, g, _ in graphs:
                times[label].append(1000.0 * replay_ms(g) / len(ring))
        mp = med(times["plain"])
        line = f"{name} {list(shape)} bf16: plain {mp:.1f} us [{min(times['plain']):.1f} .. {max(times['plain']):.1f}], {nbytes / (mp * 1e-6) / 1e9:.0f} GB/s"
        for label, _, _ in graphs[1:]:
            t = times[label]
            m = med(t)
            line += f"; fused {label} {m:.1f} us [{min(t):.1f} .. {max(t):.1f}], {nbytes / (m * 1e-6) / 1e9:.0f} GB/s, {m / mp:.2f}x plain"
            if m >= LIMIT * mp:
                line += " ** OVER THE LIMIT **"
                over.append((name, shape, label))
        print(line, flush=True)
        lines.append(line)
        del graphs
    lines.append("# every fused call under the limit" if not over else f"# OVER THE LIMIT of {LIMIT:.0f} x plain: {over}")
    print(lines[-1], flush=True)
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r11_hadamard.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if over else 0


if __name__ == "__main__":
    sys.exit(main())
