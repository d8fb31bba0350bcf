"""The outlier-aware dynamic cast on the GPU: ops.outlier_fixed_qdq in ONE launch (csrc/outlier_quant.hip) at k = 1, 2, 4 beside the chain
of torch operations and library calls that defines it (fused=False), and beside ops.dynamic_fixed_qdq per group of the same size -- the
k = 0 floor -- all on the same buffers.  Writes profiles/r22_outlier.txt (first line: tools/stamp.py --header), with the kernel's VGPR
counts from the build's resource remarks.

What decides the default route is this table: the class (ops.outlier_class) goes to the kernel by default only where it is FASTER than
the chain here; a row where it is not is marked, the exit status is 1, and the class belongs in ops.OUTLIER_CHAIN_BY_DEFAULT.  The
kernel's time against the k = 0 dynamic kernel, as us per added outlier (fused_k - dynamic) / k -- the price of a selection round -- is
recorded, not asserted.

Method (tools/bench_hqq.py's): each side's calls over a ring of input tensors larger than the 256 MiB last-level cache are captured
into ONE graph per side (every call keeps its own output), so that a replay is back-to-back kernels without the host in between; the
graphs of a row are replayed in turn, device events around every replay; per side the median over the replays of (replay time / calls)
and the spread.

    python tools/bench_outlier.py                  # the full table, written to profiles/
    python tools/bench_outlier.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
ROWS = "4096x4096:64,4096x4096:128,14336x4096:64,14336x4096:128,2048x768:64,2048x768:128"
KS = "1,2,4"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default=ROWS, help="comma-separated ROWSxCOLS:GROUP (bf16)")
    ap.add_argument("--ks", default=KS, help="comma-separated outlier counts per group")
    ap.add_argument("--format", default="XP[4,0](C_N)", help="the integer format (affine scheme)")
    ap.add_argument("--replays", type=int, default=9, help="timed replays per side")
    ap.add_argument("--warmup", type=int, default=2, help="untimed replays per side")
    ap.add_argument("--max-ring", type=int, default=160, help="the most inputs of a ring")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_outlier.txt"), help="where the table is written")
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
    a.ks = [int(v) for v in a.ks.split(",") if v]
    if not a.ks or min(a.ks) < 1 or any(k >= g for k in a.ks for _, g in rows):
        ap.error("outlier counts of at least 1 and below every group size")
    if a.replays < 3 or a.warmup < 1:
        ap.error("at least 3 timed replays and 1 warm-up replay")
    return a


def plan(args):
    """[(shape, group size, ring)] -- shared by the dry run and the timed run"""
    out = []
    for shape, g in args.rows:
        nbytes = shape[0] * shape[1] * 2
        ring = min(args.max_ring, max(2, -(-(LLC_BYTES * 3 // 2) // nbytes)))   # the ring holds 1.5 x the last-level cache where max-ring allows
        out.append((shape, g, ring))
    return out


def vgpr_counts():
    """{dtype name: VGPRs} of outlier_group_kernel from the resource remarks the build keeps beside the object, {} when they are not there"""
    path = os.path.join(ROOT, "dmx-compressor_amd", "build", "outlier_quant.o.remarks")
    names, out, cur = {"0": "f32", "1": "f16", "2": "bf16"}, {}, None
    try:
        for line in open(path, errors="replace"):
            m = re.search(r"Function Name: \S*outlier_group_kernelILi(\d)E", line)
            if m:
                cur = names.get(m.group(1))
            m = re.search(r"remark:\s+VGPRs: (\d+)", line)
            if m and cur:
                out[cur], cur = int(m.group(1)), None
    except OSError:
        pass
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    sides = ["dynamic"] + [f"{side}{k}" for k in args.ks for side in ("fused", "chain")]
    if args.dry_run:
        for shape, g, ring in rows:
            print(f"{args.format} g {g} {list(shape)} bf16: ring of {ring} inputs ({ring * shape[0] * shape[1] * 2 / 2**20:.0f} MiB) and as many "
                  f"outputs per graph; {', '.join(sides)}; {args.warmup} + {args.replays} replays per side")
        return 0

    import torch
    import dmx_compressor_amd as d

    ops = d.ops
    dev = torch.device("cuda:0")
    fmt = args.format
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    vg = vgpr_counts()
    lines.append(f"# tools/bench_outlier.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = graph replay time / calls in the graph, median of {args.replays} replays "
                 f"[min .. max], the graphs of a row replayed in turn after {args.warmup} warm-up replays each; device events; rings of at most "
                 f"{args.max_ring} inputs; fusedK = ops.outlier_fixed_qdq(fused=True) with k = K outliers per group (one launch), chainK = the "
                 f"same with fused=False (the definition: torch.sort, scatter, where and ops.dynamic_fixed_qdq per row), dynamic = "
                 f"ops.dynamic_fixed_qdq per_group of the same size (one launch, the k = 0 floor); format {fmt}, affine scheme, outlier_format "
                 f"None; per outlier = (fusedK - dynamic) / K; class = ops.outlier_class of the row")
    lines.append("# outlier_group_kernel VGPRs (the build's resource remarks, no scratch): "
                 + (", ".join(f"{k} {v}" for k, v in sorted(vg.items())) if vg else "remarks file not found beside the object"))
    lines.append("# not measured: f16 and f32 inputs, group sizes other than 64 and 128, k = 8, an outlier_format, the symmetric scheme")

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
        cls = ops.outlier_class(g, torch.bfloat16)
        fns = [("dynamic", lambda x: ops.dynamic_fixed_qdq(x, fmt, "per_group", g, fused=True))]
        for k in args.ks:
            fns.append((f"fused{k}", lambda x, k=k: ops.outlier_fixed_qdq(x, fmt, g, k, fused=True)))
            fns.append((f"chain{k}", lambda x, k=k: ops.outlier_fixed_qdq(x, fmt, g, k, fused=False)))
        graphs = [(label,) + graph_of(fn, ring) for label, fn in fns]
        for _ in range(args.warmup):
            for _, gr, _ in graphs:
                replay_ms(gr)
        times = {label: [] for label, _, _ in graphs}
        for _ in range(args.replays):
            for label, gr, _ in graphs:
                times[label].append(1000.0 * replay_ms(gr) / len(ring))
        m = {k: med(v) for k, v in times.items()}
        line = f"{fmt} g {g} {list(shape)} bf16 (class {cls}, ring {len(ring)}):"
        for label in sides:
            t = times[label]
            line += f" {label} {m[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}];"
        line += " " + ", ".join(f"chain{k} / fused{k} {m[f'chain{k}'] / m[f'fused{k}']:.1f}x" for k in args.ks)
        line += "; per outlier " + ", ".join(f"k = {k}: {(m[f'fused{k}'] - m['dynamic']) / k:.2f} us" for k in args.ks)
        line += "; fusedK / dynamic " + ", ".join(f"{m[f'fused{k}'] / m['dynamic']:.2f}x" for k in args.ks)
        if any(m[f"fused{k}"] >= m[f"chain{k}"] for k in args.ks):
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
