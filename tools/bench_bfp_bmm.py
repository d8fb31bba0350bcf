"""The batched BFP matmul on the GPU, on the two products of an attention layer: ops.bfp_bmm_packed (csrc/bfp_bmm.hip) alone, with
the two packs in front of it (ops.bfp_bmm: ops.bfp_pack of the first operand and, for P V, the column-blocked pack of V), and beside
today's path for the same formats -- ops.bfp_qdq of both operands and torch.matmul in bf16 -- on the same buffers.  Writes
profiles/r30_bfp_bmm.txt (first line: tools/stamp.py --header).

Nothing is gated on a speed: the op is opt-in for what it computes.  A row where it is slower than today's path says so.

Method (tools/bench_bfp_matmul.py's): eager calls over a ring of operand pairs larger than the 256 MiB last-level cache; a timed window
is a whole number of passes over the ring lasting at least --window-ms, device events around it; the sides' windows alternate; per
side the median over the windows of (window time / calls) and the spread.  Top/s = 2 batch M N K / median.

    python tools/bench_bfp_bmm.py                  # the full table, written to profiles/
    python tools/bench_bfp_bmm.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
SHAPES = "192x2048x64,256x2048x128"   # batch * heads x sequence x head_dim
SIDES = ("kernel", "pack+kernel", "today")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated BHxSxD (bf16 q, k, v [BH, S, D])")
    ap.add_argument("--blocks", default="64,32", help="comma-separated block sizes of BFP[8|8]{B}")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per side")
    ap.add_argument("--window-ms", type=float, default=60.0, help="least duration of a timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_bfp_bmm.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    shapes = []
    for s in a.shapes.split(","):
        dims = tuple(int(v) for v in s.lower().split("x")) if s else ()
        if len(dims) != 3 or min(dims) < 1:
            ap.error(f"shape {s}: BHxSxD")
        shapes.append(dims)
    a.shapes = shapes
    a.blocks = [int(b) for b in a.blocks.split(",") if b]
    if a.windows < 3:
        ap.error("at least 3 timed windows")
    return a


def plan(args):
    """[(product, layout, batch, M, K, N, B, ring)]: Q K^T is [S, D] x [S, D]^T ("nk"), P V is [S, S] x [S, D] ("kn"); the ring holds
    1.5 x the last-level cache of bf16 operand pairs (2 .. 8 pairs)"""
    out = []
    for bh, S, D in args.shapes:
        for name, layout, M, K, N in (("QK^T", "nk", S, D, S), ("PV", "kn", S, S, D)):
            ring = min(8, max(2, -(-(LLC_BYTES * 3 // 2) // (bh * (M + N) * K * 2))))
            out += [(name, layout, bh, M, K, N, B, ring) for B in args.blocks if K % B == 0]
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for name, layout, bh, M, K, N, B, ring in rows:
            print(f"{name} [{bh},{M},{K}] x {layout} [{bh},{N if layout == 'nk' else K},{K if layout == 'nk' else N}] bf16 BFP[8|8]{{{B}}}: ring of "
                  f"{ring} operand pairs ({ring * bh * (M + N) * K * 2 / 2**20:.0f} MiB), {2 * bh * M * N * K / 1e12:.3f} Top per call; "
                  f"{', '.join(SIDES)}; {args.windows} windows of >= {args.window_ms} ms per side")
        return 0

    import torch
    import dmx_compressor_amd as dmx

    ops = dmx.ops
    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_bfp_bmm.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = window time / calls, median of {args.windows} windows [min .. max], a window = "
                 f"whole passes over the ring of operand pairs lasting >= {args.window_ms} ms, eager calls (the host's launch cost is inside), "
                 f"device events, the sides' windows alternating; Top/s = 2 batch M N K / median; kernel = ops.bfp_bmm_packed(fused=True) on "
                 f"packed operands (one launch), pack+kernel = ops.bfp_bmm(fused=True) (two pack launches -- for PV the second is the "
                 f"column-blocked pack -- and the kernel), today = ops.bfp_qdq of both operands (V along dim -2) and torch.matmul in bf16; "
                 f"bf16 inputs and outputs, BFP[8|8]{{B}}(SN) for both operands; P is uniform in [0, 1 / 64)")

    def window(fn, ring, passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(passes):
            for item in ring:
                fn(item)
        b.record()
        torch.cuda.synchronize()
        return 1000.0 * a.elapsed_time(b) / (passes * len(ring))   # us per call

    gen = torch.Generator(device=dev).manual_seed(0)
    slower = []
    for name, layout, bh, M, K, N, B, ring_n in rows:
        f, kn = f"BFP[8|8]{{{B}}}(SN)", layout == "kn"
        if kn:
            raw = [((torch.rand((bh, M, K), generator=gen, device=dev) / 64).to(torch.bfloat16),
                    (torch.randn((bh, K, N), generator=gen, device=dev) * 0.7).to(torch.bfloat16)) for _ in range(ring_n)]
        else:
            raw = [((torch.randn((bh, M, K), generator=gen, device=dev) * 0.7).to(torch.bfloat16),
                    (torch.randn((bh, N, K), generator=gen, device=dev) * 0.7).to(torch.bfloat16)) for _ in range(ring_n)]
        packed = [ops.bfp_pack(x, 8, B) + ops.bfp_pack(w, 8, B, block_dim=-2 if kn else -1, fused=True if kn else None) for x, w in raw]
        today = ((lambda p: torch.matmul(ops.bfp_qdq(p[0], 8, B), ops.bfp_qdq(p[1], 8, B, block_dim=-2))) if kn else
                 (lambda p: torch.matmul(ops.bfp_qdq(p[0], 8, B), ops.bfp_qdq(p[1], 8, B).transpose(-1, -2))))
        sides = [("kernel", lambda p: ops.bfp_bmm_packed(*p, 8, 8, B, layout, out_dtype=torch.bfloat16, fused=True), packed),
                 ("pack+kernel", lambda p: ops.bfp_bmm(p[0], p[1], f, w_layout=layout, fused=True), raw),
                 ("today", today, raw)]
        passes = {}
        for label, fn, ring in sides:   # warm-up (code objects, the BLAS's choice) and the number of passes a window needs
            window(fn, ring, 1)
            passes[label] = max(1, int(args.window_ms * 1000.0 / (window(fn, ring, 1) * len(ring))) + 1)
        times = {label: [] for label in SIDES}
        for _ in range(args.windows):
            for label, fn, ring in sides:
                times[label].append(window(fn, ring, passes[label]))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        line = (f"{name} [{bh},{M},{K}] x {layout} [{bh},{','.join(str(d) for d in raw[0][1].shape[1:])}] bf16 BFP[8|8]{{{B}}} "
                f"(class {ops.bfp_bmm_class(packed[0][0], packed[0][2], B, layout)}):")
        for label in SIDES:
            t = times[label]
            line += f" {label} {med[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}], {2.0 * bh * M * N * K / (med[label] * 1e-6) / 1e12:.1f} Top/s;"
        line += f" today / kernel {med['today'] / med['kernel']:.2f}x, today / pack+kernel {med['today'] / med['pack+kernel']:.2f}x"
        if med["pack+kernel"] >= med["today"]:
            line += " ** SLOWER THAN TODAY'S PATH **"
            slower.append((name, bh, M, K, N, B))
        print(line, flush=True)
        lines.append(line)
        del raw, packed, sides
        torch.cuda.empty_cache()
    lines.append("# pack+kernel is faster than today's path on every row" if not slower else f"# SLOWER THAN TODAY'S PATH (pack+kernel): {slower}")
    lines.append("# not measured: f16 / f32 outputs, B = 128, precisions below 8, asymmetric codes, the kernel against its chain (the chain is a "
                 "Python loop over batch elements and blocks), the column-blocked pack alone, LDS bank conflicts of the kn staging")
    print(lines[-2], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
