"""The integer matmul on the GPU: ops.int_matmul_packed (csrc/int_matmul.hip, the int8-MFMA kernel on packed operands) alone, with
both ops.dynamic_int_pack launches in front of it (ops.int_matmul), with the activation pack only (weights packed once: a deployment),
beside today's path for the same casts -- two ops.dynamic_fixed_qdq and torch.matmul in bf16 -- and beside ops.bfp_matmul_packed at
B = 64, all on the same buffers.  Writes profiles/r31_int_matmul.txt (first line: tools/stamp.py --header).

Nothing is gated on a speed here: the op is opt-in and computes something else than today's path (the integer dot product).  A row
where kernel + activation pack is slower than today's path says so.  Shapes: the Linear layers of tests/_model_shapes.py's
llama3_8b_block and opt125m_layer.  Method (tools/bench_bfp_matmul.py's): eager calls over a ring of operand pairs larger than the
256 MiB last-level cache; a timed window is whole passes over the ring lasting at least --window-ms, device events around it; the
sides' windows alternate; per side the median over the windows of (window time / calls) and the spread.

    python tools/bench_int_matmul.py                  # the full table, written to profiles/
    python tools/bench_int_matmul.py --dry-run        # no GPU: the plan, nothing timed or written
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 << 20
SHAPES = "8192x4096x4096,8192x4096x14336,2048x768x768"   # M x K x N: x [M, K] times w [N, K]^T
SIDES = ("kernel", "packs+kernel", "apack+kernel", "today", "bfp64")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated MxKxN (bf16 x [M, K], w [N, K])")
    ap.add_argument("--groups", default="0,128", help="comma-separated weight group sizes (0: per-row scales, the row class)")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per side")
    ap.add_argument("--window-ms", type=float, default=40.0, help="least duration of a timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_int_matmul.txt"), help="where the table is written")
    ap.add_argument("--dry-run", action="store_true", help="print the plan without touching a GPU")
    ap.add_argument("--no-write", action="store_true", help="do not write the table")
    a = ap.parse_args(argv)
    a.shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",") if s]
    if any(len(d) != 3 or min(d) < 1 for d in a.shapes):
        ap.error("shapes: MxKxN")
    a.groups = [int(g) for g in a.groups.split(",") if g]
    if a.windows < 3:
        ap.error("at least 3 timed windows")
    return a


def plan(args):
    """[(M, K, N, G, ring)]: the ring holds 1.5 x the last-level cache of bf16 operand pairs (2 .. 8 pairs)"""
    out = []
    for M, K, N in args.shapes:
        ring = min(8, max(2, -(-(LLC_BYTES * 3 // 2) // ((M + N) * K * 2))))
        out += [(M, K, N, G, ring) for G in args.groups if K % (G or 16) == 0]
    return out


def main(argv=None):
    args = parse_args(argv)
    rows = plan(args)
    if args.dry_run:
        for M, K, N, G, ring in rows:
            print(f"[{M},{K}] x [{N},{K}] bf16 XP[8,0], weight scales per {G or 'row'}: ring of {ring} operand pairs, "
                  f"{2 * M * N * K / 1e12:.3f} Top per call; {', '.join(SIDES)}; {args.windows} windows of >= {args.window_ms} ms per side")
        return 0

    import torch
    import dmx_compressor_amd as dmx

    ops, fmt = dmx.ops, "XP[8,0](CSN)"
    dev = torch.device("cuda:0")
    lines = []
    if not args.no_write:
        lines.append(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "stamp.py"), "--header"], text=True).strip())
    lines.append(f"# tools/bench_int_matmul.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
                 f"{time.strftime('%Y-%m-%d')}; us per call = window time / calls, median of {args.windows} windows [min .. max], a window = "
                 f"whole passes over the ring lasting >= {args.window_ms} ms, eager calls, device events, the sides' windows alternating; "
                 f"Top/s = 2 M N K / median; kernel = ops.int_matmul_packed(fused=True); packs+kernel = ops.int_matmul (both "
                 f"ops.dynamic_int_pack launches and the kernel); apack+kernel = the activation pack and the kernel on weights packed once; "
                 f"today = ops.dynamic_fixed_qdq of both operands (symmetric) and torch.matmul in bf16; bfp64 = ops.bfp_matmul_packed "
                 f"BFP[8|8]{{64}} on the same shape; bf16 inputs and outputs, {fmt}, activations per token, weights per row or per group G")

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
    for M, K, N, G, ring_n in rows:
        gw, gs = ("per_group", G) if G else ("per_token", None)
        raw = [((torch.randn((M, K), generator=gen, device=dev) * 0.7).to(torch.bfloat16),
                (torch.randn((N, K), generator=gen, device=dev) * 0.05).to(torch.bfloat16)) for _ in range(ring_n)]
        packed = [ops.dynamic_int_pack(x, fmt) + ops.dynamic_int_pack(w, fmt, gw, gs) for x, w in raw]
        half = [(x, p[2], p[3]) for (x, _), p in zip(raw, packed)]
        bfp = [ops.bfp_pack(x, 8, 64) + ops.bfp_pack(w, 8, 64) for x, w in raw] if K % 64 == 0 else None

        def apack(p):
            ca, sa = ops.dynamic_int_pack(p[0], fmt)
            return ops.int_matmul_packed(ca, sa, p[1], p[2], gs, out_dtype=torch.bfloat16, fused=True)

        sides = [("kernel", lambda p: ops.int_matmul_packed(*p, gs, out_dtype=torch.bfloat16, fused=True), packed),
                 ("packs+kernel", lambda p: ops.int_matmul(p[0], p[1], fmt, None, "per_token", gw, gs, fused=True), raw),
                 ("apack+kernel", apack, half),
                 ("today", lambda p: torch.matmul(ops.dynamic_fixed_qdq(p[0], fmt, symmetric_qscheme=True),
                                                  ops.dynamic_fixed_qdq(p[1], fmt, gw, gs, symmetric_qscheme=True).t()), raw)]
        if bfp is not None:
            sides.append(("bfp64", lambda p: ops.bfp_matmul_packed(*p, 8, 8, 64, out_dtype=torch.bfloat16, fused=True), bfp))
        passes = {}
        for label, fn, ring in sides:   # warm-up (code objects, the BLAS's choice) and the number of passes a window needs
            window(fn, ring, 1)
            passes[label] = max(1, int(args.window_ms * 1000.0 / (window(fn, ring, 1) * len(ring))) + 1)
        times = {label: [] for label, _, _ in sides}
        for _ in range(args.windows):
            for label, fn, ring in sides:
                times[label].append(window(fn, ring, passes[label]))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        cls = ops.int_matmul_class(packed[0][0], packed[0][2], 0, G)
        line = f"[{M},{K}] x [{N},{K}] bf16 {fmt} weight scales per {G or 'row'} (class {cls}):"
        for label in times:
            t = times[label]
            line += f" {label} {med[label]:.1f} us [{min(t):.1f} .. {max(t):.1f}], {2.0 * M * N * K / (med[label] * 1e-6) / 1e12:.1f} Top/s;"
        line += f" today / kernel {med['today'] / med['kernel']:.2f}x, today / apack+kernel {med['today'] / med['apack+kernel']:.2f}x"
        if med["apack+kernel"] >= med["today"]:
            line += " ** SLOWER THAN TODAY'S PATH **"
            slower.append((M, K, N, G))
        print(line, flush=True)
        lines.append(line)
        del raw, packed, half, bfp, sides
        torch.cuda.empty_cache()
    lines.append("# apack+kernel is faster than today's path on every row" if not slower else f"# SLOWER THAN TODAY'S PATH (apack+kernel): {slower}")
    lines.append("# not measured: f16 / f32 outputs, G = 32 / 64, grouped activation scales, XP[4,0], the kernel against its chain")
    print(lines[-2], flush=True)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
