// csrc/row_class.hpp -- WHICH row kernel a softmax / LayerNorm / RMSNorm call launches (host only: no HIP call, no pointer is
// dereferenced).  approx.hip's softmax_dispatch / norm_dispatch take every decision from row_class_of and only map the class onto a
// kernel instantiation; dmxq_row_class_of (include/dmxq.h) hands the same answer to the tests, which pin every class by it.
#pragma once
#include "common.hpp"

namespace dmxq {

constexpr int kRowLdsFloats = 16 * 1024;  // 64 KiB per workgroup -> 2 workgroups per CU

#ifdef DMXQ_EXP_LN32
constexpr int kLn32OnePass = DMXQ_EXP_LN32;
#else
constexpr int kLn32OnePass = 0;
#endif

// row slots per wave iteration: about 32 fp32 values per lane (occupancy beats bytes in flight per wave here: 64 was
// 1-4 % slower on every shape of tools/bench_rows.py)
constexpr int rows_per_wave(int vpl, int epl) { return 32 / (vpl * epl) >= 4 ? 4 : (32 / (vpl * epl) >= 2 ? 2 : 1); }
// rows per iteration of the workgroup-per-row kernel, and of its one-pass form for tensors of 26-32 MiB (norm_dispatch)
constexpr int block_rows(int vpl, int epl) { return vpl * epl <= 32 ? 2 : 1; }
constexpr int block_rows_mid(int vpl) { return 16 / vpl >= 8 ? 8 : (16 / vpl >= 4 ? 4 : 2); }

// lane-vector width for the wave kernels: 16 bytes when rows and bases allow it, else 8 bytes for 16-bit rows that are
// a multiple of 4 elements; 0 = not applicable
static inline int wave_epl(int dt, int64_t cols, const void* p0, const void* p1, const void* p2, const void* p3) {
  const uintptr_t a = (uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3;
  const int full = dt == DMXQ_F32 ? 4 : 8;
  if (cols % full == 0 && (a & 15) == 0) return full;
  if (dt != DMXQ_F32 && cols % 4 == 0 && (a & 7) == 0) return 4;
  return 0;
}

// (lanes per row, vectors per lane) for a row of nv vectors: the instantiated shape with the fewest idle lane slots.
// 64 lanes: VPL in {1,2,3,4,5,6,8,10,12,16}; 32 lanes: VPL in {1,3,5}.  vpl = 0: row too long for registers.
static inline void wave_shape(int64_t nv, int* lpr, int* vpl) {
  static const int v64[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16}, v32[] = {1, 3, 5};
  int64_t best = 0;
  *lpr = 64; *vpl = 0;
  for (int v : v64)
    if ((int64_t)v * 64 >= nv) { best = (int64_t)v * 64; *vpl = v; break; }
  for (int v : v32)
    if ((int64_t)v * 32 >= nv) { if (best == 0 || (int64_t)v * 32 < best) { *lpr = 32; *vpl = v; } break; }
}

// the consumer's BFP blocks of B elements as lpb adjacent lanes of one slot: 0 = not a size the fused epilogue takes
static inline int row_bfp_lpb(int64_t B, int epl, int lpr) {
  if (B < 1 || B > 512 || B % epl != 0) return 0;
  const int lpb = (int)(B / epl);
  return (lpb & (lpb - 1)) == 0 && lpb <= lpr ? lpb : 0;
}

// The class of one call.  cast_kind: DMXQ_ROWCAST_NONE = the plain entry points; anything else = the fused-cast ones (dtype_out and
// dtype_wb equal dtype_in there); bfp_block: 0, or the block size of the *_cast_bfp entry.  rows and cols >= 1.
static inline dmxq_row_class row_class_of(int op, int dtype_in, int dtype_out, int dtype_wb, int64_t rows, int64_t cols, const void* in,
                                          const void* out, const void* weight, const void* bias, int cast_kind, int64_t bfp_block) {
  dmxq_row_class c = {};  // family = DMXQ_ROWK_UNSUPPORTED, grid = DMXQ_ROWGRID_NONE
  const bool cast = cast_kind != DMXQ_ROWCAST_NONE;
  const int full = dtype_in == DMXQ_F32 ? 4 : 8;
  const uintptr_t io = reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out);
  auto fallback = [&]() {
    if (cast) return c;  // the fused-cast form exists for register-resident rows only
    c.family = cols <= kRowLdsFloats ? DMXQ_ROWK_LDS_ROWS : DMXQ_ROWK_GLOBAL_ROWS;
    c.grid = DMXQ_ROWGRID_CAPPED;
    c.rows_per_iter = 1;
    return c;
  };
  if (op == DMXQ_ROW_SOFTMAX) {
    // register-resident kernel: same dtype in and out, a row of 1 .. 1024 lane-vectors.  Rows that are whole aligned
    // vectors take the aligned form; any other length / alignment the RAG form (unaligned 16-byte accesses + element tail)
    const uintptr_t eb = dtype_in == DMXQ_F32 ? 4 : 2;
    if (!(dtype_in == dtype_out && (io & (eb - 1)) == 0 && cols >= full && (cols + full - 1) / full <= 64 * 16)) return fallback();
    bool rag = !(cols % full == 0 && (io & 15u) == 0);
    // 16-bit rows that are a multiple of 4 elements on 8-byte bases: aligned 8-byte lane-vectors (measured 5 % faster
    // than the unaligned 16-byte form with an overlapped last vector on attention rows of 1500: 21.8 vs 22.9 us)
    const bool half_vec = rag && full == 8 && cols % 4 == 0 && cols / 4 <= 64 * 16 && (io & 7u) == 0;
    if (half_vec) rag = false;
    int lpr, vpl;
    wave_shape(half_vec ? cols / 4 : (cols + full - 1) / full, &lpr, &vpl);
    const int epl = half_vec ? 4 : full;
    if (bfp_block) {  // dmxq_softmax_cast_bfp: whole vectors, blocks of lpb adjacent lanes of one slot
      if (!cast || rag || !row_bfp_lpb(bfp_block, epl, lpr)) return c;
      c.bfpout = 1;
    }
    c.family = DMXQ_ROWK_WAVE;
    c.epl = epl; c.vpl = vpl; c.lpr = lpr;
    c.rag = rag; c.half_vec = half_vec;
    c.fast32 = dtype_in == DMXQ_F32 && !rag && cast_kind == DMXQ_ROWCAST_MAN16;
    c.grid = DMXQ_ROWGRID_ONE_PASS;
    c.rows_per_iter = 4 * rows_per_wave(vpl, epl) * (64 / lpr);
    return c;
  }
  const bool rms = op == DMXQ_ROW_RMSNORM;
  const bool same = dtype_in == dtype_out && ((!weight && !bias) || dtype_wb == dtype_in);
  const int epl = same ? wave_epl(dtype_in, cols, in, out, weight, bias) : 0;
  // (round 3: the wave kernel at 512 vectors per row -- one wave per 4096-element bf16 row, 8 vectors per lane -- measured 15.6 us against
  // the workgroup-per-row kernel's 13.4 us on 4096 x 4096)
  if (epl == full && cols / epl > 256 && cols / epl <= 8 * kThreads) {  // long rows: workgroup per row
    const int need = (int)((cols / epl + kThreads - 1) / kThreads);
    const int vpl = need <= 6 ? need : 8;
    if (bfp_block) {
      if (!cast || !row_bfp_lpb(bfp_block, epl, 64)) return c;
      c.bfpout = 1;
    }
    c.family = DMXQ_ROWK_BLOCK;
    c.epl = epl; c.vpl = vpl; c.lpr = kThreads;
    c.grid = DMXQ_ROWGRID_PERSISTENT;
    c.rows_per_iter = block_rows(vpl, epl);
    // rows per workgroup iteration (round 3, tools/tune_rows -> profiles/r03_tune_rows.txt, RMSNorm / LayerNorm rows of 4096 bf16): 2, on a
    // persistent grid (2560 / 3072 x 4096: 8.2 / 9.9 us against 9.3 / 10.8 us for one pass per workgroup) -- except tensors of 26-32 MiB,
    // which fit the chip in ONE round of workgroups when each lane keeps ~16 vectors in flight: 8 rows per workgroup, one pass, 10.9 /
    // 11.5 us against 11.9 / 13.2 us on 3584 / 4096 x 4096 (RMSNorm 63 -> 72 % of the roofline; LayerNorm 13.7 -> 12.3 us).  The fused
    // module form (CAST) gains 2 % at most from it and keeps the one geometry.
    const int64_t bytes = rows * cols * (dtype_in == DMXQ_F32 ? 4 : 2);
    const bool mid = bytes > ((int64_t)26 << 20) && bytes <= ((int64_t)32 << 20);
    if (mid && !c.bfpout) {
      if (cast && rms && vpl == 2 && epl == 8) {  // the RMSNorm MODULE on 16-bit rows of 4096: four rows, persistent (norm_dispatch)
        c.grid = DMXQ_ROWGRID_MODULE_ROWS4;
        c.rows_per_iter = 4;
      } else if (!cast && block_rows_mid(vpl) != c.rows_per_iter) {
        c.grid = DMXQ_ROWGRID_MID_ONE_PASS;
        c.rows_per_iter = block_rows_mid(vpl);
      }
    }
    return c;
  }
  if (epl && cols <= (int64_t)64 * epl * 16) {
    int lpr, vpl;
    wave_shape(cols / epl, &lpr, &vpl);
    if (bfp_block) {
      if (!cast || !row_bfp_lpb(bfp_block, epl, lpr)) return c;
      c.bfpout = 1;
    }
    c.family = DMXQ_ROWK_WAVE;
    c.epl = epl; c.vpl = vpl; c.lpr = lpr;
    c.half_vec = epl != full;
    c.grid = DMXQ_ROWGRID_PERSISTENT;
    c.rows_per_iter = 4 * rows_per_wave(vpl, epl) * (64 / lpr);
    // the LayerNorm MODULE on 16-bit rows of 768: one pass per workgroup (norm_dispatch)
    if (cast && !rms && !c.bfpout && vpl == 3 && ((epl == 8 && lpr == 32) || (kLn32OnePass > 0 && epl == 4 && lpr == 64)))
      c.grid = DMXQ_ROWGRID_MODULE_ONE_PASS;
    return c;
  }
  return fallback();
}

}  // namespace dmxq
