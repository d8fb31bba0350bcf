// csrc/gptq_cols.hpp — GPTQ's in-block column loop, shared by its two kernels: csrc/gptq.hip (dmxq_gptq_block: every cast parameter is
// fixed before the launch) and csrc/gptq_dynamic.hip (dmxq_gptq_block_dynamic: integer scales per group of input columns, derived inside
// the loop from the row's current values).  The geometry, the LDS layout and the arithmetic order are documented in csrc/gptq.hip; the
// two kernels differ only in where a FIXED cast's (scale, zero point) come from, chosen at compile time by the SCALES argument.
#pragma once
#include <math.h>

#include "bfp_math.hpp"
#include "fixedq.hpp"
#include "floatq.hpp"
#include "format_desc.hpp"
#include "reduce_common.hpp"

namespace dmxq {

constexpr int kGptqCols = 128;  // largest column block
constexpr int kGptqRows = 64;   // rows per workgroup: one wave, one lane per row

struct GptqCast {
  int wl;         // BFP precision
  uint64_t ends;  // BFP: bit i set <=> column i of a microblock closes a block
  FloatFmt f;     // FLOAT
  FixedFmt x;     // FIXED
  int per_row;    // FIXED: scale / zero point indexed by row
};

// where a FIXED cast's scale and zero point come from
struct GptqStoredScales {  // the caller's arrays, read once before the column loop (dmxq_gptq_block)
  static constexpr bool dynamic = false;
};
struct GptqGroupScales {   // one per row and group of `group` columns, derived at the group's first column (dmxq_gptq_block_dynamic)
  static constexpr bool dynamic = true;
  int group, group_log2;   // a power of two, a multiple of 4 and of the microblock; divides count
  int qmin, qmax, sym;     // dmxq_qparams' arguments
  float* scale_out;        // [rows, count / group], row stride lds
  int64_t* zp_out;         // [rows, count / group], row stride ldz
  int64_t lds, ldz;
};

// q[0 .. m) = cast of the slice w[0 .. m) of this lane's row
template <int KIND, int MB, bool ASYM>
__device__ __forceinline__ void gptq_cast(const float* w, int m, const GptqCast& c, float sc, float z, float* q) {
  if constexpr (KIND == DMXQ_GPTQ_FLOAT) {
#pragma unroll
    for (int i = 0; i < MB; i++)
      if (i < m) q[i] = float_q1<DMXQ_ROUND_NEAREST>(w[i], c.f, 0u);
  } else if constexpr (KIND == DMXQ_GPTQ_FIXED) {
#pragma unroll
    for (int i = 0; i < MB; i++)
      if (i < m) q[i] = fixed_affine_q1(w[i], sc, z, c.x);
  } else {
    // block maxima of |w| on the bit patterns (what the BFP kernels compare): a running maximum that restarts after each block end,
    // then walked back so that every element sees the maximum of its whole block
    uint32_t pm[MB];
    uint32_t run = 0u;
#pragma unroll
    for (int i = 0; i < MB; i++) {
      if (i < m) {
        const uint32_t v = f2u(w[i]) & 0x7FFFFFFFu;
        run = (i == 0 || ((c.ends >> (i - 1)) & 1u)) ? v : (run > v ? run : v);
        pm[i] = run;
      }
    }
    uint32_t bm = 0u;
#pragma unroll
    for (int i = MB - 1; i >= 0; i--) {
      if (i < m) {
        if (i == m - 1 || ((c.ends >> i) & 1u)) bm = pm[i];
        const BfpBlockParams p = bfp_block_params<ASYM, false>(bm, c.wl);
        q[i] = bfp_q1<DMXQ_ROUND_NEAREST, ASYM>(w[i], p, c.wl, DMXQ_ROUND_NEAREST, 0u);
      }
    }
  }
}

// one workgroup's 64 rows of one column block; called by every lane of the one-wave workgroup
template <int KIND, int MB, bool ASYM, class SCALES>
__device__ __forceinline__ void gptq_block_body(const float* __restrict__ wsrc, int64_t ldw, float* __restrict__ qdst, int64_t ldq,
                                                float* __restrict__ edst, int64_t lde, int64_t rows, int count,
                                                const float* __restrict__ hinv, int64_t ldh, const float* __restrict__ inv_d,
                                                const float* __restrict__ scale, const int64_t* __restrict__ zp, const GptqCast& c,
                                                const SCALES& dyn) {
  __shared__ float4 hs[kGptqCols * kGptqCols / 4];  // Hinv block, row j = hs[j * 32 .. j * 32 + 32)
  __shared__ float4 ws[kGptqCols / 4 * kGptqRows];  // the rows' block, columns 4 g .. 4 g + 3 of lane l at ws[g * 64 + l]; Q once final
  __shared__ float es[kGptqCols * kGptqRows];       // E, column k of lane l at es[k * 64 + l]
  float* const hf = (float*)hs;
  float* const wf = (float*)ws;
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kGptqRows;
  const int nr = rows - row0 < kGptqRows ? (int)(rows - row0) : kGptqRows;
  // the Hinv block: upper triangle of rows j < count, columns k < count; zero elsewhere (rows >= count are never read)
  for (int i = lane; i < count * kGptqCols; i += kGptqRows) {
    const int j = i / kGptqCols, k = i % kGptqCols;
    hf[i] = (k < count && k >= j) ? hinv[(int64_t)j * ldh + k] : 0.0f;
  }
  // the workgroup's rows, read along the rows (coalesced); rows past the last one, and the columns from `count` up to the next multiple
  // of four (which the four-column update reads and writes, and nothing outputs), are zero
  const int cpad = (count + 3) & ~3;
  for (int i = lane; i < kGptqRows * cpad; i += kGptqRows) {
    const int rl = i / cpad, k = i % cpad;
    wf[((k >> 2) * kGptqRows + rl) * 4 + (k & 3)] = rl < nr && k < count ? wsrc[(row0 + rl) * ldw + k] : 0.0f;
  }
  float sc = 1.0f, z = 0.0f;
  if constexpr (KIND == DMXQ_GPTQ_FIXED && !SCALES::dynamic) {
    const int64_t g = c.per_row ? row0 + (lane < nr ? lane : nr - 1) : 0;
    sc = scale[g];
    z = (float)zp[g];
  }
  __syncthreads();
  auto col = [&](int k) -> float& { return wf[((k >> 2) * kGptqRows + lane) * 4 + (k & 3)]; };

  for (int j1 = 0; j1 < count; j1 += MB) {
    const int m = count - j1 < MB ? count - j1 : MB;
    if constexpr (SCALES::dynamic) {
      // a group starts here (microblocks never straddle one): the extrema of the row's `group` columns AS THEY STAND -- every update of
      // the earlier microblocks and blocks is in them -- as dmxq_group_minmax reports them (a NaN makes both NaN, which qparams_one's
      // fminf / fmaxf drop: reduce_common.hpp FloatExtrema, which the dynamic cast uses too), then dmxq_qparams' own function.  A
      // lane-local scan of group / 4 LDS slots.
      if ((j1 & (dyn.group - 1)) == 0) {
        FloatExtrema ext;
        ext.init();
        for (int t = 0; t < (dyn.group >> 2); t++) {
          const float4 v = ws[((j1 >> 2) + t) * kGptqRows + lane];
          ext.add(v.x);
          ext.add(v.y);
          ext.add(v.z);
          ext.add(v.w);
        }
        int64_t zq;
        qparams_one(ext.mn(), ext.mx(), dyn.qmin, dyn.qmax, dyn.sym, sc, zq);
        z = (float)zq;
        if (lane < nr) {
          const int64_t g = j1 >> dyn.group_log2;
          dyn.scale_out[(row0 + lane) * dyn.lds + g] = sc;
          dyn.zp_out[(row0 + lane) * dyn.ldz + g] = zq;
        }
      }
    }
    float x[MB], q[MB], e[MB];
#pragma unroll
    for (int i = 0; i < MB; i++) x[i] = i < m ? col(j1 + i) : 0.0f;
    gptq_cast<KIND, MB, ASYM>(x, m, c, sc, z, q);
#pragma unroll
    for (int i = 0; i < MB; i++) {
      if (i < m) col(j1 + i) = q[i];  // (the column is final: its slot now holds Q)
      x[i] = i < m ? x[i] - q[i] : 0.0f;
    }
    const float* D = inv_d + (int64_t)(j1 / MB) * MB * MB;
    if constexpr (SCALES::dynamic && MB == 64) {
      // 64 x 64 products are past what the unroller takes in one nest: with the outer loop left rolled by the compiler, e[cc] is indexed at
      // run time and the array goes to scratch (272 bytes per lane).  Here the outer loop is rolled ON PURPOSE and writes E's LDS slots
      // only; the lane reads its own 64 slots back into registers with constant indices.  Same products, same order.  (m == MB: a
      // group is a whole number of microblocks.)
#pragma unroll 1
      for (int cc = 0; cc < MB; cc++) {
        float acc = x[0] * D[cc];
#pragma unroll
        for (int i = 1; i < MB; i++) acc = acc + x[i] * D[i * MB + cc];
        es[(j1 + cc) * kGptqRows + lane] = acc;
      }
#pragma unroll
      for (int i = 0; i < MB; i++) e[i] = es[(j1 + i) * kGptqRows + lane];
    } else {
#pragma unroll
      for (int cc = 0; cc < MB; cc++) {
        e[cc] = 0.0f;
        if (cc < m) {
          float acc = x[0] * D[cc];
#pragma unroll
          for (int i = 1; i < MB; i++)
            if (i < m) acc = acc + x[i] * D[i * MB + cc];
          e[cc] = acc;
          es[(j1 + cc) * kGptqRows + lane] = acc;
        }
      }
    }
    // the block's later columns, four at a time (only after a whole microblock: a ragged one is the block's last)
    const int k1 = j1 + MB;
    for (int k0 = k1 & ~3; k0 < count; k0 += 4) {
      float acc[4];
#pragma unroll
      for (int i = 0; i < MB; i++) {
        const float4 h = hs[(j1 + i) * (kGptqCols / 4) + (k0 >> 2)];
        const float hv[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = i == 0 ? e[0] * hv[t] : acc[t] + e[i] * hv[t];
      }
      float4& wv = ws[(k0 >> 2) * kGptqRows + lane];
      float4 v = wv;
      float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 4; t++)
        if (k0 + t >= k1) vv[t] = vv[t] - acc[t];
      wv = float4{vv[0], vv[1], vv[2], vv[3]};
    }
  }
  __syncthreads();
  // Q and E out, along the rows (coalesced)
  for (int i = lane; i < nr * count; i += kGptqRows) {
    const int rl = i / count, k = i % count;
    qdst[(row0 + rl) * ldq + k] = wf[((k >> 2) * kGptqRows + rl) * 4 + (k & 3)];
    edst[(row0 + rl) * lde + k] = es[k * kGptqRows + rl];
  }
}

}  // namespace dmxq
