// csrc/awq.hip — AWQ (Lin et al., 2023): the error of ONE candidate scale vector in ONE launch (include/dmxq.h dmxq_awq_group_error;
// DESIGN.md §8 "AWQ").  Not in the reference.
//
// For a weight w[rows, L] of dtype T, a float32 scale vector s[L] and a per-group dynamic integer format:
//   ws = T(fp32(w) * s[column])                 one fp32 multiply, one rounding to T             (ops.scale_channels, multiply)
//   wq = dmxq_dynamic_fixed_qdq(ws, group)      the cast of csrc/dynamic_quant.hip, in T         (dyn_group_kernel)
//   d  = fp32(wq) / s[column] - fp32(w)         one IEEE fp32 division, one fp32 subtraction     (ops.scale_channels, divide; torch's -)
// The contract is that four-launch chain, bit for bit: the cast's pieces are the SAME code (csrc/dynamic_quant.hpp), fed the same values.
// bf16: 2 B read, 4 B (d) + 2 B (wq, optional) written per element against the chain's ~22 B.
//
// Geometry.  The wide side decides what a lane owns (DESIGN_rounds1-5 "every memory instruction of a wave covers whole lines, 16 bytes per
// lane": a lane that owned 16 bytes of a 16-bit weight would write its eight float32 errors as two 16-byte stores 32 bytes apart, each
// instruction touching half of every line): a lane owns FOUR consecutive elements whatever the dtype -- one 16-byte load of the scales,
// one 16-byte store of d, and 16-byte (fp32) or 8-byte (16-bit) accesses of w and wq.  A group of G elements is G / 4 adjacent lanes
// (4 .. 64: G a power of two from 16 to 256), its extrema combined by DPP / xor shuffles on order-preserving keys.  A wave takes U x 64
// consecutive lane-vectors; the grid does not loop.  Lanes past the end re-read the last vector, meet only each other (the tensor ends
// on a group boundary) and store nothing.  A lane-vector never straddles a row (L % G == 0, G % 4 == 0), so its first column is
// (vector index mod vectors per row) x 4: one 32-bit remainder per lane, advanced by 64 mod (vectors per row) per slot.
// No workspace, no allocation, no synchronisation with the host: capturable.
#include <math.h>

#include "awq_lane4.hpp"
#include "dynamic_geom.hpp"
#include "dynamic_quant.hpp"

namespace dmxq {
namespace {

// groups of `lanes` adjacent lanes; nvec lane-vectors in all (a multiple of `lanes`); wave w takes vectors [w U 64, (w + 1) U 64)
template <int DT, int U>
__global__ __launch_bounds__(kDynThreads) void awq_group_error_kernel(const void* __restrict__ w, const float* __restrict__ s, float* __restrict__ d_out,
                                                                     void* __restrict__ wq_out, uint32_t nvec, uint32_t vecs_per_row,
                                                                     uint32_t step_mod /* 64 % vecs_per_row */, int lanes, const DynFmt f) {
  constexpr int V = kAwqV;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wave = blockIdx.x * (uint32_t)(kDynThreads / kWave) + threadIdx.x / kWave;
  const uint32_t base = wave * (uint32_t)(U * kWave) + lane;   // (the host keeps nvec + a workgroup's span below 2^32)
  u32x4 raw[U];
  f32x4 sv[U];
  uint32_t c = base % vecs_per_row;
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint32_t i = base + (uint32_t)u * kWave;
    raw[u] = awq_load4<DT>(w, (int64_t)(i < nvec ? i : nvec - 1));
    sv[u] = *(const f32x4*)(s + (int64_t)c * V);   // (c < vecs_per_row also past the end: a valid address, the values are not stored)
    c += step_mod;
    c = c >= vecs_per_row ? c - vecs_per_row : c;
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint32_t i = base + (uint32_t)u * kWave;
    const float sc4[V] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w};
    float x[V], xs[V], y[V];
    awq_widen4<DT>(raw[u], x);
#pragma unroll
    for (int k = 0; k < V; k++) xs[k] = x[k] * sc4[k];
    awq_round4<DT>(xs);
    DynExt e;
    e.init();
#pragma unroll
    for (int k = 0; k < V; k++) e.FloatExtrema::add(xs[k]);
    uint32_t klo, khi;
    e.keys(klo, khi);
    dyn_group_minmax(klo, khi, lanes);
    DynSeg g;
    g.setup(klo, khi, f);
    const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(g.sc)) == 0ull;
    const bool all_zp0 = __builtin_amdgcn_ballot_w64(g.z != 0.0f) == 0ull;
    dyn_cast_vec<V>(xs, y, g, all_fast, all_zp0, f);
    const u32x4 q = awq_round4<DT>(y);
    float d[V];
#pragma unroll
    for (int k = 0; k < V; k++) d[k] = y[k] / sc4[k] - x[k];
    if (i < nvec) {
      if (wq_out) awq_store4<DT>(wq_out, (int64_t)i, q);
      *(f32x4*)(d_out + (int64_t)i * V) = f32x4{d[0], d[1], d[2], d[3]};
    }
  }
}

template <int DT>
int awq_launch(const void* w, const float* s, float* d_out, void* wq_out, int64_t n, int64_t L, int64_t group, const DynFmt& f, hipStream_t st) {
  const int64_t nvec = n / kAwqV;
  const int lanes = (int)(group / kAwqV);   // 4 .. 64
  const uint32_t vpr = (uint32_t)(L / kAwqV);
  // one vector per lane while that already fills the device, four independent loads per lane beyond (csrc/dynamic_quant.hip dyn_launch)
  const bool deep = plan_norm(nvec) > ((int64_t)1 << 19);
  const int64_t per_wg = (int64_t)kDynThreads * (deep ? 4 : 1);
  const int64_t grid = (nvec + per_wg - 1) / per_wg;
  if (grid * per_wg > 0xFFFFFFFFll || grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  if (deep) DMXQ_LAUNCH((awq_group_error_kernel<DT, 4>), dim3((unsigned)grid), dim3(kDynThreads), 0, st, w, s, d_out, wq_out, (uint32_t)nvec, vpr, (uint32_t)(kWave % vpr), lanes, f);
  else DMXQ_LAUNCH((awq_group_error_kernel<DT, 1>), dim3((unsigned)grid), dim3(kDynThreads), 0, st, w, s, d_out, wq_out, (uint32_t)nvec, vpr, (uint32_t)(kWave % vpr), lanes, f);
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

// 1: dmxq_awq_group_error takes rows of L elements of dtype_w with groups of `group` (given 16-byte aligned pointers), 0: it refuses them
extern "C" int dmxq_awq_class(int dtype_w, int64_t L, int64_t group) {
  if (!valid_dtype(dtype_w) || L <= 0) return 0;
  if (!dyn_pow2(group) || group < 16 || group > 256) return 0;
  if (L % group != 0 || L / kAwqV > 0x7FFFFFFF) return 0;
  return 1;
}

extern "C" int dmxq_awq_group_error(const void* w, int dtype_w, const float* s, float* d_out, void* wq_out, int64_t rows, int64_t L, int64_t group,
                                    int precision, int fraction, int clamp, int symmetric, int qmin, int qmax, int symmetric_qscheme, void* stream) {
  if (!valid_dtype(dtype_w) || rows < 0 || L < 0 || group < 1 || precision < 1 || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  if (rows > 0 && L > 0 && (!w || !s || !d_out)) return DMXQ_ERR_BAD_ARG;
  // what the kernel takes; everything else is the caller's chain (nothing launched)
  if (fraction != 0 || !clamp || precision > 22) return DMXQ_ERR_UNSUPPORTED;
  if (rows == 0 || L == 0) return DMXQ_OK;
  if (!dmxq_awq_class(dtype_w, L, group)) return DMXQ_ERR_UNSUPPORTED;
  if (!aligned16(w) || !aligned16(s) || !aligned16(d_out) || (wq_out && !aligned16(wq_out))) return DMXQ_ERR_UNSUPPORTED;
  if (rows > INT64_MAX / (L * 4)) return DMXQ_ERR_UNSUPPORTED;
  const FixedFmt x = make_fixed_fmt(precision, 0, 1, symmetric, DMXQ_ROUND_NEAREST, 0ull);
  const DynFmt f{x.t_min, x.t_max, qmin, qmax, symmetric_qscheme ? 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = rows * L;
  if (dtype_w == DMXQ_BF16) return awq_launch<DMXQ_BF16>(w, s, d_out, wq_out, n, L, group, f, st);
  if (dtype_w == DMXQ_F16) return awq_launch<DMXQ_F16>(w, s, d_out, wq_out, n, L, group, f, st);
  return awq_launch<DMXQ_F32>(w, s, d_out, wq_out, n, L, group, f, st);
}
