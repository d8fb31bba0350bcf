// csrc/awq_clip.hip — AWQ weight clipping (Lin et al., 2023; AutoAWQ's clip search) in ONE launch (include/dmxq.h dmxq_awq_clip;
// DESIGN.md §8 "AWQ clipping", whose text is the contract).  Not in the reference.
//
// For every group of g consecutive columns of every row of w[rows, L] (dtype T) and every candidate ratio r_i (r_0 = 1):
//   a   = max |W|                                  the group's extrema, dmxq_group_minmax's NaN rule          (DynExt, dyn_group_minmax)
//   c_i = fp32(T(a * r_i))                         one fp32 multiply, one rounding to T
//   v   = W > c_i ? c_i : (W < -c_i ? -c_i : W)    selects: in-range values keep their bits
//   q   = dmxq_dynamic_fixed_qdq(v, group)         the cast of csrc/dynamic_quant.hip, in T                   (DynSeg, dyn_cast_vec)
//   d   = fp32(q) - W
//   t_j = sum_l blocks[k][j][l] * d_l              in index order from the first product, every product and sum its own fp32 operation
//   loss_i = tsum_j(d_j * t_j)                     the adjacent-pair tree                                     (hqq_vec_sum, hqq_group_sum)
// and the group keeps the lowest i among the minimal finite losses (0 when none is finite); y = T(v of that i).  A group whose a is
// not finite and positive keeps its own bits, i = 0, clip = a and NaN losses.  The build passes -ffp-contract=off.
//
// Geometry.  A workgroup owns ONE column group k and a slab of rows: it stages blocks[k] TRANSPOSED in LDS once (Bt[l][j], g x g floats:
// 1 KiB at g = 16, the whole 64 KiB a kernel gets without an opt-in at g = 128) and loops over its rows.  csrc/awq.hip's layout: a lane
// owns four consecutive elements, a group is g / 4 adjacent lanes (4 .. 32), a wave holds 256 / g rows of the column group and the four
// waves 1024 / g.  For its own four j a lane runs the loop over l in order: the four d of source lane m reach it by four lane exchanges
// (no LDS: g = 128 stays inside 64 KiB), and Bt[4 m + c][4 sub .. 4 sub + 3] is one 16-byte LDS read -- the lanes of a group read
// consecutive 16 bytes, the other rows of the wave the same addresses (a broadcast): conflict-free.  The candidates run in a loop that
// keeps only the best loss and index; the winning clamp is formed again for the store.
// Lanes past the last row re-read it, take part in every stage (a group's lanes share their row, so they meet only each other) and
// store nothing.  No workspace, no host synchronisation, no float atomics: capturable.
#include <math.h>

#include "awq_lane4.hpp"
#include "dynamic_geom.hpp"
#include "dynamic_quant.hpp"

namespace dmxq {
namespace {

constexpr int kClipMaxRatios = 32;
constexpr int kClipBlocksPerCu = 4;   // the grid's cap; the rest of the rows by the loop over passes

template <int DT, int GS>
__global__ __launch_bounds__(kDynThreads) void awq_clip_kernel(const void* w /* may be y_out: in place */, const float* __restrict__ blocks,
                                                              const float* __restrict__ ratios, int n_ratios, void* y_out,
                                                              uint8_t* __restrict__ best_out, float* __restrict__ clip_out,
                                                              float* __restrict__ losses_out, int64_t rows, int64_t vecs_per_row, int64_t G,
                                                              int64_t passes, const DynFmt f) {
  constexpr int V = kAwqV;
  constexpr int LANES = GS / V;                   // lanes per group: 4 .. 32
  constexpr int RPW = kWave / LANES;              // rows per wave
  constexpr int RPB = RPW * (kDynThreads / kWave);   // rows per pass of the workgroup
  __shared__ float Bt[GS * GS];                   // Bt[l * GS + j] = blocks[k][j][l]
  const int64_t k = blockIdx.x;
  {
    const float* src = blocks + k * (int64_t)(GS * GS);
    for (int e = threadIdx.x; e < GS * GS; e += kDynThreads) Bt[(e % GS) * GS + e / GS] = src[e];
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LANES - 1);
  const int first = lane - sub;                   // the group's first lane
  const int row_in_pass = (threadIdx.x / kWave) * RPW + lane / LANES;
  const f32x4* bt4 = (const f32x4*)Bt + sub;      // + l * (GS / 4): Bt[l][4 sub .. 4 sub + 3]
  for (int64_t p = blockIdx.y; p < passes; p += gridDim.y) {   // (uniform over the workgroup)
    const int64_t row = p * RPB + row_in_pass;
    const bool ok = row < rows;
    const int64_t vec = (ok ? row : rows - 1) * vecs_per_row + k * LANES + sub;
    const u32x4 raw = awq_load4<DT>(w, vec);
    float x[V];
    awq_widen4<DT>(raw, x);
    // step 1: a = max |W|, NaN if any element is
    float a;
    {
      DynExt e;
      e.init();
#pragma unroll
      for (int j = 0; j < V; j++) e.FloatExtrema::add(x[j]);
      uint32_t klo, khi;
      e.keys(klo, khi);
      dyn_group_minmax(klo, khi, LANES);
      const float mn = fkey_inv(klo), mx = fkey_inv(khi);
      a = mn != mn ? mx : fmaxf(fabsf(mn), fabsf(mx));
    }
    const bool ordinary = fabsf(a) < INFINITY && a > 0.0f;
    const int64_t grp = row * G + k;
    float best_loss = INFINITY, best_c = a;
    int best = 0;
    for (int i = 0; i < n_ratios; i++) {
      // step 3
      float c4[V] = {a * ratios[i], 0.0f, 0.0f, 0.0f};
      awq_round4<DT>(c4);
      const float c = c4[0];
      float v[V], q[V], d[V];
#pragma unroll
      for (int j = 0; j < V; j++) v[j] = x[j] > c ? c : (x[j] < -c ? -c : x[j]);
      DynExt e;
      e.init();
#pragma unroll
      for (int j = 0; j < V; j++) e.FloatExtrema::add(v[j]);
      uint32_t klo, khi;
      e.keys(klo, khi);
      dyn_group_minmax(klo, khi, LANES);
      DynSeg g;
      g.setup(klo, khi, f);
      const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(g.sc)) == 0ull;
      const bool all_zp0 = __builtin_amdgcn_ballot_w64(g.z != 0.0f) == 0ull;
      dyn_cast_vec<V>(v, q, g, all_fast, all_zp0, f);
      awq_round4<DT>(q);
#pragma unroll
      for (int j = 0; j < V; j++) d[j] = q[j] - x[j];
      // step 4: t_j for this lane's four j, l in order; -0 + x is x for every x, so the sum starts from the first product
      float t[V] = {-0.0f, -0.0f, -0.0f, -0.0f};
#pragma unroll 4
      for (int m = 0; m < LANES; m++) {
        float dl[V];
#pragma unroll
        for (int cc = 0; cc < V; cc++) dl[cc] = __shfl(d[cc], first + m);
#pragma unroll
        for (int cc = 0; cc < V; cc++) {
          const f32x4 b = bt4[(m * V + cc) * (GS / 4)];
          t[0] = t[0] + b.x * dl[cc];
          t[1] = t[1] + b.y * dl[cc];
          t[2] = t[2] + b.z * dl[cc];
          t[3] = t[3] + b.w * dl[cc];
        }
      }
#pragma unroll
      for (int j = 0; j < V; j++) t[j] = d[j] * t[j];
      const float loss = hqq_group_sum(hqq_vec_sum<V>(t), LANES);
      // step 5 (ordered comparisons: a NaN loss is never kept)
      const bool better = ordinary && fabsf(loss) < INFINITY && loss < best_loss;
      best_loss = better ? loss : best_loss;
      best_c = better ? c : best_c;
      best = better ? i : best;
      if (ok && sub == 0 && losses_out) losses_out[grp * n_ratios + i] = ordinary ? loss : u2f(0x7FC00000u);
    }
    // step 6: the winning clamp again; a group that is not ordinary keeps its bits
    if (ok) {
      u32x4 r = raw;
      if (ordinary) {
        float v[V];
#pragma unroll
        for (int j = 0; j < V; j++) v[j] = x[j] > best_c ? best_c : (x[j] < -best_c ? -best_c : x[j]);
        r = awq_round4<DT>(v);
      }
      awq_store4<DT>(y_out, row * vecs_per_row + k * LANES + sub, r);
      if (sub == 0) {
        if (best_out) best_out[grp] = (uint8_t)best;
        if (clip_out) clip_out[grp] = best_c;
      }
    }
  }
}

template <int DT, int GS>
int awq_clip_launch_g(const void* w, const float* blocks, const float* ratios, int n, void* y, uint8_t* best, float* clip, float* losses,
                      int64_t rows, int64_t L, const DynFmt& f, hipStream_t st) {
  constexpr int RPB = (kWave / (GS / kAwqV)) * (kDynThreads / kWave);
  const int64_t G = L / GS;
  const int64_t passes = (rows + RPB - 1) / RPB;
  int64_t slabs = ((int64_t)plan_cus() * kClipBlocksPerCu + G - 1) / G;   // workgroups per column group
  slabs = slabs < passes ? slabs : passes;
  if (G > 0x7FFFFFFF || slabs > 65535) return DMXQ_ERR_UNSUPPORTED;
  DMXQ_LAUNCH((awq_clip_kernel<DT, GS>), dim3((unsigned)G, (unsigned)slabs), dim3(kDynThreads), 0, st, w, blocks, ratios, n, y, best, clip, losses,
              rows, L / kAwqV, G, passes, f);
  return launch_status();
}

template <int DT>
int awq_clip_launch(const void* w, const float* blocks, const float* ratios, int n, void* y, uint8_t* best, float* clip, float* losses,
                    int64_t rows, int64_t L, int64_t group, const DynFmt& f, hipStream_t st) {
  switch (group) {
    case 16: return awq_clip_launch_g<DT, 16>(w, blocks, ratios, n, y, best, clip, losses, rows, L, f, st);
    case 32: return awq_clip_launch_g<DT, 32>(w, blocks, ratios, n, y, best, clip, losses, rows, L, f, st);
    case 64: return awq_clip_launch_g<DT, 64>(w, blocks, ratios, n, y, best, clip, losses, rows, L, f, st);
    case 128: return awq_clip_launch_g<DT, 128>(w, blocks, ratios, n, y, best, clip, losses, rows, L, f, st);
  }
  return DMXQ_ERR_UNSUPPORTED;
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

// 1: dmxq_awq_clip takes rows of L elements of dtype_w with groups of `group` (given 16-byte aligned pointers), 0: it refuses them
extern "C" int dmxq_awq_clip_class(int dtype_w, int64_t L, int64_t group) {
  if (!valid_dtype(dtype_w) || L <= 0) return 0;
  if (group != 16 && group != 32 && group != 64 && group != 128) return 0;
  if (L % group != 0 || L / group > 0x7FFFFFFF) return 0;
  return 1;
}

extern "C" int dmxq_awq_clip(const void* w, int dtype_w, const float* blocks, const float* ratios, int n_ratios, void* y_out, uint8_t* best_out,
                             float* clip_out, float* losses_out, int64_t rows, int64_t L, int64_t group, int precision, int fraction, int clamp,
                             int symmetric, int qmin, int qmax, int symmetric_qscheme, void* stream) {
  if (!valid_dtype(dtype_w) || rows < 0 || L < 0 || group < 1 || precision < 1 || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  if (n_ratios < 1 || n_ratios > kClipMaxRatios || !ratios) return DMXQ_ERR_BAD_ARG;
  if (rows > 0 && L > 0 && (!w || !blocks || !y_out)) return DMXQ_ERR_BAD_ARG;
  // what the kernel takes; everything else is the caller's chain (nothing launched)
  if (fraction != 0 || !clamp || precision > 22) return DMXQ_ERR_UNSUPPORTED;
  if (rows == 0 || L == 0) return DMXQ_OK;
  if (!dmxq_awq_clip_class(dtype_w, L, group)) return DMXQ_ERR_UNSUPPORTED;
  if (!aligned16(w) || !aligned16(blocks) || !aligned16(ratios) || !aligned16(y_out) || (best_out && !aligned16(best_out)) ||
      (clip_out && !aligned16(clip_out)) || (losses_out && !aligned16(losses_out)))
    return DMXQ_ERR_UNSUPPORTED;
  if (rows > INT64_MAX / (L * 4) || rows * (L / group) > INT64_MAX / (4 * kClipMaxRatios)) return DMXQ_ERR_UNSUPPORTED;
  const FixedFmt x = make_fixed_fmt(precision, 0, 1, symmetric, DMXQ_ROUND_NEAREST, 0ull);
  const DynFmt f{x.t_min, x.t_max, qmin, qmax, symmetric_qscheme ? 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  if (dtype_w == DMXQ_BF16) return awq_clip_launch<DMXQ_BF16>(w, blocks, ratios, n_ratios, y_out, best_out, clip_out, losses_out, rows, L, group, f, st);
  if (dtype_w == DMXQ_F16) return awq_clip_launch<DMXQ_F16>(w, blocks, ratios, n_ratios, y_out, best_out, clip_out, losses_out, rows, L, group, f, st);
  return awq_clip_launch<DMXQ_F32>(w, blocks, ratios, n_ratios, y_out, best_out, clip_out, losses_out, rows, L, group, f, st);
}
