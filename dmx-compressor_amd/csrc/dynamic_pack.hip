// csrc/dynamic_pack.hip — the dynamic per-token / per-group integer cast as PACKED operands (include/dmxq.h dmxq_dynamic_fixed_pack;
// DESIGN.md §8 "Integer matmul"): int8 codes + one fp32 scale per segment in ONE launch, what csrc/int_matmul.hip multiplies.
//
// Defined for the symmetric scheme (zero point 0) and the clamped nearest-rounding format XP[p,0], 2 <= p <= 8, by
// dmxq_dynamic_fixed_qdq(symmetric_qscheme = 1) on the same segments:
//   * scale[s] is the value that entry writes to scale_out, bit for bit: the SAME code computes it (dynamic_quant.hpp DynExt,
//     dyn_group_minmax, DynSeg::setup -> qparams_one), NaN / Inf rule included (a NaN anywhere: scale eps; an Inf: scale Inf);
//   * code = the clamped integer v of dyn_q_of<true>(x / scale): v = clamp(rintf((q + 0.5f) - 0.5f), t_min, t_max), the value the cast
//     multiplies by the scale -- so codes.float() * scale IS the cast of a float32 tensor (a -0 result of the cast is +0 here: int8
//     has one zero).  The quotient is the reciprocal form (common.hpp div_for_clamped_int: the same clamped integer as the IEEE
//     division) while recip_ok(scale) holds for every segment of the wave, the division otherwise.
//   * an element whose quotient is NaN (a NaN element; Inf in a segment whose scale is Inf) packs to code 0; every other element of a
//     segment with a NaN (scale eps) or an Inf (scale Inf: finite x / Inf = 0) packs to what the clamp gives: +-t_max / 0.
//
// Geometry.  A lane owns a UNIT of two 16-byte input vectors (16 sixteen-bit or 8 fp32 elements), held raw between the extrema pass
// and the cast, and stores its codes as ONE 16-byte (8-byte for fp32 input) vector; a segment's scale leaves as one dword store of
// its first lane.  Segments are dynamic_geom.hpp dyn_class's with the unit as the vector: powers of two 16 .. 256 inside a wave
// (S / unit adjacent lanes, DPP / xor-shuffle extrema), or whole rows of any multiple of the unit up to 16384 -- a wave per row up to
// 8 units per lane, four rows per workgroup; a 256-lane workgroup per row above that.  Lanes past the end re-read the last unit, meet
// only each other and store nothing.  One read of x, 1 (0.5 / 0.25) byte written per element, no workspace: capturable.
#include <math.h>

#include "dynamic_geom.hpp"
#include "dynamic_quant.hpp"

namespace dmxq {
namespace {

inline int dynp_class(int64_t S, int E, bool whole_rows) {
  const int c = dyn_class(S, E, whole_rows);
  return (c == DMXQ_DYN_WAVE_ROW && S / E > 8 * kWave) ? DMXQ_DYN_BLOCK_ROW : c;   // (8 units = 16 raw vectors per lane at most)
}

// a lane's unit: two adjacent raw vectors
template <int DT>
struct PackUnit {
  static constexpr int V = 16 / Elem<DT>::bytes, E = 2 * V, CW = E / 4;   // elements per vector / per unit; code dwords per unit
  u32x4 r[2];
  __device__ __forceinline__ void load(const void* in, int64_t unit) {
    r[0] = load_raw16<true>(in, unit * 32);
    r[1] = load_raw16<true>(in, unit * 32 + 16);
  }
  __device__ __forceinline__ void add(DynExt& e) const {
    e.add<DT, V>(r[0]);
    e.add<DT, V>(r[1]);
  }
  // the unit's E codes -> codes[unit * E ..), one vector store
  __device__ __forceinline__ void store(int8_t* codes, int64_t unit, const DynSeg& s, bool all_fast, const DynFmt& f) const {
    uint32_t w[CW];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      float x[V];
      widen<DT, V>(r[h], x);
#pragma unroll
      for (int k = 0; k < V; k += 4) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const float q = all_fast ? div_for_clamped_int(x[k + b], Recip{s.sc, s.rs}) : x[k + b] / s.sc;
          float v = rintf((q + 0.5f) - 0.5f);                                    // dyn_q_of<true>'s integer
          v = v > f.t_max ? f.t_max : (v < f.t_min ? f.t_min : v);
          const int c = v == v ? (int)v : 0;                                     // NaN quotient: code 0
          word |= ((uint32_t)c & 0xFFu) << (8 * b);
        }
        w[(h * V + k) / 4] = word;
      }
    }
    if constexpr (CW == 4) *(u32x4*)(codes + unit * E) = u32x4{w[0], w[1], w[2], w[3]};
    else *(u32x2*)(codes + unit * E) = u32x2{w[0], w[1]};
  }
};

// segments of `lanes` adjacent lanes (1 .. 32), one unit per lane; nunit = n_segments * lanes
template <int DT>
__global__ __launch_bounds__(kDynThreads) void dynp_group_kernel(const void* __restrict__ in, int8_t* __restrict__ codes,
                                                                float* __restrict__ scale, int64_t nunit, int lanes, int lanes_log2,
                                                                const DynFmt f) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kDynThreads + threadIdx.x;
  PackUnit<DT> u;
  u.load(in, i < nunit ? i : nunit - 1);
  DynExt e;
  e.init();
  u.add(e);
  uint32_t klo, khi;
  e.keys(klo, khi);
  dyn_group_minmax(klo, khi, lanes);
  DynSeg s;
  s.setup(klo, khi, f);
  const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(s.sc)) == 0ull;
  if (i < nunit) {
    u.store(codes, i, s, all_fast, f);
    if ((lane & (lanes - 1)) == 0) scale[i >> lanes_log2] = s.sc;
  }
}

// rows of nu units; WAVES = 1: a wave per row, four rows per workgroup; WAVES = 4: the workgroup's row.  U x 64 x WAVES >= nu.
template <int DT, int U, int WAVES>
__global__ __launch_bounds__(kDynThreads) void dynp_rows_kernel(const void* __restrict__ in, int8_t* __restrict__ codes,
                                                               float* __restrict__ scale, int64_t rows, int nu, const DynFmt f) {
  constexpr int T = kWave * WAVES, RPB = kDynThreads / T;
  const int t = threadIdx.x & (T - 1);
  int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / T;
  const bool row_ok = row < rows;   // (wave-uniform; a wave past the last row re-reads it and stores nothing)
  row = row_ok ? row : rows - 1;
  const int64_t u0 = row * nu;
  PackUnit<DT> u[U];
  DynExt e;
  e.init();
#pragma unroll
  for (int k = 0; k < U; k++) {
    const int v = t + k * T;
    u[k].load(in, u0 + (v < nu ? v : nu - 1));   // clamped: a repeated unit cannot change a min / max
  }
#pragma unroll
  for (int k = 0; k < U; k++) u[k].add(e);
  uint32_t klo, khi;
  e.keys(klo, khi);
  dyn_group_minmax(klo, khi, kWave);
  if constexpr (WAVES > 1) {
    __shared__ uint32_t s_lo[WAVES], s_hi[WAVES];
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) { s_lo[w] = klo; s_hi[w] = khi; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WAVES; i++) { klo = min(klo, s_lo[i]); khi = max(khi, s_hi[i]); }
  }
  DynSeg s;
  s.setup(klo, khi, f);
  const bool all_fast = recip_ok(s.sc);   // one segment per wave: wave-uniform
  if (t == 0 && row_ok) scale[row] = s.sc;
#pragma unroll
  for (int k = 0; k < U; k++) {
    const int v = t + k * T;
    if (v < nu && row_ok) u[k].store(codes, u0 + v, s, all_fast, f);
  }
}

template <int DT>
int dynp_launch(const void* in, int8_t* codes, float* scale, int64_t n_segments, int64_t S, bool whole_rows, const DynFmt& f, hipStream_t s) {
  constexpr int E = PackUnit<DT>::E;
  const int cls = dynp_class(S, E, whole_rows);
  if (cls == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  const int64_t nu = S / E;
  if (cls == DMXQ_DYN_GROUP) {
    int l2 = 0;
    while ((1 << l2) < (int)nu) l2++;
    const int64_t nunit = n_segments * nu;
    const int64_t grid = (nunit + kDynThreads - 1) / kDynThreads;
    if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
    DMXQ_LAUNCH((dynp_group_kernel<DT>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, codes, scale, nunit, (int)nu, l2, f);
    return launch_status();
  }
  const bool wave_row = cls != DMXQ_DYN_BLOCK_ROW;
  const int64_t rpb = wave_row ? kDynThreads / kWave : 1;
  const int64_t grid = (n_segments + rpb - 1) / rpb;
  if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  const int64_t T = wave_row ? kWave : kDynThreads, per_lane = (nu + T - 1) / T;   // <= 8 in either form
#define DMXQ_DYNP_ROWS(U_, W_) \
  DMXQ_LAUNCH((dynp_rows_kernel<DT, U_, W_>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, codes, scale, n_segments, (int)nu, f)
  if (wave_row) {
    if (per_lane <= 1) DMXQ_DYNP_ROWS(1, 1);
    else if (per_lane <= 2) DMXQ_DYNP_ROWS(2, 1);
    else if (per_lane <= 4) DMXQ_DYNP_ROWS(4, 1);
    else DMXQ_DYNP_ROWS(8, 1);
  } else {
    if (per_lane <= 4) DMXQ_DYNP_ROWS(4, 4);
    else DMXQ_DYNP_ROWS(8, 4);
  }
#undef DMXQ_DYNP_ROWS
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_dynamic_pack_class(int dtype, int64_t segment, int whole_rows) {
  if (!valid_dtype(dtype)) return DMXQ_DYN_NONE;
  return dynp_class(segment, dtype == DMXQ_F32 ? 8 : 16, whole_rows != 0);
}

extern "C" int dmxq_dynamic_fixed_pack(const void* in, int dtype_in, int8_t* codes, float* scale, int64_t n_segments, int64_t segment,
                                       int whole_rows, int precision, int symmetric, int qmin, int qmax, void* stream) {
  if (!valid_dtype(dtype_in) || n_segments < 0 || segment < 0 || precision < 1 || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!in || !codes || !scale)) return DMXQ_ERR_BAD_ARG;
  if (precision < 2 || precision > 8) return DMXQ_ERR_UNSUPPORTED;   // int8 codes
  if (dmxq_dynamic_pack_class(dtype_in, segment, whole_rows) == DMXQ_DYN_NONE && segment > 0) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments == 0 || segment == 0) return DMXQ_OK;
  if (!aligned16(in) || !aligned16(codes) || (reinterpret_cast<uintptr_t>(scale) & 3u)) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments > INT64_MAX / (segment * 4)) return DMXQ_ERR_UNSUPPORTED;
  const FixedFmt x = make_fixed_fmt(precision, 0, 1, symmetric, DMXQ_ROUND_NEAREST, 0ull);
  const DynFmt f{x.t_min, x.t_max, qmin, qmax, 1};
  hipStream_t s = (hipStream_t)stream;
  if (dtype_in == DMXQ_BF16) return dynp_launch<DMXQ_BF16>(in, codes, scale, n_segments, segment, whole_rows != 0, f, s);
  if (dtype_in == DMXQ_F16) return dynp_launch<DMXQ_F16>(in, codes, scale, n_segments, segment, whole_rows != 0, f, s);
  return dynp_launch<DMXQ_F32>(in, codes, scale, n_segments, segment, whole_rows != 0, f, s);
}
