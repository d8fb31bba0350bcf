// csrc/reduce_common.hpp -- pieces of the calibration reductions shared by csrc/reduce.hip (dmxq_group_minmax, dmxq_histc) and
// csrc/hist_observer.hip (the device HistogramObserver): raw 16-byte loads widened to fp32, and torch.histc's bin rule.
#pragma once
#include <math.h>

#include "common.hpp"

namespace dmxq {

// 8 consecutive elements, compile-time dtype: the RAW 16-byte vectors first (so that a batch of loads is issued back to
// back), widened afterwards.  (reduce.hip's runtime-dtype load8_rt wraps every load in a dtype branch whose conversion
// waits for that load: one access in flight per lane.)
template <int DT>
struct Raw8 {
  u32x4 a, b;  // b only for fp32
};
template <int DT>
__device__ __forceinline__ Raw8<DT> load8_raw(const void* p, int64_t e) {
  Raw8<DT> r;
  // non-temporal: the reductions read their operand exactly once
  if (DT == DMXQ_F32) { r.a = __builtin_nontemporal_load((const u32x4*)((const float*)p + e)); r.b = __builtin_nontemporal_load((const u32x4*)((const float*)p + e + 4)); }
  else { r.a = __builtin_nontemporal_load((const u32x4*)((const uint16_t*)p + e)); r.b = r.a; }
  return r;
}
template <int DT>
__device__ __forceinline__ void widen8(const Raw8<DT>& r, float (&v)[8]) {
  if (DT == DMXQ_F32) {
#pragma unroll
    for (int j = 0; j < 4; j++) { v[j] = u2f(r.a[j]); v[4 + j] = u2f(r.b[j]); }
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (DT == DMXQ_BF16) { v[2 * j] = u2f(r.a[j] << 16); v[2 * j + 1] = u2f(r.a[j] & 0xFFFF0000u); }
      else { v[2 * j] = half_lo(r.a[j]); v[2 * j + 1] = half_hi(r.a[j]); }
    }
  }
}

constexpr int kHistThreads = 1024;
constexpr int kHistMaxBins = 8192;  // 32 KiB of LDS counters
// FAST: width in [2^-20, 2^20] (checked by the caller: recip_ok): the quotient comes from div_for_clamped_int (common.hpp), which IS the IEEE
// quotient for 2^-100 <= |n| <= 2^100; n = (v - lo) * bins is below 2^34 for an in-range v, and a smaller |n| truncates to bin 0
// whatever its last bit is.  3 FMA-class operations instead of the ~14 of v_div_scale/fmas/fixup per element.
// (Tried and measured slower on the same box, profiles/r02_histc_variants.txt: a branch-free add of 0 for out-of-range elements;
// 2 / 4 / 8 interleaved copies of the counters against same-bin collisions; 128 or 512 workgroups.)
template <bool FAST>
__device__ __forceinline__ void hist_add(uint32_t* s, float v, float lo, float hi, float fb, const Recip& width, int bins) {
  if (v >= lo && v <= hi) {
    const float n = (v - lo) * fb;
    int pos = (int)(FAST ? div_for_clamped_int(n, width) : n / width.d);
    pos = pos < bins ? pos : bins - 1;
    atomicAdd(&s[pos], 1u);
  }
}

// Running minimum and maximum of float VALUES with dmxq_group_minmax's NaN rule, for the kernels that derive a segment's scale themselves
// (csrc/dynamic_quant.hip, csrc/gptq_cols.hpp): fminf / fmaxf drop a NaN operand, so a NaN is noticed on the |x| bit patterns instead
// (above +Inf's pattern <=> a NaN was seen) and makes BOTH extrema NaN (torch.amin / amax propagate it; reduce.hip nan_to_both), which
// qparams_one's fminf / fmaxf then drop in turn.
struct FloatExtrema {
  float lo, hi;
  uint32_t am;   // max of the |x| bit patterns
  __device__ __forceinline__ void init() { lo = INFINITY; hi = -INFINITY; am = 0u; }
  __device__ __forceinline__ void add(float x) { lo = fminf(lo, x); hi = fmaxf(hi, x); am = max(am, f2u(x) & 0x7FFFFFFFu); }
  __device__ __forceinline__ bool nan() const { return am > 0x7F800000u; }
  __device__ __forceinline__ float mn() const { return nan() ? u2f(0xFFC00000u) : lo; }   // (-NaN, +NaN): they win every later min / max
  __device__ __forceinline__ float mx() const { return nan() ? u2f(0x7FC00000u) : hi; }
};

// ORDER-PRESERVING KEYS of float values: key(f) = bits ^ (sign ? ~0 : 1 << 31) orders like the floats as an unsigned integer and puts
// -NaN below -Inf and +NaN above +Inf, so a minimum / maximum across lanes is an integer one (DPP, shuffles, LDS) and a (-NaN, +NaN)
// pair wins it.  csrc/reduce.hip (dmxq_group_minmax) and csrc/dynamic_quant.hip (a segment's extrema).
__device__ __forceinline__ uint32_t fkey(float f) { const uint32_t b = f2u(f); return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u); }
__device__ __forceinline__ float fkey_inv(uint32_t k) { return u2f(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu)); }

// (min, max) -> (scale, zero_point) of one group (numerical/observer.py:59-115 _calculate_qparams): dmxq_qparams and the
// HistogramObserver's search kernel (csrc/hist_observer.hip)
__device__ __forceinline__ void qparams_one(float mn, float mx, int qmin, int qmax, int sym, float& scale, int64_t& zp) {
  const float eps = 1.1920928955078125e-07f;  // torch.finfo(torch.float32).eps (observer.py:37)
  const float min_neg = fminf(mn, 0.0f);
  const float max_pos = fmaxf(mx, 0.0f);
  if (sym) {
    const float m = fmaxf(-min_neg, max_pos);
    scale = fmaxf(m / ((float)(qmax - qmin) / 2.0f), eps);
    zp = 0;
  } else {
    const float s = fmaxf((max_pos - min_neg) / (float)(qmax - qmin), eps);
    float z = (float)qmin - rintf(min_neg / s);
    z = fminf(fmaxf(z, (float)qmin), (float)qmax);
    scale = s;
    zp = (int64_t)z;
  }
}
}  // namespace dmxq
