// csrc/fixedq.hpp — fixed point Q->DQ of one element (numerical/format.py:134-142 -> quant_cpu.cpp:127-209, sim_helper.cpp:5-38) and
// the host evaluation of its clamp limits, for every kernel that casts to a fixed point format: the elementwise kernels
// (elementwise.hip, fixed_multi.hip), SBFP's codes (blockfmt.hip), the dynamic cast's limits (dynamic_quant.hip), and through
// format_desc.hpp the GPTQ column kernels (gptq_cols.hpp), the fused rotation (hadamard.hip) and the error sweep (error_stats.hip).
#pragma once
#include <math.h>

#include "common.hpp"

namespace dmxq {

struct FixedFmt {
  int sigma, clamp, rounding;
  float t_min, t_max;
  uint64_t seed;
};
// sim_helper.cpp:5-12 fixed_min_max in its float/double mix, on the host: the ONE evaluation of t_min / t_max (fraction 0 is no special
// form: ldexp(1.0, 0) == 1.0)
inline FixedFmt make_fixed_fmt(int precision, int fraction, int clamp, int symmetric, int rounding, uint64_t seed) {
  const int sigma = -fraction;
  float t_min = (float)(-ldexp(1.0, precision - fraction - 1));
  const float t_max = (float)(-(double)t_min - ldexp(1.0, sigma));
  if (symmetric) t_min = (float)((double)t_min + ldexp(1.0, sigma));
  return FixedFmt{sigma, clamp ? 1 : 0, rounding, t_min, t_max, seed};
}

// sim_helper.cpp:14-21 round(a, r, sigma): ldexp; a1 = (float)(a + r); nearbyint((double)a1 - 0.5) (half-even);
// narrow to float; ldexp.  The fp32 add comes first — that is what makes 0.5 + 2^-24 round to 0 — and the
// double subtraction is exact.  It is reproduced in fp32 only (no f64 VALU, half rate on gfx950):
//   |a1| <  2^23 : a1 - 0.5f is exactly representable, rintf of it is the same integer;
//   |a1| >= 2^23 : a1 is an integer, a1 - 0.5 is an exact tie between a1-1 and a1 -> the even one: a1 unless it
//                  is odd (only possible below 2^24, where the mantissa LSB is the units bit), then a1 - 1.
// sim_helper.cpp:24-38 for up (ceil) / down (floor).
__device__ __forceinline__ float rne_minus_half(float a1) {
  const float mag = fabsf(a1);
  const float small = rintf(a1 - 0.5f);
  const bool odd = (f2u(a1) & 1u) != 0u && mag < 16777216.0f;
  const float big = odd ? a1 - 1.0f : a1;
  return mag >= 8388608.0f ? big : small;
}
__device__ __forceinline__ float fixed_q1(float a, const FixedFmt& f, float r) {
  a = ldexpf(a, -f.sigma);
  if (f.rounding == DMXQ_ROUND_UP) a = ceilf(a);
  else if (f.rounding == DMXQ_ROUND_DOWN) a = floorf(a);
  else a = rne_minus_half(a + r);
  a = ldexpf(a, f.sigma);
  if (f.clamp) a = a > f.t_max ? f.t_max : (a < f.t_min ? f.t_min : a);
  return a;
}
// the affine wrapper of numerical/cast.py:278-296 around the nearest cast: x / sc + z -> cast -> (q - z) * sc, the division IEEE
__device__ __forceinline__ float fixed_affine_q1(float x, float sc, float z, const FixedFmt& f) {
  return (fixed_q1(x / sc + z, f, 0.5f) - z) * sc;
}

}  // namespace dmxq
