// csrc/mxfp_math.hpp — the GENERAL path of an MXFP block (numerical/format.py:545-564): scale = 2^floor(log2 max|x|) / 2^(2^(e-1)),
// element = float(x / scale) * scale.  Used by blockfmt.hip (dmxq_mxfp_qdq, whose fast paths are bit-identical to this one by
// construction and fall back to it) and by hadamard.hip (dmxq_hadamard_qdq with DMXQ_GPTQ_MXFP, float32 input rules).
#pragma once
#include <math.h>

#include "floatq.hpp"

namespace dmxq {

// the constants of an element format with `exp_bits` exponent bits (host)
struct MxfpConsts {
  int bias;      // 2^(e-1) - 1
  int big_log2;  // 2^(e-1)
  float big;     // 2^(2^(e-1))
};
inline MxfpConsts make_mxfp_consts(int exp_bits) {
  const int big_log2 = 1 << (exp_bits - 1);
  return MxfpConsts{big_log2 - 1, big_log2, (float)ldexp(1.0, big_log2)};
}

// Does the reference's float32 log2 of m = 2^v (1 - j 2^-24), v != 0, round UP to the integer v?  (oracle/oracle.c oracle_floor_log2f:
// iff j <= jmax(g), g = -log2 of half the float32 gap at |v|.)  The one statement of the rule: normal and denormal maxima both ask it.
__device__ __forceinline__ bool mxfp_log2_rounds_up(int v, uint32_t j) {
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  const int c = 31 - __builtin_clz(a);
  const int g = (v > 0 && (a & (a - 1u)) == 0u) ? 25 - c : 24 - c;  // 17 .. 25
  // jmax = floor(2^24 (1 - 2^(-2^-g))): 88 44 22 11 | 5 2 1 | 0 0, as bytes of two constants
  const uint32_t jmax = g <= 20 ? ((0x0B162C58u >> (8 * (g - 17))) & 0xFFu) : (g <= 23 ? ((0x00010205u >> (8 * (g - 21))) & 0xFFu) : 0u);
  return j <= jmax;
}

// maxbits: fp32 bit pattern of the block's max|x|.  exact_exponent: the maximum came from a 16-bit tensor (see below).
__device__ __forceinline__ float mxfp_block_scale(uint32_t maxbits, int big_log2, float big, int exact_exponent) {
  // the reference evaluates 2^floor(log2 m) / 2^(2^(e-1)) in fp32 (format.py:551-555).  No libm: a float32 log2 within an ulp
  // of the truth crosses an integer only for m = 2^v (1 - j 2^-24) with j <= jmax(v) (the rule and its proof sketch are in
  // oracle/oracle.c oracle_floor_log2f; checked against torch.log2 for every exponent, fixtures tests/golden/boundaries.npz);
  // a maximum with at most 11 significant bits (bf16 / fp16 inputs) has j >= 2^13 and never does.
  int eb = (int)(maxbits >> 23);
  float scale;
  if (eb >= 1 && eb <= 254) {
    const uint32_t man = maxbits & 0x007FFFFFu;
    const int v = eb - 126;  // floor(log2 m) + 1
    if (!exact_exponent && man != 0u && v != 0 && mxfp_log2_rounds_up(v, 0x00800000u - man)) eb += 1;
    const int se = eb - big_log2;
    if (eb == 255) scale = INFINITY;                      // 2^128: the reference's fp32 power overflows too
    else if (se >= 1) scale = u2f((uint32_t)se << 23);
    else scale = ldexpf(1.0f, se - 127);                  // a denormal (or zero) scale, exact
  } else if (eb == 0 && maxbits != 0u) {
    // a denormal maximum k 2^-149 = 2^v (1 - j 2^-24) with v = bitlength(k) - 149 and j = (2^n - k) 2^(24 - n): the same rule, no libm
    // either.  The device's log2f is within an ulp but not correctly rounded: at k = 2^23 - 1 the reference's float32 log2 is exactly
    // -126 (j = 2 <= 44), the device's floor came out as -127 and the scale as half the reference's (tests/test_gpu_blockfmt.py).
    // k = 2^(n-1) has j = 2^23: never rounds up.
    const int n = 32 - __builtin_clz(maxbits);            // 1 .. 23
    const int v = n - 149;                                // -148 .. -126
    const uint32_t j = ((1u << n) - maxbits) << (24 - n);
    const int fl = v - 1 + (mxfp_log2_rounds_up(v, j) ? 1 : 0);   // (g = 18 or 17 here: jmax 44 or 88)
    scale = ldexpf(1.0f, fl - big_log2);                  // 2^fl / big: a denormal, or zero (the reference's quotient rounds the same way)
  } else {
    scale = exp2f(floorf(log2f(u2f(maxbits)))) / big;     // zero (the caller's `zero`), Inf, NaN maxima
  }
  return scale;
}

// one element of a block with that scale; zero: the block's maximum is 0 (the elements keep their signs)
__device__ __forceinline__ float mxfp_q1(float x, float scale, bool zero, int man, int exp_bits, int bias) {
  if (zero) return x * 0.0f;
  return float_q1<DMXQ_ROUND_NEAREST>(x / scale, FloatFmt{man, exp_bits, bias, 0, 0, DMXQ_ROUND_NEAREST, 0ull}, 0u) * scale;
}

}  // namespace dmxq
