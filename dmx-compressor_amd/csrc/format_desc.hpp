// csrc/format_desc.hpp — host side: a dmxq_gptq_format (include/dmxq.h) as the pieces the device-side leaves take, with the range checks
// every entry point that accepts the descriptor shares (dmxq_gptq_block, dmxq_gptq_block_dynamic, dmxq_cast_error, dmxq_hadamard_qdq).
// What differs between them stays with them, in their own order: which kinds they accept at all, the block_size rules, per_row, null
// scales.  Nearest rounding throughout (the descriptor has no rounding field).
#pragma once
#include "fixedq.hpp"
#include "floatq.hpp"
#include "mxfp_math.hpp"

namespace dmxq {

struct FormatDesc {
  int wl, asym;        // BFP: precision, "(_N)"
  FloatFmt f;          // FLOAT
  FixedFmt x;          // FIXED
  int man, exp_bits;   // MXFP: the element format's mantissa and exponent bits,
  MxfpConsts k;        //       and the constants of its exponent range
};

// DMXQ_OK, or DMXQ_ERR_UNSUPPORTED for a field outside what the casts take; g.kind is one of the four kinds (the caller's check)
inline int format_desc(const dmxq_gptq_format& g, FormatDesc* d) {
  *d = FormatDesc{};
  if (g.kind == DMXQ_GPTQ_BFP) {
    if (g.precision < 2 || g.precision > 22) return DMXQ_ERR_UNSUPPORTED;
    d->wl = g.precision;
    d->asym = g.symmetric == 0;
  } else if (g.kind == DMXQ_GPTQ_FIXED) {
    if (g.precision < 1 || g.precision > 24) return DMXQ_ERR_UNSUPPORTED;
    d->x = make_fixed_fmt(g.precision, g.fraction, g.clamp, g.symmetric, DMXQ_ROUND_NEAREST, 0ull);
  } else {
    if (g.exp_bits < 1 || g.exp_bits > 8 || g.man_bits < 0 || g.man_bits > 22) return DMXQ_ERR_UNSUPPORTED;
    if (g.kind == DMXQ_GPTQ_FLOAT) {
      d->f = FloatFmt{g.man_bits, g.exp_bits, g.exp_bias, g.flush_subnormal ? 1 : 0, g.unsigned_abs ? 1 : 0, DMXQ_ROUND_NEAREST, 0ull};
    } else {   // MXFP: dmxq_mxfp_qdq's element format, field by field
      d->man = g.man_bits;
      d->exp_bits = g.exp_bits;
      d->k = make_mxfp_consts(g.exp_bits);
    }
  }
  return DMXQ_OK;
}

}  // namespace dmxq
