// csrc/dynamic_geom.hpp — the launch geometry of the dynamic casts, shared by the integer cast (dynamic_quant.hip) and the scaled float
// cast (dynamic_float.hip): segments inside a wave, a wave per row, a workgroup per row -- and, for the float cast only, square tiles.
#pragma once
#include "common.hpp"

namespace dmxq {

constexpr int kDynThreads = 256;
constexpr int kDynMaxRow = 16384;

inline bool dyn_pow2(int64_t v) { return v >= 1 && (v & (v - 1)) == 0; }

// The launch geometry of a segment length: THE rule, used by the launchers and handed out through dmxq_dynamic_class /
// dmxq_dynamic_float_class (the front end's ops.dynamic_class, by which the default route and the measurement tables name a geometry).
// V: elements per 16-byte vector.
inline int dyn_class(int64_t S, int V, bool whole_rows) {
  if (S < 1 || S % V != 0 || S > kDynMaxRow) return DMXQ_DYN_NONE;
  if (dyn_pow2(S) && S >= 16 && S <= 256) return DMXQ_DYN_GROUP;
  if (!whole_rows) return DMXQ_DYN_NONE;   // (a group that is no such power of two: a wave per short segment would idle most lanes)
  const int64_t nv = S / V;
  if (nv < kWave) return DMXQ_DYN_SHORT_ROW;               // a wave per row with idle lanes (measured apart)
  return nv <= 16 * kWave ? DMXQ_DYN_WAVE_ROW : DMXQ_DYN_BLOCK_ROW;
}

// a g x g tile of the last two dims: 32, 64 or 128 (a tile's 16-byte vectors stay in the registers of a wave or a workgroup)
inline int dyn_tile_class(int64_t g) { return (g == 32 || g == 64 || g == 128) ? DMXQ_DYN_TILE : DMXQ_DYN_NONE; }

}  // namespace dmxq
