// csrc/hadamard_row.hip — orthonormal Hadamard rotation of a WHOLE row, fused with the dynamic per-token / per-group integer cast
// (include/dmxq.h dmxq_hadamard_row_qdq; DESIGN.md §8 "Full-row Hadamard rotation").  Not in the reference: the online rotation of
// QuaRot / SpinQuant over the hidden or intermediate dimension (4096 .. 28672 / 2), which csrc/hadamard.hip cannot serve -- its block
// lives in one wave, 256 elements at most -- and which users spell as a dense [n, n] matmul followed by the three-launch dynamic chain.
//
// Arithmetic (the contract; tests/_hadamard_row_ref.py restates it on the CPU).  A row of n = m 2^k elements, m in {1, 12, 20, 28},
// 512 <= n <= 16384, widened to fp32 (exact); element i = a 2^k + b; the matrix is H_m (x) H_{2^k}:
//   1. the k butterfly stages, strides s = 1, 2, .., 2^(k-1) ASCENDING, inside each of the m chunks of 2^k elements: for every b with
//      bit s clear  v[b], v[b+s] = v[b] + v[b+s], v[b] - v[b+s]  (old values on the right, lower index minus upper, each ONE fp32
//      operation: csrc/hadamard.hip's rule);
//   2. for m > 1 the m-point stage across the chunks: for every b,  w[a] = sum over a' = 0 .. m-1 of H_m[a][a'] v[a' 2^k + b],
//      accumulated left to right in fp32 from +-v[b] (a negation is exact), every further term ONE fp32 add or subtract (formed here as
//      acc + (+-v): x - y and x + (-y) are the same IEEE operation), all m outputs of a column from the old values;
//   3. ONE fp32 multiply by c = (float)(1 / sqrt((double)n)).
// H_12, H_20: Paley I (q = 11, 19): H = I + S, S = [[0, 1^T], [-1, Q]], Q[i][j] = chi_q(j - i).  H_28: Paley II (q = 13): S = [[0, 1^T],
// [1, Q]] of order 14, H = S (x) [[1, 1], [1, -1]] + I (x) [[1, -1], [-1, -1]].  Built below by code from Legendre symbols, once.
// The Paley I tables are not symmetric, so the inverse of R is R^T, a definition of its own: the m-point stage FIRST, with H_m^T and the
// same left-to-right order, then the butterflies ascending, then the multiply.  For m = 1 and m = 28 (H_28 is symmetric) R^T and R are
// the same map, and for m = 1 the same bits; for m = 28 the bits may differ because the m-point stage runs before the butterflies.
//   out = round_to(dtype_out, R(x))                      precision == 0
//   out = round_to(dtype_out, Q(R(x)))                   precision  > 0, inverse == 0
//   out = round_to(dtype_out, R^T(Q(R(x))))              precision  > 0, inverse != 0          (`transpose` swaps R and R^T throughout)
// Q: the dynamic integer cast of csrc/dynamic_quant.hip on the rotated fp32 row -- segment = n: the row is the segment (per token);
// segment = g, a power of two 16 .. 256 dividing 2^k: groups of g consecutive elements -- with the SHARED csrc/dynamic_quant.hpp
// (DynExt's NaN rule, dyn_group_minmax, qparams_one through DynSeg, the reciprocal / division rule of dyn_cast_vec).
// NaN / Inf propagate through the adds.  No FMA anywhere in the rotation (-ffp-contract=off).
//
// Geometry: ONE ROW PER WORKGROUP, read once with 16-byte loads, written once; everything between lives in registers and LDS.
//   * vector layout: thread t holds the 16-byte vectors j = t + u T (u < U) of the row, V = 8 sixteen-bit or 4 fp32 elements each.  A wave's 64
//     lanes of one u are 64 V consecutive elements ("span"): strides below V run inside the lane's vector, strides V .. 32 V across
//     lanes with __shfl_xor in csrc/hadamard.hip's own form (the lower lane adds, the upper lane subtracts partner - own).
//   * column layout, for the strides from 64 V up and for the m-point stage: the row goes to an fp32 copy in LDS (address = element
//     index), and after one barrier thread t owns the columns b' = t, t + T, ..: neighbouring lanes take neighbouring b', so every LDS
//     access of a wave is 64 consecutive words -- distinct banks.  A column's 2^k / (64 V) elements per chunk (high strides) and its m
//     elements per b (m-point stage) are loaded into registers, transformed, and written back in place: the same thread owns a column in
//     both passes (64 V is a multiple of T), so no barrier separates them.  One more barrier, and the row returns to the vector layout.
//   The stage ORDER never changes -- only which thread holds which element: R = low strides (vector layout) -> exchange -> high strides,
//   m-point stage (column layout) -> exchange -> multiply; R^T = exchange -> m-point stage -> exchange -> low strides -> exchange -> high
//   strides -> exchange -> multiply (exchanges with nothing to do between them are skipped).  The cast and the store want the vector
//   layout: a group of g elements is g / V adjacent lanes, as in csrc/dynamic_quant.hip.
//   * extrema: fkey keys, dyn_group_minmax inside the wave; per token the waves' keys meet in the first words of the LDS row, which is
//     dead between two exchanges.
//   * LDS: 4 n bytes of dynamic LDS, 64 KiB at n = 16384 -- exactly the limit a launch may ask for without an attribute; the key
//     exchange reuses the row, so nothing is added to it.
//   * classes (dmxq_hadamard_row_class): WAVE = 64 threads, rows of up to 256 vectors (U = 1, 2, 4); BLOCK = 256 threads beyond (U = 2,
//     4, 8, 16).  U and the dtypes are compile-time; m (1 / 12 / 20 / 28) and the high-stride count select compile-time bodies through
//     wave-uniform switches; 2^k, the lane count of the shuffles and the group width are run-time and wave-uniform.  H_m reaches the
//     kernel as sign masks, one 32-bit word per row (bit a' set: H_m[a][a'] = -1), by value, H_m and H_m^T both.
//   * lanes past the row's last vector re-read it, meet only each other in the shuffles (the row ends on a span or chunk boundary),
//     take no part in the extrema and store nothing.  The whole row is read before any of it is written: in == out is fine when both
//     dtypes have one width.  64-bit row offsets.  No allocation, no host synchronisation: capturable.
#include <math.h>

#include "dynamic_quant.hpp"   // DynFmt, DynExt, dyn_group_minmax, DynSeg, dyn_cast_vec: shared with csrc/dynamic_quant.hip, csrc/awq.hip

namespace dmxq {
namespace {

constexpr int kHrMaxM = 28;
constexpr int kHrMinRow = 512, kHrMaxRow = 16384;

struct HadRowArgs {
  int n, P, m;         // row = m chunks of P = 2^k elements
  int lanes;           // lanes of a low-stride butterfly group: min(P, 64 V) / V
  int hh;              // high strides: P / (64 V) elements of a column per chunk, 1: none
  int transpose, inverse, prec;
  int seg_lanes;       // lanes per group (g / V), 0: the row is the segment
  int seg_per_row;     // n / g
  float c;
  DynFmt f;
};

struct HadRowTab {
  uint32_t fwd[kHrMaxM];   // sign masks of the FIRST rotation's m-point stage (H_m, or H_m^T under `transpose`)
  uint32_t inv[kHrMaxM];   // ... of the rotation back (the other one)
};

// strides 1 .. V lanes / 2 of the vector layout
template <int V, int U>
__device__ __forceinline__ void hr_low(float (&x)[U][V], int lanes, int lane) {
#pragma unroll
  for (int u = 0; u < U; u++) {
#pragma unroll
    for (int s = 1; s < V; s <<= 1) {
#pragma unroll
      for (int i = 0; i < V; i++) {
        if (!(i & s)) {
          const float a = x[u][i], b = x[u][i + s];
          x[u][i] = a + b;
          x[u][i + s] = a - b;
        }
      }
    }
  }
  for (int msk = 1; msk < lanes; msk <<= 1) {   // (every lane of the wave takes part: `lanes` is uniform)
    const bool upper = (lane & msk) != 0;
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
      for (int i = 0; i < V; i++) {
        const float p = __shfl_xor(x[u][i], msk);
        x[u][i] = upper ? p - x[u][i] : x[u][i] + p;
      }
    }
  }
}

template <int V, int T, int U>
__device__ __forceinline__ void hr_to_lds(const float (&x)[U][V], float* s, int t, int nvec) {
  __syncthreads();   // (every reader of the row's previous contents is done)
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = u * T + t;
    if (j < nvec) {
#pragma unroll
      for (int q = 0; q < V; q += 4) *(f32x4*)(s + j * V + q) = (f32x4){x[u][q], x[u][q + 1], x[u][q + 2], x[u][q + 3]};
    }
  }
  __syncthreads();
}

template <int V, int T, int U>
__device__ __forceinline__ void hr_from_lds(float (&x)[U][V], const float* s, int t, int nvec) {
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = u * T + t;
    const int jc = j < nvec ? j : nvec - 1;
#pragma unroll
    for (int q = 0; q < V; q += 4) {
      const f32x4 v = *(const f32x4*)(s + jc * V + q);
      x[u][q] = v.x; x[u][q + 1] = v.y; x[u][q + 2] = v.z; x[u][q + 3] = v.w;
    }
  }
}

// strides 64 V .. P / 2, in place in the LDS row: column b' < 64 V of chunk a holds HH elements, 64 V apart
template <int HH, int V, int T>
__device__ __forceinline__ void hr_high(float* s, int P, int m, int t) {
  constexpr int B1 = kWave * V;
  for (int a = 0; a < m; a++) {
    for (int b = t; b < B1; b += T) {
      float* col = s + a * P + b;
      float v[HH];
#pragma unroll
      for (int h = 0; h < HH; h++) v[h] = col[h * B1];
#pragma unroll
      for (int st = 1; st < HH; st <<= 1) {
#pragma unroll
        for (int h = 0; h < HH; h++) {
          if (!(h & st)) {
            const float p = v[h], q = v[h + st];
            v[h] = p + q;
            v[h + st] = p - q;
          }
        }
      }
#pragma unroll
      for (int h = 0; h < HH; h++) col[h * B1] = v[h];
    }
  }
}

// the m-point stage, in place in the LDS row: column b < P holds M elements, P apart; w: the sign masks (scalar registers)
template <int M, int T>
__device__ __forceinline__ void hr_mstage(float* s, int P, const uint32_t (&w)[kHrMaxM], int t) {
  for (int b = t; b < P; b += T) {
    float v[M];
#pragma unroll
    for (int a = 0; a < M; a++) v[a] = s[a * P + b];
#pragma unroll
    for (int a = 0; a < M; a++) {
      const uint32_t row = w[a];
      float acc = u2f(f2u(v[0]) ^ (row << 31));
#pragma unroll
      for (int k = 1; k < M; k++) acc = acc + u2f(f2u(v[k]) ^ ((row << (31 - k)) & 0x80000000u));
      s[a * P + b] = acc;
    }
  }
}

template <int T>
__device__ __forceinline__ void hr_mstage_any(float* s, const HadRowArgs& A, const uint32_t (&w)[kHrMaxM], int t) {
  if (A.m == 12) hr_mstage<12, T>(s, A.P, w, t);
  else if (A.m == 20) hr_mstage<20, T>(s, A.P, w, t);
  else hr_mstage<28, T>(s, A.P, w, t);
}

template <int V, int T>
__device__ __forceinline__ void hr_high_any(float* s, const HadRowArgs& A, int t) {
  switch (A.hh) {
    case 2: hr_high<2, V, T>(s, A.P, A.m, t); break;
    case 4: hr_high<4, V, T>(s, A.P, A.m, t); break;
    case 8: hr_high<8, V, T>(s, A.P, A.m, t); break;
    case 16: hr_high<16, V, T>(s, A.P, A.m, t); break;
    case 32: hr_high<32, V, T>(s, A.P, A.m, t); break;
    default: if constexpr (V == 4) hr_high<64, V, T>(s, A.P, A.m, t); break;
  }
}

// R (tr == false) or R^T (tr == true) of the row, vector layout in and out; tr and everything in A: uniform over the workgroup
template <int V, int T, int U>
__device__ __forceinline__ void hr_rotate(float (&x)[U][V], float* s, const HadRowArgs& A, const uint32_t (&w)[kHrMaxM], bool tr, int t,
                                          int nvec) {
  const int lane = t & (kWave - 1);
  if (tr && A.m > 1) {
    hr_to_lds<V, T, U>(x, s, t, nvec);
    hr_mstage_any<T>(s, A, w, t);
    hr_from_lds<V, T, U>(x, s, t, nvec);
  }
  hr_low<V, U>(x, A.lanes, lane);
  const bool m_after = !tr && A.m > 1;
  if (A.hh > 1 || m_after) {
    hr_to_lds<V, T, U>(x, s, t, nvec);
    if (A.hh > 1) hr_high_any<V, T>(s, A, t);
    if (m_after) hr_mstage_any<T>(s, A, w, t);
    hr_from_lds<V, T, U>(x, s, t, nvec);
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
#pragma unroll
    for (int i = 0; i < V; i++) x[u][i] = x[u][i] * A.c;
  }
}

// one row per workgroup of T threads; U x T >= n / V.  QUANT: built with the cast (DTI == DTO)
template <int DTI, int DTO, int T, int U, bool QUANT>
__global__ __launch_bounds__(T) void hadamard_row_kernel(const void* in, void* out, const HadRowArgs A, const HadRowTab tab,
                                                        float* __restrict__ scale_out, int64_t* __restrict__ zp_out) {
  constexpr int V = 16 / Elem<DTI>::bytes;
  extern __shared__ __attribute__((aligned(16))) float s_row[];
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int nvec = A.n / V;
  const int64_t row = blockIdx.x;
  const int64_t e_row = row * (int64_t)A.n;
  float x[U][V];
  {
    u32x4 raw[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int j = u * T + t;
      raw[u] = load_raw16<true>(in, (e_row + (int64_t)(j < nvec ? j : nvec - 1) * V) * Elem<DTI>::bytes);
    }
#pragma unroll
    for (int u = 0; u < U; u++) widen<DTI, V>(raw[u], x[u]);
  }
  hr_rotate<V, T, U>(x, s_row, A, tab.fwd, A.transpose != 0, t, nvec);
  if constexpr (QUANT) {
    if (A.prec > 0) {
      if (A.seg_lanes == 0) {   // the row is the segment
        DynExt e;
        e.init();
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (u * T + t < nvec) {
#pragma unroll
            for (int k = 0; k < V; k++) e.FloatExtrema::add(x[u][k]);
          }
        }
        uint32_t klo, khi;
        e.keys(klo, khi);
        dyn_group_minmax(klo, khi, kWave);
        if constexpr (T > kWave) {   // (the LDS row is dead here: the keys take its first words)
          uint32_t* su = (uint32_t*)s_row;
          constexpr int W = T / kWave;
          __syncthreads();
          if (lane == 0) { su[t / kWave] = klo; su[W + t / kWave] = khi; }
          __syncthreads();
#pragma unroll
          for (int i = 0; i < W; i++) { klo = min(klo, su[i]); khi = max(khi, su[W + i]); }
        }
        DynSeg sg;
        sg.setup(klo, khi, A.f);
        const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.sc)) == 0ull;
        const bool all_zp0 = __builtin_amdgcn_ballot_w64(sg.z != 0.0f) == 0ull;
        if (t == 0) {
          if (scale_out) scale_out[row] = sg.sc;
          if (zp_out) zp_out[row] = sg.zp;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          float y[V];
          dyn_cast_vec<V>(x[u], y, sg, all_fast, all_zp0, A.f);
#pragma unroll
          for (int k = 0; k < V; k++) x[u][k] = y[k];
        }
      } else {   // groups of seg_lanes adjacent lanes
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int j = u * T + t;
          DynExt e;
          e.init();
#pragma unroll
          for (int k = 0; k < V; k++) e.FloatExtrema::add(x[u][k]);
          uint32_t klo, khi;
          e.keys(klo, khi);
          dyn_group_minmax(klo, khi, A.seg_lanes);
          DynSeg sg;
          sg.setup(klo, khi, A.f);
          const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.sc)) == 0ull;
          const bool all_zp0 = __builtin_amdgcn_ballot_w64(sg.z != 0.0f) == 0ull;
          float y[V];
          dyn_cast_vec<V>(x[u], y, sg, all_fast, all_zp0, A.f);
#pragma unroll
          for (int k = 0; k < V; k++) x[u][k] = y[k];
          if (j < nvec && (lane & (A.seg_lanes - 1)) == 0) {
            const int64_t g = row * (int64_t)A.seg_per_row + j / A.seg_lanes;
            if (scale_out) scale_out[g] = sg.sc;
            if (zp_out) zp_out[g] = sg.zp;
          }
        }
      }
      if (A.inverse) hr_rotate<V, T, U>(x, s_row, A, tab.inv, A.transpose == 0, t, nvec);
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = u * T + t;
    if (j < nvec) store_vec<DTO, V>(out, e_row + (int64_t)j * V, x[u]);
  }
}

// ---------------------------------------------------------------------------------------------------- host: tables, routing, launch
inline int legendre(int a, int q) {   // chi_q(a): 0, or +1 for a quadratic residue mod q, else -1
  a = ((a % q) + q) % q;
  if (a == 0) return 0;
  for (int r = 1; r < q; r++)
    if (r * r % q == a) return 1;
  return -1;
}

// H_m[a][b] in {+1, -1}; m in {12, 20, 28}
void hr_matrix(int m, int8_t (&H)[kHrMaxM][kHrMaxM]) {
  if (m == 12 || m == 20) {   // Paley I
    const int q = m - 1;
    for (int a = 0; a < m; a++)
      for (int b = 0; b < m; b++) {
        int sgn;
        if (a == b) sgn = 1;                            // I (S has a zero diagonal)
        else if (a == 0) sgn = 1;
        else if (b == 0) sgn = -1;
        else sgn = legendre((b - 1) - (a - 1), q);
        H[a][b] = (int8_t)sgn;
      }
  } else {   // Paley II, q = 13
    const int q = 13, N = q + 1;
    for (int a = 0; a < N; a++)
      for (int b = 0; b < N; b++) {
        const int sv = a == b ? 0 : (a == 0 || b == 0) ? 1 : legendre((b - 1) - (a - 1), q);
        const int blk_s[2][2] = {{1, 1}, {1, -1}}, blk_i[2][2] = {{1, -1}, {-1, -1}};
        for (int i = 0; i < 2; i++)
          for (int j = 0; j < 2; j++) H[2 * a + i][2 * b + j] = (int8_t)(sv * blk_s[i][j] + (a == b ? blk_i[i][j] : 0));
      }
  }
}

// n = m 2^k with m in {1, 12, 20, 28} (the odd part of n is 1, 3, 5 or 7), 512 <= n <= 16384; -> false otherwise
bool hr_split(int64_t n, int* m, int* P) {
  if (n < kHrMinRow || n > kHrMaxRow) return false;
  int64_t odd = n;
  while ((odd & 1) == 0) odd >>= 1;
  if (odd != 1 && odd != 3 && odd != 5 && odd != 7) return false;
  *m = odd == 1 ? 1 : (int)odd * 4;
  *P = (int)(n / *m);
  return true;
}

// THE routing rule: 0 = not taken, DMXQ_HADROW_WAVE = a 64-thread workgroup per row, DMXQ_HADROW_BLOCK = a 256-thread one
int hr_class(int64_t n, int dtype, int64_t segment) {
  int m, P;
  if (!valid_dtype(dtype) || !hr_split(n, &m, &P)) return DMXQ_HADROW_NONE;
  const int V = dtype == DMXQ_F32 ? 4 : 8;
  if (segment != 0 && segment != n) {   // groups: a power of two 16 .. 256 dividing 2^k
    if (segment < 16 || segment > 256 || (segment & (segment - 1)) != 0 || P % segment != 0) return DMXQ_HADROW_NONE;
  }
  return n / V <= 256 ? DMXQ_HADROW_WAVE : DMXQ_HADROW_BLOCK;
}

const HadRowTab& hr_tab(int m, bool transpose) {
  static HadRowTab tabs[3][2];
  static const bool ready = [] {
    const int ms[3] = {12, 20, 28};
    for (int i = 0; i < 3; i++) {
      int8_t H[kHrMaxM][kHrMaxM];
      hr_matrix(ms[i], H);
      for (int a = 0; a < ms[i]; a++) {
        uint32_t plain = 0u, trans = 0u;
        for (int b = 0; b < ms[i]; b++) {
          if (H[a][b] < 0) plain |= 1u << b;
          if (H[b][a] < 0) trans |= 1u << b;
        }
        tabs[i][0].fwd[a] = plain; tabs[i][0].inv[a] = trans;
        tabs[i][1].fwd[a] = trans; tabs[i][1].inv[a] = plain;
      }
    }
    return true;
  }();
  (void)ready;
  return tabs[m == 12 ? 0 : (m == 20 ? 1 : 2)][transpose ? 1 : 0];   // (m == 1: never read by the kernel)
}

template <int DTI, int DTO, bool QUANT>
int hr_launch(const void* in, void* out, int64_t rows, const HadRowArgs& A, const HadRowTab& tab, float* scale_out, int64_t* zp_out,
              hipStream_t s) {
  constexpr int V = 16 / Elem<DTI>::bytes;
  const int nvec = A.n / V;
  const size_t lds = (size_t)A.n * 4;   // <= 64 KiB
#define DMXQ_HR(T_, U_) \
  DMXQ_LAUNCH((hadamard_row_kernel<DTI, DTO, T_, U_, QUANT>), dim3((unsigned)rows), dim3(T_), lds, s, in, out, A, tab, scale_out, zp_out)
  if (nvec <= 64) DMXQ_HR(64, 1);
  else if (nvec <= 128) DMXQ_HR(64, 2);
  else if (nvec <= 256) DMXQ_HR(64, 4);
  else if (nvec <= 512) DMXQ_HR(256, 2);
  else if (nvec <= 1024) DMXQ_HR(256, 4);
  else if (nvec <= 2048) DMXQ_HR(256, 8);
  else if constexpr (V == 4) DMXQ_HR(256, 16);
  else return DMXQ_ERR_UNSUPPORTED;
#undef DMXQ_HR
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_hadamard_row_class(int64_t n, int dtype_in, int64_t segment) { return hr_class(n, dtype_in, segment); }

extern "C" int dmxq_hadamard_matrix(int m, int8_t* table) {
  if (!table || (m != 1 && m != 12 && m != 20 && m != 28)) return DMXQ_ERR_BAD_ARG;
  if (m == 1) { table[0] = 1; return DMXQ_OK; }
  int8_t H[kHrMaxM][kHrMaxM];
  hr_matrix(m, H);
  for (int a = 0; a < m; a++)
    for (int b = 0; b < m; b++) table[a * m + b] = H[a][b];
  return DMXQ_OK;
}

extern "C" int dmxq_hadamard_row_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t rows, int64_t n, int transpose,
                                     int inverse, int precision, int symmetric, int64_t segment, float* scale_out,
                                     int64_t* zero_point_out, void* stream) {
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || rows < 0 || n < 0 || segment < 0 || precision < 0) return DMXQ_ERR_BAD_ARG;
  if (precision == 0 && inverse) return DMXQ_ERR_BAD_ARG;
  if (rows > 0 && n > 0 && (!in || !out)) return DMXQ_ERR_BAD_ARG;
  const int bi = dtype_in == DMXQ_F32 ? 4 : 2, bo = dtype_out == DMXQ_F32 ? 4 : 2;
  if (in && in == (const void*)out && bi != bo) return DMXQ_ERR_BAD_ARG;   // in place: equal widths only
  // what the kernel takes; everything else is the caller's chain (nothing launched)
  const int cls = hr_class(n, dtype_in, precision > 0 ? segment : 0);
  if (cls == DMXQ_HADROW_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (precision > 0 ? (dtype_out != dtype_in || precision < 2 || precision > 22 || segment == 0)
                    : (dtype_out != dtype_in && dtype_out != DMXQ_F32))
    return DMXQ_ERR_UNSUPPORTED;
  if (rows == 0) return DMXQ_OK;
  if (!aligned16(in) || !aligned16(out) || rows > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  const int V = 16 / bi;
  HadRowArgs A{};
  A.n = (int)n;
  hr_split(n, &A.m, &A.P);
  const int span = kWave * V;
  A.lanes = (A.P < span ? A.P : span) / V;
  A.hh = A.P > span ? A.P / span : 1;
  A.transpose = transpose ? 1 : 0;
  A.inverse = inverse ? 1 : 0;
  A.prec = precision;
  A.seg_lanes = (precision > 0 && segment != n) ? (int)(segment / V) : 0;
  A.seg_per_row = A.seg_lanes ? (int)(n / segment) : 1;
  A.c = (float)(1.0 / sqrt((double)n));
  if (precision > 0) {
    const int fmt_sym = (symmetric & 2) ? 1 : 0;
    const FixedFmt x = make_fixed_fmt(precision, 0, 1, fmt_sym, DMXQ_ROUND_NEAREST, 0ull);
    const int qmax = (1 << (precision - 1)) - 1, qmin = -(1 << (precision - 1)) + fmt_sym;
    A.f = DynFmt{x.t_min, x.t_max, qmin, qmax, (symmetric & 1) ? 1 : 0};
  }
  const HadRowTab& tab = hr_tab(A.m, transpose != 0);
  hipStream_t s = (hipStream_t)stream;
  if (dtype_in == DMXQ_BF16 && dtype_out == DMXQ_BF16) return hr_launch<DMXQ_BF16, DMXQ_BF16, true>(in, out, rows, A, tab, scale_out, zero_point_out, s);
  if (dtype_in == DMXQ_F16 && dtype_out == DMXQ_F16) return hr_launch<DMXQ_F16, DMXQ_F16, true>(in, out, rows, A, tab, scale_out, zero_point_out, s);
  if (dtype_in == DMXQ_F32 && dtype_out == DMXQ_F32) return hr_launch<DMXQ_F32, DMXQ_F32, true>(in, out, rows, A, tab, scale_out, zero_point_out, s);
  if (dtype_in == DMXQ_BF16) return hr_launch<DMXQ_BF16, DMXQ_F32, false>(in, out, rows, A, tab, scale_out, zero_point_out, s);
  return hr_launch<DMXQ_F16, DMXQ_F32, false>(in, out, rows, A, tab, scale_out, zero_point_out, s);
}
