/* include/dmxq.h — C ABI of libdmxq.so, the MI355X (gfx950) fake-quantisation / sparsity operator library.
 *
 * This is the drop-in boundary for the hot path of d-matrix-ai/dmx-compressor (reference paths below are
 * relative to /root/reference/src/dmx/compressor/).  The reference's native seam is a pair of pybind
 * modules, `quant_cpu` / `quant_cuda`, picked per call by quant/quant_function.py:38-43; each entry point
 * here replaces one family of those pybind functions *and* the Python loop that drives it, so that one call
 * (= one kernel launch) handles a whole tensor.
 *
 * Conventions (all entry points):
 *   - plain C: raw DEVICE pointers + explicit 64-bit sizes, no torch types, never throws, no state for the caller to manage
 *     (the reductions -- dmxq_group_minmax, dmxq_channel_maxabs, dmxq_histc -- keep 64 KiB of flag words per device, allocated on
 *     first use and never freed: ONE wave of the kernel initialises the outputs and publishes the launch's epoch, the workgroups wait
 *     for it before their atomics, instead of a fill launch in front of every call.  Which wave is decided by a claim on an election
 *     word -- an extra workgroup without data volunteers at once, any waiting workgroup takes the job over after a bounded number of
 *     polls -- so the protocol does not depend on dispatch order or on what else occupies the GPU; csrc/reduce.hip "init gate".
 *     While `stream` is being captured into a graph, and with DMXQ_NO_INIT_GATE set in the environment, they use the fill launch,
 *     so a captured call is replayable.  HARDWARE ASSUMPTION of the default build: the publishing wave orders its plain `sc1` stores
 *     (the identities) before its flag store with `s_waitcnt vmcnt(0)`, and the waiting waves read the flag with agent-scope atomics --
 *     i.e. it relies on gfx950 acknowledging an `sc1` store only once it is visible at the agent coherence point (all eight XCD L2s)
 *     and on atomics never being served from a stale cached line.  That is behaviour of this hardware, not a guarantee of the LLVM
 *     AMDGPU memory model; `-DDMXQ_GATE_FENCES=1` builds the formal release / acquire form (measured slower than the fill launch it
 *     replaces, profiles/r05_gate_ab.txt; built as lib/libdmxq_gate_fences.so and put through the same stress tests, tests/test_gpu_round6.py), and DMXQ_NO_INIT_GATE=1 removes the protocol at run time);
 *   - caller-allocated outputs (the reference allocates with zeros_like and returns a new tensor,
 *     quant_cuda.cpp:116-139 — the host mirror keeps that ownership contract above this ABI);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); launches are asynchronous;
 *   - as for any HIP launch, the device that owns the pointers and the stream must be CURRENT on the calling thread
 *     (the host mirror and the torch extension switch to the tensor's device around every call and restore it);
 *   - return value: DMXQ_OK, or an error code (see dmxq_status_string); nothing is launched on error;
 *   - tensors are described as a contiguous [outer, L, inner] (or [outer, C, inner]) view: `L`/`C` is the
 *     extent of the blocked / channel dimension, `inner` the product of the dimensions after it
 *     (block_dim=-1  <=>  inner = 1).  in and out may alias exactly (in-place) but must not partially overlap.
 */
#ifndef DMXQ_H
#define DMXQ_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { DMXQ_F32 = 0, DMXQ_F16 = 1, DMXQ_BF16 = 2 } dmxq_dtype;

/* Rounding modes, numbered like the reference's `enum Mode` (quant/quant_cpu/quant_cpu.cpp:9-15). */
typedef enum { DMXQ_ROUND_UP = 0, DMXQ_ROUND_DOWN = 1, DMXQ_ROUND_NEAREST = 2, DMXQ_ROUND_STOCHASTIC = 3 } dmxq_rounding;

typedef enum {
  DMXQ_OK = 0,
  DMXQ_ERR_BAD_ARG = 1,     /* null pointer, negative size, misaligned/invalid enum ... */
  DMXQ_ERR_UNSUPPORTED = 2, /* parameter outside what the reference defines (e.g. mantissa bits = 23: UB there) */
  DMXQ_ERR_LAUNCH = 3,      /* hipGetLastError() != hipSuccess after the launch */
  DMXQ_ERR_PENDING = 4      /* a HIP error of ANOTHER user of this host thread was already pending before the call (HIP keeps one
                               "last error" per thread): the launches were issued but cannot be verified, so the outputs must not be
                               trusted; the foreign error is left in place for its owner to collect (hipGetLastError) */
} dmxq_status;

const char* dmxq_status_string(int status);
/* ABI version: bumped on any signature change.  Additions since 4 (dmxq_gptq_block, dmxq_hist_observe, dmxq_hist_qparams, dmxq_error_stats, dmxq_cast_error,
 * dmxq_error_scratch_bytes, dmxq_hadamard_qdq, dmxq_dynamic_fixed_qdq, dmxq_dynamic_class, dmxq_gptq_block_dynamic,
 * dmxq_dynamic_float_qdq, dmxq_dynamic_float_class, dmxq_channel_sumsq_accumulate, dmxq_channel_sumsq_workspace_bytes, dmxq_wanda_nm,
 * dmxq_wanda_class, dmxq_row_class_of, dmxq_channel_sumabs_accumulate, dmxq_awq_group_error, dmxq_awq_class,
 * dmxq_block_scaled_float_qdq, dmxq_block_scaled_float_class, dmxq_block_scaled_tensor_scale, dmxq_nm_mask_class, dmxq_lsq_backward, dmxq_lsq_class, dmxq_lsq_scratch_bytes,
 * dmxq_codebook_qdq, dmxq_codebook_class, dmxq_codebook_accumulate, dmxq_codebook_workspace_bytes, dmxq_hqq_qdq, dmxq_hqq_class,
 * dmxq_outlier_fixed_qdq, dmxq_outlier_class, dmxq_awq_clip, dmxq_awq_clip_class, dmxq_adaround_forward, dmxq_adaround_backward,
 * dmxq_adaround_class, dmxq_adaround_scratch_bytes, dmxq_vq_qdq, dmxq_vq_class, dmxq_vq_accumulate, dmxq_vq_workspace_bytes) leave it at 4: a caller built against 4 runs on
 * this library unchanged.  4 = round 5: + dmxq_float_qdq_multi, dmxq_fixed_float_qdq_multi; 3 = round 4: + dmxq_weight_hypernet_multi,
 * dmxq_unary_cast_table, dmxq_lut16_apply.  Nothing was ever removed or changed: a caller built against version n runs on any library >= n. */
int dmxq_abi_version(void);

/* Block floating point Q->DQ ("BFP[p|8]{B}", MXINT).
 * Replaces: numerical/format.py:304-343 BlockFloatingPoint.cast (split / per-chunk / cat loop)
 *           -> quant/quant_function.py:87-117 block_quantize -> quant_cpu.cpp:239-311 / quant_cuda/quant.cu:14-112
 *           + format.py:349-372 make_mantissa_asymmetric (symmetric = 0)
 *           + the `.float()` / `.to(physical_dtype)` round trip of numerical/cast.py:262,306 (dtype_in/dtype_out).
 * Blocks are `block_size` consecutive indices along L (stride `inner`); a ragged last block is allowed
 * (torch.split semantics).  block_size == 1 takes the reference's float_quantize detour (format.py:312-320).
 * precision = total mantissa bits incl. sign ("8" in BFP[8|8]); 2 <= precision <= 22 when block_size > 1.
 * symmetric: 1 = symmetric codes; 0 = the asymmetric format "(_N)" = symmetric pass + make_mantissa_asymmetric, which is
 * all the Python layer ever asks for (format.py:332 forces the native flag to true); DMXQ_BFP_ASYM_NATIVE (2) = the
 * native `symmetric = false` of the pybind seam block_quantize_*(a, wl, dim, symmetric) (quant_cpu.cpp:247-253: an
 * element equal to -max whose maximum has its top 7 mantissa bits set takes the next exponent), float32 only. */
#define DMXQ_BFP_ASYM_NATIVE 2
int dmxq_bfp_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t outer, int64_t L, int64_t inner,
                 int64_t block_size, int precision, int rounding, int symmetric, uint64_t seed, void* stream);

/* Multi-tensor BFP Q->DQ: exactly the result of one dmxq_bfp_qdq call per tensor (same dtype pair and format for all),
 * in as few launches as possible.  Replaces the per-module loop of modeling/model.py fold_weights_and_biases /
 * DmxModule.weight_hypernet over MANY small weights (opt-125m: 73 Linear weights of 768x768 .. 3072x768, each of which
 * is launch-bound on its own: ~4 us per launch for 0.4-1.6 us of streaming).  `tensors` is a HOST array; tensors that
 * are flat row-blocked (inner == 1, L % block_size == 0, 16-byte aligned, nearest rounding) are packed 48 to a launch
 * over a concatenated tile space, the others get their own launch (stochastic rounding: seed + index). */
typedef struct { const void* in; void* out; int64_t outer, L, inner; } dmxq_tensor_desc;
int dmxq_bfp_qdq_multi(const dmxq_tensor_desc* tensors, int64_t n_tensors, int dtype_in, int dtype_out,
                       int64_t block_size, int precision, int rounding, int symmetric, uint64_t seed, void* stream);

/* Introspection (no launch): writes into buf (NUL-terminated, at most buf_len bytes) the kernel and tile geometry that
 * dmxq_bfp_qdq would launch for these arguments; `aligned` = both pointers are 16-byte aligned.  bench.py reports it
 * next to the roofline numbers, so that the named kernel is the dispatcher's own choice, not a constant. */
int dmxq_bfp_qdq_describe(int dtype_in, int dtype_out, int64_t outer, int64_t L, int64_t inner, int64_t block_size,
                          int precision, int rounding, int symmetric, int aligned, char* buf, int64_t buf_len);

/* Scaled block floating point Q->DQ ("SBFP<XP[p,0](CSN)><FP[0|e|m,bias](FN)>{B}", e.g. SBFP12_16 weight storage).
 * Replaces: numerical/format.py:453-479 ScaledBlockFloatingPoint.cast.  Per block: s = max|x| / (2^(p-1)-1);
 * y = fixed(x / s; p, 0, clamp, symmetric, nearest) * |float(s; man, exp, bias, flush)| where s > 0, else x.
 * Same [outer, L, inner] / ragged-tail conventions as dmxq_bfp_qdq. */
int dmxq_sbfp_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t outer, int64_t L, int64_t inner,
                  int64_t block_size, int precision, int clamp, int symmetric, int scaler_man_bits, int scaler_exp_bits,
                  int scaler_exp_bias, int scaler_flush_subnormal, void* stream);

/* MX floating point Q->DQ ("MXFP8[E4M3]{32}", ...): low-bit float elements with a power-of-two (E8M0) block scale.
 * Replaces: numerical/format.py:545-564 MXFP.cast.  Per block: scale = 2^floor(log2 max|x|) / 2^(2^(e-1));
 * y = float(x / scale; man, exp, bias = 2^(e-1)-1, no flush, nearest) * scale.  Blocks run along L as in
 * dmxq_bfp_qdq (the reference's `cat(dim=block_dim)` slip is not reproduced); an all-zero block stays zero (the
 * reference produces NaN through log2(0)). */
int dmxq_mxfp_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t outer, int64_t L, int64_t inner,
                  int64_t block_size, int man_bits, int exp_bits, void* stream);

/* Packed on-wire BFP: int8 mantissa codes + one uint8 shared exponent per block (the com.microsoft::QuantizeBFP /
 * DequantizeBFP pair the reference's export names, numerical/cast.py:34-55; type ids numerical/onnx.py).
 * x is [rows, L] contiguous, blocks of block_size along L (ragged tail allowed); mant: int8[rows*L];
 * exps: uint8[rows * ceil(L / block_size)] = biased fp32 exponent of the block maximum.  precision <= 8.
 * dmxq_bfp_unpack(dmxq_bfp_pack(x)) == dmxq_bfp_qdq(x) bit for bit for blocks with a normal finite maximum
 * (denormal / zero maxima pack to zeros, Inf/NaN maxima to exps = 255 -> NaN). */
int dmxq_bfp_pack(const void* in, int dtype_in, int8_t* mant, uint8_t* exps, int64_t rows, int64_t L,
                  int64_t block_size, int precision, int symmetric, void* stream);
int dmxq_bfp_unpack(const int8_t* mant, const uint8_t* exps, void* out, int dtype_out, int64_t rows, int64_t L,
                    int64_t block_size, int precision, void* stream);

/* Low-bit floating point Q->DQ ("FP[s|e|m,bias](F|_ N|S)").
 * Replaces: numerical/format.py:208-233 FloatingPoint.cast -> quant_function.py:120-152 float_quantize
 *           -> quant_cpu.cpp:359-402 / quant_cuda/float_kernel.cu.  0 <= man_bits <= 22 (23 is UB in the
 *           reference; the host mirror treats FP32 as the identity), 1 <= exp_bits <= 8.
 * unsigned_abs != 0 applies the final `.abs()` of sign-less formats (format.py:233). */
int dmxq_float_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n, int man_bits, int exp_bits,
                   int exp_bias, int flush_subnormal, int unsigned_abs, int rounding, uint64_t seed, void* stream);

/* Multi-tensor twin of dmxq_float_qdq (round 5): exactly the result of one dmxq_float_qdq call per tensor (same dtype pair and format for
 * all; tensor i holds outer * L * inner elements), in as few launches as possible.  Replaces the per-module bias casts of a layer
 * (modeling/nn/core.py:191-203 `_bias = self.bias_cast(self.bias)`, one launch per Linear per forward while biases are not folded:
 * an opt-125m decoder layer has six of 768 .. 3072 elements).  `tensors` is a HOST array.  Batched: nearest rounding, whole 16-byte
 * vectors, 16-byte aligned, < 2^31 elements; every other tensor gets its own launch (stochastic rounding: seed + index). */
int dmxq_float_qdq_multi(const dmxq_tensor_desc* tensors, int64_t n_tensors, int dtype_in, int dtype_out, int man_bits, int exp_bits,
                         int exp_bias, int flush_subnormal, int unsigned_abs, int rounding, uint64_t seed, void* stream);

/* Fixed point Q->DQ ("XP[p,f](C|_ S|_ R)") with the optional affine wrapper fused in.
 * Replaces: numerical/format.py:134-142 FixedPoint.cast -> quant_function.py:47-84 fixed_point_quantize
 *           -> quant_cpu.cpp:127-209 (CPU rounding: half-to-even through sim_helper.cpp:14-21), and
 *           numerical/cast.py:278-296:  x/sc + zp -> cast -> (x - zp)*sc.
 * The tensor is [outer, C, inner]; channel c uses scale[c / group_size], zero_point[c / group_size]
 * (cast.py:281-292 repeat_interleave).  scale == NULL: no affine.  per-tensor: C = 1, group_size = 1. */
int dmxq_fixed_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t outer, int64_t C, int64_t inner,
                   int precision, int fraction, int clamp, int symmetric, int rounding, const float* scale,
                   const int64_t* zero_point, int64_t group_size, uint64_t seed, void* stream);

/* Multi-tensor twin of dmxq_fixed_qdq: exactly the result of one dmxq_fixed_qdq call per tensor (same dtype pair, format
 * and group_size for all; each tensor its own scale / zero-point arrays), in as few launches as possible.  Replaces the
 * per-module loop over the INT8 group-quantised Linear weights of a whole model (numerical/cast.py:278-296 once per module;
 * opt-125m: 73 weights).  `tensors` is a HOST array.  Batched (20 tensors per launch, each with its own op instance in the argument block): integer formats (fraction 0, clamped,
 * nearest), outer == 1 with row slabs of group_size channels or a single group, inner a multiple of the 16-byte vector,
 * < 2^31 elements; every other tensor gets its own launch (stochastic rounding: seed + index). */
typedef struct { const void* in; void* out; const float* scale; const int64_t* zero_point; int64_t outer, C, inner; } dmxq_affine_desc;
int dmxq_fixed_qdq_multi(const dmxq_affine_desc* tensors, int64_t n_tensors, int dtype_in, int dtype_out, int precision,
                         int fraction, int clamp, int symmetric, int rounding, int64_t group_size, uint64_t seed, void* stream);

/* dmxq_fixed_qdq_multi AND dmxq_float_qdq_multi in ONE launch (round 5): a layer's affine integer weight casts and its float bias casts
 * (modeling/nn/core.py:178-203: `_weight` and `_bias` of every module, every forward while nothing is folded), one dtype in and out for all.
 * Exactly the results of the two calls.  Combined: at most 12 + 12 tensors (21 in all), 32 MiB in all, every tensor batchable by its own
 * multi call's rules, nearest rounding on both sides; any other set is run as those two calls. */
int dmxq_fixed_float_qdq_multi(const dmxq_affine_desc* fixed, int64_t n_fixed, int precision, int fraction, int clamp, int symmetric,
                               int rounding_fixed, int64_t group_size, const dmxq_tensor_desc* flt, int64_t n_float, int man_bits,
                               int exp_bits, int exp_bias, int flush_subnormal, int unsigned_abs, int rounding_float, int dtype,
                               uint64_t seed, void* stream);

/* N:M structured-sparsity mask ("BTOPK{K:M,dim}") and its application.
 * Replaces: sparse.py:163-180 BlockTopK.forward (argsort + scatter) and sparse.py:300 `x * mask`.
 * Groups are M consecutive indices along L (stride inner); L % M == 0 required (sparse.py:166-168).
 * Rule: within a group, rank_i = #{j : s_j < s_i or (s_j == s_i and j < i)}, NaN ranks highest;
 * mask_i = 1 iff rank_i >= M-K (stable ascending argsort, first M-K zeroed).
 * mask_out (dtype_mask, float mask of 0/1) and/or y_out = x * mask (dtype_y) may be NULL.  M <= 64. */
int dmxq_nm_mask(const void* score, int dtype_score, const void* x, int dtype_x, void* mask_out, int dtype_mask,
                 void* y_out, int dtype_y, int64_t outer, int64_t L, int64_t inner, int K, int M, void* stream);

/* Which kernel dmxq_nm_mask launches for one call (csrc/nm_mask.hip), answered by the function the entry itself decides with.  A host
 * function: no GPU involved, no HIP call, the four addresses are never dereferenced -- only whether they are NULL (mask_out / y_out: that
 * output is not wanted) and their 16-byte alignment matter.  *route (dmxq_nm_route):
 *   NONE      an empty tensor: nothing is launched;
 *   TYPED     y only, compile-time dtypes (csrc/hypernet.hip): inner == 1, M in {2, 4, 8}, n % 16 == 0, 16-byte bases and (x, score -> y)
 *             one of (bf16, bf16 -> bf16), (f16, f16 -> f16), (f32, f32 -> f32), (bf16, f32 -> f32), (f16, f32 -> f32), (bf16, f32 -> bf16);
 *   F32_MASK  mask only, float32 score and mask, M in {2, 4, 8}, the same geometry: a lane per 16-byte vector;
 *   VECTOR    any other call of that geometry, M = 16 included: a lane per 8 (M = 16: 16) consecutive elements, run-time dtypes;
 *   GROUP_M   M in {2, 4, 8, 16} otherwise (inner != 1, n % 16 != 0 or a base off the 16-byte grid): a lane per group, scalar accesses;
 *   ANY_M     every other M up to 64: the same with run-time loops.
 * Returns DMXQ_OK, or DMXQ_ERR_BAD_ARG exactly where dmxq_nm_mask does (and for route == NULL).
 * DMXQ_GRID_CAP: the most workgroups a grid-stride kernel of the library is launched with (VECTOR, GROUP_M, ANY_M, and the chunk loops
 * of dmxq_topk_mask); larger tensors take further rounds of the same grid. */
#define DMXQ_GRID_CAP 2048
typedef enum { DMXQ_NM_NONE = 0, DMXQ_NM_TYPED = 1, DMXQ_NM_F32_MASK = 2, DMXQ_NM_VECTOR = 3, DMXQ_NM_GROUP_M = 4, DMXQ_NM_ANY_M = 5 } dmxq_nm_route;
int dmxq_nm_mask_class(int dtype_score, int dtype_x, int dtype_mask, int dtype_y, int64_t outer, int64_t L, int64_t inner, int K, int M,
                       const void* score, const void* x, const void* mask_out, const void* y_out, int* route);

/* Unstructured top-k mask ("TOPK{density}") and its application: the n_zero lowest scores of the flattened tensor are
 * zeroed.  Replaces: sparse.py:109-123 TopK.forward (argsort + scatter; n_zero = int(n * (1 - density))) and
 * sparse.py:300 `x * mask`.  Order: ascending, -0 == +0, NaN largest; scores equal to the threshold value are zeroed
 * lowest index first (the reference's unstable argsort leaves that choice undefined).  mask_out (float 0/1 in
 * dtype_mask) and/or y_out = x * mask may be NULL.  workspace: dmxq_topk_workspace_bytes(n) bytes of device memory,
 * 8-byte aligned, contents irrelevant before and after.  n < 2^32. */
int64_t dmxq_topk_workspace_bytes(int64_t n);
int dmxq_topk_mask(const void* score, int dtype_score, const void* x, int dtype_x, void* mask_out, int dtype_mask,
                   void* y_out, int dtype_y, int64_t n, int64_t n_zero, void* workspace, void* stream);

/* Bernoulli supermask ("BERN"): mask[i] = 1 with probability score[i] (scores in [0, 1]), else 0.
 * Replaces: sparse.py:201-221 Bernoulli.forward (torch.bernoulli on the global generator; here a counter-based
 * stream keyed by `seed` and the element index, reproducible, statistically equivalent). */
int dmxq_bernoulli_mask(const void* score, void* mask_out, int dtype_score, int dtype_mask, int64_t n, uint64_t seed,
                        void* stream);

/* Per-group min/max over slabs of `group_size` channels (MinMaxObserver on torch.split slabs).
 * Replaces: numerical/cast.py:179-226 _observer_step + numerical/observer.py:173-193.
 * mn/mx: float[ceil(C/group_size)] device buffers (fully overwritten). */
int dmxq_group_minmax(const void* in, int dtype_in, int64_t outer, int64_t C, int64_t inner, int64_t group_size,
                      float* mn, float* mx, void* stream);

/* The same reduction folded INTO running values: mn[g] = min(mn[g], min over group g), mx[g] = max(mx[g], max over group g), in ONE
 * launch (no initialising launch: mn / mx must hold valid values, +inf / -inf before the first observation).  Replaces
 * numerical/observer.py:173-193 MinMaxObserver.forward as a whole -- the two reductions AND `min_val = torch.min(x_min, min_val)` /
 * `max_val = torch.max(...)` (4 launches with dmxq_group_minmax, ~10 per group in the reference).  Exact and order-independent (integer
 * atomics on the float bit patterns). */
int dmxq_group_minmax_accumulate(const void* in, int dtype_in, int64_t outer, int64_t C, int64_t inner, int64_t group_size,
                                 float* mn, float* mx, void* stream);

/* (min,max) -> (scale, zero_point).  Replaces numerical/observer.py:59-115 _calculate_qparams. */
int dmxq_qparams(const float* mn, const float* mx, int64_t n_groups, int qmin, int qmax, int symmetric_qscheme,
                 float* scale, int64_t* zero_point, void* stream);

/* torch.histc of a flat tensor: hist[b] = #{x : bin(x) == b}, bin(x) = (int64)((x - lo) * bins / (hi - lo)) in
 * fp32, x == hi counted in the last bin, x outside [lo, hi] and NaN dropped (ATen's CPU histc, which the
 * reference's HistogramObserver calls).  Replaces: numerical/observer.py:470-472 and :489-491.
 * Requires finite lo < hi (the "lo == hi means the data's own range" convention of torch.histc is resolved by
 * the caller) and bins <= 8192.  hist: float[bins] device buffer, fully overwritten. */
int dmxq_histc(const void* in, int dtype_in, int64_t n, int64_t bins, float lo, float hi, float* hist, void* stream);

/* Per-channel max|x| (SmoothQuant).  Replaces numerical/smoothquant.py:285-299 _maxabs. out: float[C].
 * DMXQ_ERR_UNSUPPORTED: a plane of C * inner >= 2^32 elements that is not whole 16-byte vectors from an aligned pointer. */
int dmxq_channel_maxabs(const void* in, int dtype_in, int64_t outer, int64_t C, int64_t inner, float* out, void* stream);

/* SmoothQuant scale = clamp(a^alpha / clamp(b, min)^(1-alpha), min).  Replaces smoothquant.py:301-321. */
int dmxq_smoothquant_scale(const float* a_maxabs, const float* b_maxabs, int64_t C, float alpha, float scale_min,
                           float* scale, void* stream);

/* y = x * s[c] (divide = 0) or x / s[c] (divide = 1) along the channel dim of [outer, C, inner], computed in
 * fp32 and rounded once to dtype_out.  Replaces smoothquant.py:255-283 scale_a / scale_b. */
int dmxq_scale_channels(const void* in, void* out, int dtype_in, int dtype_out, int64_t outer, int64_t C,
                        int64_t inner, const float* scale, int divide, void* stream);

/* Fused weight hypernet: N:M mask -> SmoothQuant weight scale -> BFP Q->DQ in one pass over a [rows, L] weight.
 * Replaces the chain of modeling/nn/core.py:178-198 (weight_sparsifier -> smoothquant.scale_weight ->
 * weight_cast) that DmxModule re-runs on every forward, for the Linear layout (mask groups, scale channels and
 * BFP blocks all along the contiguous last dim).  M = 0: no mask (score ignored); sq_scale = NULL: no scaling
 * (else float[L], one per input channel).  Results are bit-identical to the unfused chain, whose intermediate
 * dtypes are reproduced (see csrc/hypernet.hip).  Returns DMXQ_ERR_UNSUPPORTED for geometries it does not fuse
 * (L % block_size != 0, block_size not a power of two in [8,512], M not in {0,2,4,8}, unaligned pointers,
 * dtype combination outside {w,score,out}: the caller then runs the unfused ops). */
int dmxq_weight_hypernet(const void* w, int dtype_w, const void* score, int dtype_score, int K, int M,
                         const float* sq_scale, void* out, int dtype_out, int64_t rows, int64_t L, int64_t block_size,
                         int precision, int symmetric, void* stream);

/* Multi-tensor form of dmxq_weight_hypernet: exactly the result of one dmxq_weight_hypernet call per tensor (one dtype triple, one
 * N:M pattern, one BFP format for all), in as few launches as possible -- up to 32 weights per launch over a concatenated tile
 * space.  Replaces the per-module loop of modeling/nn/core.py:178-198 (DmxModule.weight_hypernet, once per module and forward) and
 * of modeling/model.py fold_weights_and_biases over the Linear weights of a layer: under row sharding over 8 GPUs a
 * rank's seven Llama-3-8B shards are 1-15 MB each, launch-bound one by one.  `tensors` is a HOST array; sq_scale is float[L] for
 * every tensor or NULL for every tensor; score is ignored when M == 0.  All-or-nothing: DMXQ_ERR_UNSUPPORTED (nothing launched)
 * when any tensor has a geometry dmxq_weight_hypernet does not fuse -- the caller then goes tensor by tensor. */
typedef struct { const void* w; const void* score; const float* sq_scale; void* out; int64_t rows, L; } dmxq_hypernet_desc;
int dmxq_weight_hypernet_multi(const dmxq_hypernet_desc* tensors, int64_t n_tensors, int dtype_w, int dtype_score, int K, int M,
                               int dtype_out, int64_t block_size, int precision, int symmetric, void* stream);

/* The same chain for layouts whose blocked dimension is not the contiguous one: w viewed as [outer, L, inner] with the N:M groups,
 * the SmoothQuant channels and the BFP blocks all along L (stride inner) -- Conv1d / Conv2d weights [out, in, k...], whose weight
 * cast, sparsifier and SmoothQuant axis are dim 1 (modeling/nn/torch_modules.py:582-585, 674-677; the chain is
 * modeling/nn/core.py:178-198 as above).  Any block size >= 2 and a ragged last block (torch.split); M in {0, 2, 4, 8} dividing
 * block_size; every dtype combination.  Bit-identical to the unfused chain.  These weights are small: the call is launch-bound and
 * the point is one launch instead of three. */
int dmxq_weight_hypernet_strided(const void* w, int dtype_w, const void* score, int dtype_score, int K, int M,
                                 const float* sq_scale, void* out, int dtype_out, int64_t outer, int64_t L, int64_t inner,
                                 int64_t block_size, int precision, int symmetric, void* stream);

/* The activation twin of the fused weight path: SmoothQuant input scaling -> BFP input cast in one pass over x[rows, L]
 * (channels and blocks along the contiguous last dim).  out = BFP_QDQ(x / sq_scale[c]); the quotient is an IEEE fp32 division
 * and stays fp32 -- torch's promotion of (input dtype, fp32 scale), i.e. what `a / scale` returns in
 * numerical/smoothquant.py:255-268 -- which is then the dtype CastTo sees and returns (numerical/cast.py:262,306), so
 * dtype_out must be DMXQ_F32.  Replaces the first two steps of DmxModule.forward (modeling/nn/core.py:228-232:
 * smoothquant.scale_input -> input_casts) for Linear-layout modules: 6 B/element (bf16 in) instead of 14 (2+4, then 4+4).
 * Bit-identical to dmxq_scale_channels(divide) followed by dmxq_bfp_qdq.  DMXQ_ERR_UNSUPPORTED as dmxq_weight_hypernet. */
int dmxq_input_hypernet(const void* x, int dtype_x, const float* sq_scale, void* out, int dtype_out, int64_t rows, int64_t L,
                        int64_t block_size, int precision, int symmetric, void* stream);

/* A binary DmxModule (ResAdd, Mul) in one pass: out = cast_out(cast_a(a) op cast_b(b)), all three tensors of one dtype, the op
 * evaluated as torch does (fp32 arithmetic on the widened operands, one RNE rounding to the tensor dtype).  Replaces the four
 * launches of modeling/nn/core.py:228-264 for such a module (CastToDict.forward on both inputs, numerical/cast.py:59-86; the op;
 * the output cast): 6 B/element instead of 18.  A cast is described by its FloatingPoint format (numerical/format.py:174-233,
 * nearest rounding, signed, man_bits <= 22); NULL or exp_bits == 0 = SAME.  Two forms: when every cast is RANGE-ONLY for a 16-bit
 * tensor dtype (bf16 with man_bits >= 7, fp16 with man_bits >= 10; subnormals flushed: the FLOAT16-style formats of the BASIC rules)
 * everything happens on the packed 16-bit words; otherwise (casts that round, float32 tensors) per element in fp32 with the
 * arithmetic of dmxq_float_qdq.  DMXQ_ERR_UNSUPPORTED: n not a whole number of 16-byte vectors, unaligned pointers (the caller runs
 * the unfused ops).  Bit-identical to that chain; a / b may alias out.  (The host mirror maps the reference's pass-through of a
 * dtype's own format, numerical/format.py:209-212, to SAME before calling.) */
typedef struct { int man_bits, exp_bits, exp_bias, flush_subnormal; } dmxq_float_fmt;
enum { DMXQ_BINARY_ADD = 0, DMXQ_BINARY_MUL = 1 };
int dmxq_binary_cast(const void* a, const void* b, void* out, int dtype, int64_t n, int op, const dmxq_float_fmt* cast_a,
                     const dmxq_float_fmt* cast_b, const dmxq_float_fmt* cast_out, void* stream);

/* A ReLU DmxModule (modeling/nn/torch_modules.py ReLU through core.py:228-264: input cast, F.relu, output cast) in one pass on
 * the two forms of dmxq_binary_cast: out = cast_out(clamp_min(cast_in(x), 0)).  A third of the traffic of the three launches. */
int dmxq_relu_cast(const void* in, void* out, int dtype, int64_t n, const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out,
                   void* stream);

/* dmxq_binary_cast / dmxq_relu_cast followed by the BFP input cast of the ONE module that consumes the result (a Mul feeding the down
 * projection, a ReLU feeding fc2: each module casts its own input, modeling/nn/core.py:228-264 `input_casts`, so the producer's output
 * is read back once more just to be cast) in the producer's launch: out = BFP_QDQ(module(...)) over blocks of `block_size` along
 * contiguous rows of `row_len` elements (symmetric, nearest, `precision` mantissa bits), bit-identical to the two launches; the two
 * forms of dmxq_binary_cast.  DMXQ_ERR_UNSUPPORTED (the caller runs the two launches): row_len not a whole number of
 * blocks, block_size / (16 bytes of elements) not a power of two <= 64, and what dmxq_binary_cast does not take. */
int dmxq_binary_cast_bfp(const void* a, const void* b, void* out, int dtype, int64_t n, int op, const dmxq_float_fmt* cast_a,
                         const dmxq_float_fmt* cast_b, const dmxq_float_fmt* cast_out, int64_t row_len, int64_t block_size, int precision,
                         void* stream);
int dmxq_relu_cast_bfp(const void* in, void* out, int dtype, int64_t n, const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out,
                       int64_t row_len, int64_t block_size, int precision, void* stream);

/* One operand (q or k) of an ApplyRotaryPosEmb DmxModule (modeling/nn/custom_modules.py:142-194) with the module's casts:
 * out = cast_out(rope(cast_x(x), cast_cos(cos), cast_sin(sin))), rope as dmxq_rope below (torch's op-by-op arithmetic in the
 * tensor dtype).  Replaces, per operand, three input casts, the ~6 torch kernels of the exact function and the output cast.
 * The two forms of dmxq_binary_cast (range-only casts of 16-bit tensors on packed words; anything else per element in fp32). */
int dmxq_rope_cast(const void* x, const void* cos_tab, const void* sin_tab, void* out, int dtype, int64_t B, int64_t n1, int64_t n2,
                   int64_t D, int broadcast_over_dim1, const dmxq_float_fmt* cast_x, const dmxq_float_fmt* cast_cos,
                   const dmxq_float_fmt* cast_sin, const dmxq_float_fmt* cast_out, void* stream);

/* Approximator-slot ops.  The reference evaluates the exact torch.nn.functional op and then overwrites it with a
 * vsimd approximation that lives in a private package (functional/approximate.py:9-14, 300-327); with vsimd
 * absent (the public reference) the exact function is the result, and that is what these compute, in fp32.
 * Replaces: ApproximationMixin.approx_forward for GELU (torch_modules.py GELU), Softmax (torch_modules.py:
 * 989-998, `input_clamp` wrapper argument = input_clamp_min, -INFINITY disables) and LayerNorm (:1062-1082).
 * softmax / layernorm act on the contiguous last dim of a [rows, cols] view. weight/bias may be NULL. */
int dmxq_gelu(const void* in, void* out, int dtype_in, int dtype_out, int64_t n, int tanh_form, void* stream);

/* The other per-element function ids of the approximator slot (src/dmx/compressor/__init__.py:108-139).
 * GELU / GELU_TANH / SILU / EXP: the exact torch function in fp32, rounded once to dtype_out (what the reference computes
 * with vsimd absent, functional/approximate.py:300-304; modules torch_modules.py:1559-1576 SiLU, :236-242 Exp).
 * QUICK_GELU: transformers' QuickGELUActivation `x * sigmoid(1.702 * x)` (modeling/nn/custom_modules.py:112-117),
 * evaluated in the INPUT dtype like torch does (three roundings for 16-bit tensors).
 * SILU_EXPERIMENTAL: the reference's one in-repo approximation, functional/functions.py:7-21
 * `relu(x.to(float16)) * scale` (param = scale; dtype_out must be DMXQ_F16), reproduced bit for bit. */
typedef enum {
  DMXQ_UNARY_GELU = 0, DMXQ_UNARY_GELU_TANH = 1, DMXQ_UNARY_SILU = 2, DMXQ_UNARY_QUICK_GELU = 3, DMXQ_UNARY_EXP = 4,
  DMXQ_UNARY_SILU_EXPERIMENTAL = 5
} dmxq_unary_kind;
int dmxq_unary(const void* in, void* out, int dtype_in, int dtype_out, int64_t n, int kind, float param, void* stream);

/* RMSNorm over the contiguous last dim of a [rows, cols] view: y = x * rsqrt(mean(x^2) + eps) * weight, in fp32,
 * rounded once to dtype_out (torch.nn.functional.rms_norm's CPU result).  Replaces: modeling/nn/torch_modules.py:
 * 1144-1170 RMSNorm._forward -> approx_forward(F.rms_norm).  weight may be NULL. */
int dmxq_rmsnorm(const void* in, void* out, int dtype_in, int dtype_out, int64_t rows, int64_t cols, const void* weight,
                 int dtype_w, float eps, void* stream);
int dmxq_softmax(const void* in, void* out, int dtype_in, int dtype_out, int64_t rows, int64_t cols,
                 float input_clamp_min, void* stream);
int dmxq_layernorm(const void* in, void* out, int dtype_in, int dtype_out, int64_t rows, int64_t cols,
                   const void* weight, const void* bias, int dtype_wb, float eps, void* stream);

/* An activation-function or normalisation DmxModule in ONE pass: out = cast_out(f(cast_in(x))), x and out of one dtype.
 * Replaces the three launches of modeling/nn/core.py:228-264 for the modules whose `_forward` is one of these functions
 * (torch_modules.py GELU / SiLU :1559-1576 / Exp :236-242, custom_modules.py:112-117 QuickGELU, Softmax :989-998, LayerNorm
 * :1062-1082, RMSNorm :1144-1170; both casts are FLOAT16 in BASIC mode, src/dmx/compressor/__init__.py:360-455): input CastTo,
 * the exact torch function (functional/approximate.py:300-304 with vsimd absent), output CastTo -- 4 B/element for a 16-bit
 * tensor instead of 12.  The casts are the bit-exact casts of dmxq_float_qdq with CastTo's `.to(dtype)` after each (formats as
 * in dmxq_binary_cast: NULL or exp_bits == 0 = SAME); f is evaluated in fp32 on the cast input and rounded once to the tensor
 * dtype, as torch evaluates it (QUICK_GELU: in the tensor dtype).  The function is floating point: out == cast_out(v) for a v
 * within 1 ulp of the tensor dtype (16-bit tensors) of the correctly rounded f(cast_in(x)); float32 tensors: within the ulps of
 * the unfused functions before the output cast.
 * DMXQ_ERR_UNSUPPORTED (the caller runs the three launches): 16-bit tensors with a cast that is not range-only for the dtype
 * (bf16: man_bits >= 7, fp16: man_bits >= 10, subnormals flushed); unaligned pointers; n not a whole number of 16-byte
 * vectors; rows that do not take the register-resident row kernels (longer than 1024 lane-vectors, or -- norms -- not a
 * multiple of 4 elements); weight / bias are in the row dtype.  kind: DMXQ_UNARY_GELU .. DMXQ_UNARY_EXP. */
int dmxq_unary_cast(const void* in, void* out, int dtype, int64_t n, int kind, float param, const dmxq_float_fmt* cast_in,
                    const dmxq_float_fmt* cast_out, void* stream);

/* The same module on a 16-bit tensor as a TABLE (csrc/lut16.hip): cast_out(f(cast_in(x))) is a function of the 16 input bits.
 * dmxq_unary_cast_table fills table[p] (65,536 entries of 16 bits, device memory owned by the caller) with the module's result for
 * input PATTERN p: the two casts are the bit-exact casts of dmxq_float_qdq (ANY FloatingPoint format with man_bits <= 22, nearest
 * rounding -- rounding casts too, which dmxq_unary_cast refuses on 16-bit tensors) with CastTo's `.to(dtype)`, and f is evaluated in
 * float64 and rounded ONCE to the tensor dtype: the correctly rounded f(cast_in(x)) (QUICK_GELU: its three roundings in the tensor
 * dtype; DMXQ_UNARY_SILU_EXPERIMENTAL: functional/functions.py:7-21 with scale = param).  dmxq_lut16_apply then computes
 * out[i] = table[in[i]] with the table in the LDS: no arithmetic per element.  dtype: DMXQ_BF16 or DMXQ_F16.  The table is the
 * caller's to keep (one per (function, casts, dtype)); the library holds no state.  dmxq_lut16_apply: DMXQ_ERR_UNSUPPORTED when n
 * is not a whole number of 16-byte vectors or a pointer is not 16-byte aligned. */
int dmxq_unary_cast_table(int dtype, int kind, float param, const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out, void* table,
                          void* stream);
int dmxq_lut16_apply(const void* in, void* out, int64_t n, const void* table, void* stream);
int dmxq_softmax_cast(const void* in, void* out, int dtype, int64_t rows, int64_t cols, float input_clamp_min,
                      const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out, void* stream);
/* ... followed by the NEXT module's BFP input cast of the result (the `input_casts` entry of the ActActMatMul / Linear that consumes the
 * probabilities: modeling/nn/core.py:228-264, numerical/format.py:304-343, blocks of `block_size` along the rows, symmetric, nearest):
 * out = BFP_QDQ(cast_out(softmax(cast_in(x)))) in ONE pass, bit-identical to dmxq_softmax_cast followed by dmxq_bfp_qdq(.., block_size,
 * precision, nearest, symmetric).  The consumer then skips that cast.  DMXQ_ERR_UNSUPPORTED: as dmxq_softmax_cast, or rows that are not
 * whole lane-vectors, or a block size that is not 2^k lane-vectors (16-byte vectors; 8-byte ones for 16-bit rows of 4 k elements). */
int dmxq_softmax_cast_bfp(const void* in, void* out, int dtype, int64_t rows, int64_t cols, float input_clamp_min,
                          const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out, int64_t block_size, int precision, void* stream);
int dmxq_layernorm_cast(const void* in, void* out, int dtype, int64_t rows, int64_t cols, const void* weight, const void* bias,
                        float eps, const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out, void* stream);
int dmxq_rmsnorm_cast(const void* in, void* out, int dtype, int64_t rows, int64_t cols, const void* weight, float eps,
                      const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out, void* stream);
/* The norm modules followed by the (identical) BFP input casts of the modules that consume the result -- the q / k / v Linears after a
 * pre-attention norm, gate / up (fc1) after a pre-MLP norm: `input_casts` of modeling/nn/core.py:228-264 -- in ONE launch, as
 * dmxq_softmax_cast_bfp: out = BFP_QDQ(cast_out(norm(cast_in(x)))), bit-identical to the module's launch followed by dmxq_bfp_qdq. */
int dmxq_layernorm_cast_bfp(const void* in, void* out, int dtype, int64_t rows, int64_t cols, const void* weight, const void* bias,
                            float eps, const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out, int64_t block_size, int precision,
                            void* stream);
int dmxq_rmsnorm_cast_bfp(const void* in, void* out, int dtype, int64_t rows, int64_t cols, const void* weight, float eps,
                          const dmxq_float_fmt* cast_in, const dmxq_float_fmt* cast_out, int64_t block_size, int precision, void* stream);

/* APPLY_LLAMA_ROPE: x_embed = (x * cos) + (rotate_half(x) * sin), evaluated in the tensor dtype like torch does (every
 * product and the sum rounded to the dtype: bit-identical to torch's CPU result).  Replaces: modeling/nn/custom_modules.py:
 * 142-172 ApplyRotaryPosEmbBase.forward for ONE of q / k (call it twice).  x, out: [B, n1, n2, D] contiguous, out != x;
 * cos_tab / sin_tab: [B, n2, D] when broadcast_over_dim1 != 0 (unsqueeze_dim = 1: x = [B, heads, S, D]), else [B, n1, D]
 * (unsqueeze_dim = 2: x = [B, S, heads, D]); all of dtype `dtype`.  DMXQ_ERR_UNSUPPORTED: D not a multiple of two 16-byte
 * vectors, unaligned pointers, >= 2^31 elements (the caller keeps torch's own ops). */
int dmxq_rope(const void* x, const void* cos_tab, const void* sin_tab, void* out, int dtype, int64_t B, int64_t n1, int64_t n2,
              int64_t D, int broadcast_over_dim1, void* stream);

/* GPTQ (optimal brain compression): the in-block column loop of ONE column block, in one launch.
 * Replaces: layer_reconstruction.py:300-318 (per microblock of columns: weight_hypernet of the slice, (w - q) @ inv(Hinv block),
 * slice copies, the update of the block's later columns), i.e. >= 5 launches per column at microblock 1.
 * All float32.  w: the block W[:, i1:i2] (rows x count, row stride ldw; read only); q: Q[:, i1:i2] (row stride ldq); err: the error
 * block E (rows x count, row stride lde); hinv: Hinv[i1:i2, i1:i2] (count x count, row stride ldh, the upper Cholesky factor of H^-1:
 * only its upper triangle is read); inv_d: the inverses of the diagonal microblocks of hinv, ceil(count / microblock) matrices of
 * microblock x microblock (a ragged last one padded with the identity; microblock 1: 1 / hinv[j][j]).  The trailing update
 * W[:, i2:] -= E @ Hinv[i1:i2, i2:] is the caller's (a GEMM).
 * Arithmetic (csrc/gptq.hip): every product and difference separately rounded; microblock 1: q = cast(w_j), e = (w_j - q) * inv_d[j],
 * w_k = w_k - e * hinv[j][k]; microblock m > 1: q = cast(slice), err[c] = sum_i (w - q)[i] * inv_d[i][c] and
 * w_k = w_k - sum_i err[i] * hinv[j1 + i][k], both sums accumulated in index order starting from the i = 0 product.
 * The cast of each microblock slice is bit-identical to the module's weight cast of that [rows, m] slice:
 *   DMXQ_GPTQ_BFP    BFP[precision|8]{block_size} with nearest rounding, symmetric or "(_N)", blocks along the slice's columns
 *                    (block_size >= 2 divides microblock; 2 <= precision <= 22);
 *   DMXQ_GPTQ_FLOAT  FP[..] with nearest rounding (man_bits <= 22), as dmxq_float_qdq;
 *   DMXQ_GPTQ_FIXED  XP[precision, fraction] with nearest rounding and the affine wrapper x / scale + zp -> cast -> (x - zp) * scale,
 *                    scale / zero_point per row (per_row = 1) or one for all rows (per_row = 0).
 * count <= 128; microblock in {1, 8, 16, 32, 64} (BFP: not 1).  DMXQ_ERR_BAD_ARG: null pointers, sizes out of range, strides below
 * count; DMXQ_ERR_UNSUPPORTED: a format, microblock or count outside the above (nothing launched: the caller runs its own loop). */
typedef enum { DMXQ_GPTQ_BFP = 0, DMXQ_GPTQ_FLOAT = 1, DMXQ_GPTQ_FIXED = 2,
               DMXQ_GPTQ_MXFP = 3 /* dmxq_hadamard_qdq only: dmxq_gptq_block and dmxq_cast_error refuse it like any unknown kind */
} dmxq_gptq_kind;
typedef struct {
  int kind;                                                    /* dmxq_gptq_kind */
  int precision, block_size, symmetric;                        /* BFP (precision, block_size, symmetric) and FIXED (precision, symmetric); MXFP: block_size */
  int man_bits, exp_bits, exp_bias, flush_subnormal, unsigned_abs;   /* FLOAT; MXFP: man_bits, exp_bits */
  int fraction, clamp, per_row;                                /* FIXED */
} dmxq_gptq_format;
int dmxq_gptq_block(const float* w, int64_t ldw, float* q, int64_t ldq, float* err, int64_t lde, int64_t rows, int64_t count,
                    const float* hinv, int64_t ldh, const float* inv_d, int64_t microblock, const dmxq_gptq_format* fmt,
                    const float* scale, const int64_t* zero_point, void* stream);

/* dmxq_gptq_block with DYNAMIC per-group integer scales (csrc/gptq_dynamic.hip): the scale of a group of `group` input
 * columns is found while the column loop runs, from the row's current, already error-compensated values.  Not in the reference, whose
 * group quantisation groups output channels and whose GPTQ reads scales that a calibration run fixed.
 * Arguments as dmxq_gptq_block's with fmt->kind == DMXQ_GPTQ_FIXED (per_row is ignored: every row has its own scales), plus the
 * format's rounding, and qmin / qmax / symmetric_qscheme as dmxq_qparams takes them.  Per row, with w the row's block as the loop
 * updates it:
 *   at every column j with j % group == 0, before the microblock that starts there is cast:
 *     (mn, mx)  dmxq_group_minmax of the float32 values w[j .. j + group) as they stand at that moment (the updates of all earlier
 *               microblocks and -- through the caller's trailing updates -- earlier blocks included; one NaN makes both NaN);
 *     (sc, zp)  dmxq_qparams(mn, mx, qmin, qmax, symmetric_qscheme), in its float32 operations;
 *     scale_out[row * lds + j / group] = sc, zp_out[row * ldz + j / group] = zp  (DEVICE arrays [rows, count / group]);
 *   every column of the group is cast with that (sc, zp) exactly as DMXQ_GPTQ_FIXED casts with a per-row scale:
 *   (cast(w / sc + zp) - zp) * sc with IEEE division and nearest rounding.
 * Everything else -- the inv_d products, the update of the later columns, q and err -- is dmxq_gptq_block's, in its order.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its own loop): group not in {16, 32, 64, 128}; count % group != 0 or
 * group % microblock != 0 (a microblock never straddles a group; microblock == group is allowed); count > 128; microblock not in
 * {1, 8, 16, 32, 64}; rounding other than nearest; fraction != 0; no clamp; precision outside 1 .. 22.
 * DMXQ_ERR_BAD_ARG: dmxq_gptq_block's rules, a kind other than DMXQ_GPTQ_FIXED, an invalid rounding, group < 1, qmax <= qmin, null
 * scale_out / zp_out, lds or ldz below count / group.  No workspace, no allocation, no host synchronisation: capturable. */
int dmxq_gptq_block_dynamic(const float* w, int64_t ldw, float* q, int64_t ldq, float* err, int64_t lde, int64_t rows, int64_t count,
                            const float* hinv, int64_t ldh, const float* inv_d, int64_t microblock, const dmxq_gptq_format* fmt,
                            int rounding, int64_t group, int qmin, int qmax, int symmetric_qscheme, float* scale_out, int64_t lds,
                            int64_t* zp_out, int64_t ldz, void* stream);

/* HistogramObserver on the device, for G = ceil(C / group_size) groups at once (slabs of group_size channels of the [outer, C, inner]
 * view, as dmxq_group_minmax; per tensor: outer = C = 1, inner = n, group_size = 1).  csrc/hist_observer.hip; DESIGN.md §3.
 * dmxq_hist_observe replaces numerical/observer.py:453-510 HistogramObserver.forward (min / max, torch.histc, the merge onto the
 * running range, observer.py:400-458 re-binning) and the per-slab loop of numerical/cast.py:185-213; dmxq_hist_qparams replaces
 * observer.py:331-397 _search_range and 59-115 _calculate_qparams.  Bit for bit the host code of dmx-compressor_amd/observer.py, save the
 * two sums that ATen leaves unordered (torch.sum(hist), err.sum()): here fp64 in a fixed order, rounded once.
 * State (caller-allocated, device, float32 unless said): hist [G, bins] and min_val / max_val [G] -- +inf / -inf before the first
 * observation --, status: one int, 0 at first, raised to 1 (an infinite extremum: int(inf) raises OverflowError on the host) or 2 (a NaN:
 * ValueError) by an observation that the host code would have refused; such a group's state is left unchanged.
 * scratch: >= (2 + bins) * G * 4 bytes of device memory, contents free (scratch_bytes: its size).  bins <= 8192, upsample_rate <= 2^20.
 * No host synchronisation, no allocation: both calls can be captured into a graph.  n == 0 changes nothing.
 * dmxq_hist_qparams: levels = 2^precision; a group with min_val = +inf, max_val = -inf gets (1, 0). */
int dmxq_hist_observe(const void* in, int dtype_in, int64_t outer, int64_t C, int64_t inner, int64_t group_size, int64_t bins,
                      int64_t upsample_rate, float* hist, float* min_val, float* max_val, int* status, void* scratch, int64_t scratch_bytes,
                      void* stream);
int dmxq_hist_qparams(const float* hist, const float* min_val, const float* max_val, int64_t n_groups, int64_t bins, int precision, int qmin,
                      int qmax, int symmetric_qscheme, float* scale, int64_t* zero_point, void* stream);

/* Quantization-error statistics on the device (csrc/error_stats.hip).  Replaces utils/benchmark.py:349-389
 * compute_mse_error / compute_maxdelta_error (per tensor pair one mse_loss, one abs().max() and two .item() synchronisations) and, for a
 * comparison of K formats on one tensor, K casts followed by 2 K torch reductions over temporaries.
 * A row of statistics is double[4] in device memory: [sum_sq_err, sum_sq_ref, max_abs_err, count] for a reference r and a test t of n
 * elements, with d = float(r) - float(t) (one fp32 subtraction): sum_sq_err = sum d^2 and sum_sq_ref = sum float(r)^2, every square
 * formed exactly in fp64 and summed in fp64; max_abs_err = torch's (r - t).float().abs().max(), i.e. the largest |d| rounded to the
 * promoted dtype of the pair (the dtype itself when both agree, else float32); count = n.  mse = row[0] / row[3],
 * sqnr_db = 10 log10(row[1] / row[0]).  A NaN difference makes sum_sq_err and max_abs_err NaN.  No floating-point atomics: the same
 * input twice gives the same bits.  accumulate != 0 merges into the row already in `stats` (sums add, max takes the max, count adds),
 * so statistics run over many batches without a host read.  scratch: dmxq_error_scratch_bytes(n, n_formats) bytes of device memory,
 * 8-byte aligned, contents free.  No allocation, no host synchronisation: both calls can be captured into a graph.  n == 0 writes the
 * identity row [0, 0, 0, 0], or with accumulate leaves the row unchanged (nothing launched).
 * dmxq_error_stats: ref / test of any dtype pair; 16-byte aligned pointers take the vector loads, others an element-wise kernel.
 * dmxq_cast_error: `in` is [rows, L] contiguous and is read ONCE; row k of stats (double[n_formats][4]) is the row of dmxq_error_stats
 * between `in` and the library's cast of that [rows, L] tensor to formats[k] -- blocks along L, the result rounded to `dtype` as
 * CastTo.forward returns it -- bit for bit in count and max_abs_err (the sums differ only by the order of an fp64 sum).  Nothing is
 * written but the statistics.  formats: a HOST array of dmxq_gptq_format with per_row = 0:
 *   DMXQ_GPTQ_BFP    nearest rounding, symmetric or "(_N)", 2 <= precision <= 22, block_size in {8, 16, 32, 64, 128} dividing L;
 *   DMXQ_GPTQ_FLOAT  nearest rounding, man_bits <= 22;
 *   DMXQ_GPTQ_FIXED  nearest rounding with the affine wrapper, scale[k] / zero_point[k] (DEVICE arrays indexed like formats; may be NULL
 *                    without a FIXED format).
 * Status: DMXQ_ERR_BAD_ARG for an invalid dtype or format kind, n_formats < 1, or a scratch smaller than the query says;
 * DMXQ_ERR_UNSUPPORTED, nothing launched, for everything else these entry points do not take -- a null pointer or a negative size,
 * more than 8 formats, a format or block size outside the list, L % 8 != 0 or a block size that does not divide L, a misaligned
 * pointer (dmxq_cast_error: `in` not 16-byte aligned): the caller then runs the library's cast followed by dmxq_error_stats. */
int64_t dmxq_error_scratch_bytes(int64_t n, int n_formats);
int dmxq_error_stats(const void* ref, int dtype_ref, const void* test, int dtype_test, int64_t n, int accumulate, double* stats,
                     void* scratch, int64_t scratch_bytes, void* stream);
int dmxq_cast_error(const void* in, int dtype, int64_t rows, int64_t L, const dmxq_gptq_format* formats, int n_formats,
                    const float* scale, const int64_t* zero_point, int accumulate, double* stats, void* scratch, int64_t scratch_bytes,
                    void* stream);

/* Orthonormal block-Hadamard rotation fused into a quantize-dequantize cast (csrc/hadamard.hip).  Not in the reference:
 * the rotate -> quantize -> rotate back companion of the 4- to 8-bit block formats (QuaRot, SpinQuant, the MXFP4 training recipes), one
 * read and one write per element instead of a dense [size, size] matmul and two more passes around the cast.
 * in / out: [rows, L] contiguous; blocks of `size` consecutive elements along L; size in {8, 16, 32, 64, 128, 256}, L % size == 0.
 * R (one block, widened to fp32): butterfly stages of stride s = 1, 2, .., size / 2 in that order -- for every i with bit s clear
 * v[i], v[i + s] = v[i] + v[i + s], v[i] - v[i + s] from the old values, each ONE fp32 operation -- then ONE fp32 multiply by
 * (float)(1 / sqrt((double)size)).  R is symmetric and orthonormal: its own inverse.  NaN / Inf propagate through the adds.
 *   fmt == NULL            out = round_to(dtype_out, R(x))  (inverse must be 0)
 *   fmt, inverse == 0      out = round_to(dtype_out, Q(R(x)))
 *   fmt, inverse != 0      out = round_to(dtype_out, R(Q(R(x))))
 * Q: the library's cast of the rotated FLOAT32 tensor to fmt, float32 in and out, blocks along L, nearest rounding -- bit for bit
 * dmxq_bfp_qdq / dmxq_float_qdq / dmxq_fixed_qdq / dmxq_mxfp_qdq on that tensor; ONE rounding to dtype_out at the very end.
 *   DMXQ_GPTQ_BFP    symmetric or "(_N)", 2 <= precision <= 22, block_size a power of two >= 2 dividing size;
 *   DMXQ_GPTQ_FLOAT  man_bits <= 22;
 *   DMXQ_GPTQ_FIXED  the affine wrapper x / scale + zp -> cast -> (x - zp) * scale; per_row = 0: scale[0] / zero_point[0],
 *                    per_row = 1: scale[rows] / zero_point[rows] (DEVICE arrays);
 *   DMXQ_GPTQ_MXFP   man_bits <= 22, exp_bits, block_size a power of two dividing size (dmxq_mxfp_qdq's float32 rules, its
 *                    floor(log2 max) rule near powers of two included; zero blocks stay zero).
 * in == out is allowed when both dtypes have one width (every block is fully read before any of it is written); pointers need not be
 * 16-byte aligned (such a call loads and stores element by element).  No allocation, no host synchronisation: the call can be captured
 * into a graph.  DMXQ_ERR_BAD_ARG: null pointers, negative sizes, an invalid dtype or kind, inverse without a format, in == out with
 * dtypes of different widths; DMXQ_ERR_UNSUPPORTED, nothing launched: a size outside the list, L % size != 0, a format or block size
 * outside the above (the caller runs rotation, cast and rotation as three launches). */
int dmxq_hadamard_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t rows, int64_t L, int64_t size, int inverse,
                      const dmxq_gptq_format* fmt, const float* scale, const int64_t* zero_point, void* stream);

/* Dynamic integer cast (csrc/dynamic_quant.hip): every segment of `segment` consecutive elements of the contiguous
 * [n_segments, segment] tensor takes its scale and zero point from its OWN minimum and maximum, on every call, in ONE launch.  Not in
 * the reference (its integer casts read what a calibration run stored); the arithmetic is the reference's, applied per call:
 *   (mn, mx)     the segment's extrema as dmxq_group_minmax reports them (one NaN makes both NaN, which the next step's fminf / fmaxf drop);
 *   (scale, zp)  dmxq_qparams(mn, mx, qmin, qmax, symmetric_qscheme)  (numerical/observer.py:59-115);
 *   out          dmxq_fixed_qdq with that one (scale, zp) per segment  (numerical/cast.py:278-296), nearest rounding.
 * Bit for bit that three-launch chain, scale_out / zp_out included (each NULL, or a DEVICE array of n_segments entries).
 * whole_rows != 0: the segments are the rows of the caller's tensor (per token / per output channel) -- any segment % V == 0 up to
 * 16384, V = 8 sixteen-bit or 4 fp32 elements; whole_rows == 0: groups inside rows -- a power of two from 16 to 256 only.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs the chain): dtype_in != dtype_out, a segment outside the above, a base that
 * is not 16-byte aligned, rounding other than nearest, fraction != 0, no clamp, precision > 22.  DMXQ_ERR_BAD_ARG: null data
 * pointers, negative sizes, invalid dtype / rounding, qmax <= qmin.  No workspace, no allocation, no host synchronisation: capturable. */
/* The launch geometry dmxq_dynamic_fixed_qdq picks for segments of `segment` elements of `dtype` (no GPU involved; the same function
 * makes the choice inside the entry): NONE = refused (DMXQ_ERR_UNSUPPORTED), GROUP = power-of-two segments of 16 .. 256 inside a wave,
 * SHORT_ROW = a wave per row of fewer than 64 vectors (lanes idle), WAVE_ROW = a wave per row of 64 .. 1024 vectors, BLOCK_ROW = a
 * 256-thread workgroup per row; TILE (dmxq_dynamic_float_class only) = a g x g tile per wave or workgroup.  Returns the enum value, not
 * a status. */
typedef enum { DMXQ_DYN_NONE = 0, DMXQ_DYN_GROUP = 1, DMXQ_DYN_SHORT_ROW = 2, DMXQ_DYN_WAVE_ROW = 3, DMXQ_DYN_BLOCK_ROW = 4,
               DMXQ_DYN_TILE = 5 } dmxq_dynamic_geometry;
int dmxq_dynamic_class(int dtype, int64_t segment, int whole_rows);
int dmxq_dynamic_fixed_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_segments, int64_t segment, int whole_rows,
                           int precision, int fraction, int clamp, int symmetric, int rounding, int qmin, int qmax,
                           int symmetric_qscheme, float* scale_out, int64_t* zp_out, void* stream);

/* Learned step size (LSQ, Esser et al. 2020; LSQ+, Bhalgat et al. 2020): the BACKWARD pass of an integer cast whose scale s and float zero
 * point z are trained (csrc/lsq.hip; DESIGN.md §8 "Learned step size").  Not in the reference, whose casts are identity straight-through
 * estimators.  The forward is dmxq_fixed_qdq with one (s, zq) per segment, zq = clamp(rint(z), qmin, qmax).  x, g, dx: the contiguous
 * [n_segments, segment] tensor, the incoming gradient and the gradient of x, one dtype; scale, zero_point: DEVICE float32 [n_segments];
 * ds, dz: DEVICE float32 [n_segments] outputs.  Per element, every operation fp32 in this order:
 *   v = x / s + zq (IEEE division);  r = the forward's nearest rounding of v;  in = qmin <= r <= qmax;  q = clamp(r, qmin, qmax);
 *   dx = in ? g : 0;  e = in ? q - v : q - zq;  ts = g * e;  tz = in ? 0 : -(g * s)
 * and per segment ds = (float)(grad_factor * sum (double)ts), dz = (float)(grad_factor * sum (double)tz): float64 sums without
 * floating-point atomics, in an order that depends on the shape alone (the same call twice gives the same bits).  A NaN x gives
 * dx = 0 there and a NaN ds for its segment; a NaN g gives a NaN ds and is passed on as dx where the element is `in`.
 * want_dz == 0: tz is not formed and dz not written (may be NULL).  dx == NULL: dx is not stored.
 * whole_rows: 0 -- groups inside rows, a power of two from 16 to 256; 1 -- rows, any multiple of a 16-byte vector (8 sixteen-bit or
 * 4 fp32 elements) up to 16384; 2 -- the whole tensor as ONE segment (n_segments <= 1) of any whole number of vectors: workgroups write
 * float64 partial rows into `scratch` (dmxq_lsq_scratch_bytes(segment) bytes of device memory, 8-byte aligned, contents free; unused
 * and may be NULL otherwise) and a second small launch folds them in a fixed order.
 * dmxq_lsq_class: the geometry the entry picks (dmxq_dynamic_geometry, or DMXQ_LSQ_TENSOR under whole_rows == 2), DMXQ_DYN_NONE where
 * it refuses; dmxq_lsq_scratch_bytes: both host functions, no GPU involved.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain of torch operations): dtypes that differ, a segment outside the
 * above or not whole vectors, x / g / dx not 16-byte aligned, rounding other than nearest, precision > 22, no scratch for the
 * tensor class.  DMXQ_ERR_BAD_ARG: null pointers, negative sizes, invalid dtype / rounding / whole_rows, qmax <= qmin, more than one
 * segment under whole_rows == 2, a scratch smaller than the query says.  No allocation, no host synchronisation: capturable. */
typedef enum { DMXQ_LSQ_TENSOR = 6 } dmxq_lsq_geometry;
int dmxq_lsq_class(int dtype, int64_t segment, int whole_rows);
int64_t dmxq_lsq_scratch_bytes(int64_t n);
int dmxq_lsq_backward(const void* x, const void* g, void* dx, int dtype_x, int dtype_g, int dtype_dx, int64_t n_segments, int64_t segment,
                      int whole_rows, int precision, int rounding, int qmin, int qmax, const float* scale, const float* zero_point,
                      double grad_factor, int want_dz, float* ds, float* dz, void* scratch, int64_t scratch_bytes, void* stream);

/* Dynamic SCALED float cast (csrc/dynamic_float.hip): every segment of the contiguous tensor is scaled by its OWN absolute
 * maximum, on every call, in ONE launch -- per token, per group, per 2-D tile (the FP8 recipe's activations and weights).  Not in the
 * reference, whose float casts are unscaled; the per-element arithmetic is dmxq_float_qdq's.  The format is the SIGNED float
 * (man_bits, exp_bits < 8, exp_bias, flush_subnormal) with largest output fmax = 2^(2^(exp_bits-1)) (2 - 2^-man_bits).  Per segment, in fp32:
 *   amax = max |x| (one NaN anywhere makes it NaN);  s = amax / fmax (IEEE);
 *   pow2_scale != 0: s rounded UP to a power of two on its bits, b = (b & 0x7F800000) + ((b & 0x007FFFFF) ? 0x00800000 : 0);
 *   s = 1 when s is not finite or below 2^-126 (an all-zero, a NaN, an Inf segment);
 *   out = float_q(x / s) * s: IEEE quotient, the format's nearest cast (flush flag kept, NaN / Inf saturate as in dmxq_float_qdq), one
 *   fp32 multiply, one rounding to dtype_out.
 * mode: DMXQ_DYNF_GROUP -- n_segments groups of `segment` consecutive elements, a power of two from 16 to 256; DMXQ_DYNF_ROWS --
 * n_segments rows of `segment` elements, any multiple of a 16-byte vector (8 sixteen-bit or 4 fp32 elements) up to 16384 (rows, cols
 * unused in both); DMXQ_DYNF_TILE -- the [rows, cols] matrix in segment x segment tiles, segment = 32, 64 or 128 dividing both (leading
 * batch dims fold into rows), n_segments = (rows / segment) (cols / segment), tile t = (row tile) * (cols / segment) + (column tile).
 * scale_out: NULL or a DEVICE array of n_segments floats, the s of every segment.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain of launches): dtype_in != dtype_out, rounding other than nearest, a
 * base that is not 16-byte aligned, a segment outside the above, man_bits > 22.  DMXQ_ERR_BAD_ARG: null data pointers, negative sizes,
 * invalid dtype / rounding / mode, exp_bits outside 1 .. 7 (8: fp32's exponent range has no finite maximum), a tile size that does not
 * divide rows and cols or an n_segments that is not their tile count.  No workspace, no allocation, no host synchronisation: capturable.
 * dmxq_dynamic_float_class: the geometry (dmxq_dynamic_geometry) the entry picks for `segment` under `mode`, no GPU involved. */
typedef enum { DMXQ_DYNF_GROUP = 0, DMXQ_DYNF_ROWS = 1, DMXQ_DYNF_TILE = 2 } dmxq_dynamic_float_mode;
int dmxq_dynamic_float_class(int dtype, int mode, int64_t segment);
int dmxq_dynamic_float_qdq(const void* in, void* out, int dtype_in, int dtype_out, int mode, int64_t n_segments, int64_t segment,
                           int64_t rows, int64_t cols, int man_bits, int exp_bits, int exp_bias, int flush_subnormal, int rounding,
                           int pow2_scale, float* scale_out, void* stream);

/* Codebook casts (csrc/codebook.hip; DESIGN.md §8 "Codebook casts"): a small table of ARBITRARY levels under a per-segment absolute-maximum
 * scale -- NF4, Lloyd-Max / k-means tables -- in ONE launch, and the weighted Lloyd statistics that fit a table on the device.  Not in
 * the reference.  levels: a DEVICE array of K float32 levels, non-decreasing (never read back, taken as is); the kernels derive, in fp32,
 * the thresholds t_j = (c_j + c_{j+1}) * 0.5f, the zero level z (the lowest index of the level with the smallest |c|) and, for
 * norm <= 0, norm = max(|c_0|, |c_{K-1}|).  Per segment of the contiguous tensor, in fp32:
 *   amax = max |x| (one NaN anywhere makes it NaN);  s = amax / norm (IEEE);  s = 1 when s is not finite or below 2^-126;
 *   u = x / s (IEEE);  idx = #{ j : u > t_j } (a tie goes to the lower level; a NaN u takes idx = z);  out = c[idx] * s, one fp32
 *   multiply, one rounding to dtype_out.
 * mode: DMXQ_DYNF_GROUP -- n_segments groups of `segment` consecutive elements, a power of two from 16 to 256; DMXQ_DYNF_ROWS --
 * n_segments rows of `segment` elements, any multiple of a 16-byte vector up to 16384.  scale_out: NULL or a DEVICE array of n_segments
 * floats; index_out: NULL or a DEVICE array of one uint8 per element, 16-byte aligned.
 * dmxq_codebook_accumulate: the Lloyd statistics of the same (scale, u, idx), float64 acc[K][3]: over the elements whose u is finite,
 * acc[idx] (+)= { w u, w, 1 } with w = (double)s * (double)s; accumulate != 0 adds to acc, 0 overwrites it.  No floating-point atomics, a
 * fixed order: the same input gives the same bits.  workspace: DEVICE memory of dmxq_codebook_workspace_bytes(...) bytes, 8-byte
 * aligned, contents free.  An empty tensor launches nothing and leaves acc as it is.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain): dtype_in != dtype_out, K > 16, a segment outside the above, a base
 * that is not 16-byte aligned.  DMXQ_ERR_BAD_ARG: null pointers, negative sizes, invalid dtype / mode (tiles are not taken), K outside
 * 2 .. 256, a norm that is NaN or +Inf.  No allocation, no host synchronisation: capturable.
 * dmxq_codebook_class: the geometry (dmxq_dynamic_geometry) the entries pick for `segment` under `mode`, no GPU involved. */
int dmxq_codebook_class(int dtype, int mode, int64_t segment);
int dmxq_codebook_qdq(const void* in, void* out, int dtype_in, int dtype_out, int mode, int64_t n_segments, int64_t segment,
                      const float* levels, int K, float norm, float* scale_out, uint8_t* index_out, void* stream);
int64_t dmxq_codebook_workspace_bytes(int dtype, int mode, int64_t n_segments, int64_t segment);
int dmxq_codebook_accumulate(const void* in, int dtype_in, int mode, int64_t n_segments, int64_t segment, const float* levels, int K,
                             float norm, double* acc, int accumulate, void* workspace, void* stream);

/* Vector codebook casts (csrc/vq.hip; DESIGN.md §8 "Vector codebook casts", whose text is the contract): `dim` consecutive elements are
 * replaced together by one row of a [K, dim] table under a per-segment absolute-maximum scale -- GPTVQ / AQLM / QuIP#-style tables -- in
 * ONE launch, and the weighted k-means statistics that fit such a table on the device.  Not in the reference.  table: a DEVICE array of
 * K * dim float32 entries, row-major, finite (never read back, taken as is), 2 <= K <= 256, dim 2, 4 or 8; no order is required and
 * duplicate rows are allowed.  In fp32, every operation rounded on its own:
 *   D_k(u) = (((t_0 t_0) + t_1 t_1) + ...) + t_{dim-1} t_{dim-1}, t_j = u_j - c_kj;  z = the lowest k minimising D_k(0);  for norm <= 0,
 *   norm = max |c_kj|.  Per segment: amax, s = amax / norm and the fallback s = 1 as dmxq_codebook_qdq;  u = x / s (IEEE);  per
 *   dim-vector: best = +Inf, idx = z, for k = 0 .. K-1: D_k(u) < best takes k (a tie keeps the lower index; a vector whose distances
 *   are all NaN or +Inf takes z);  out_j = c[idx][j] * s, one fp32 multiply, one rounding to dtype_out.
 * mode and segment: as dmxq_codebook_qdq; `segment` is a multiple of dim, so that a vector never straddles a segment.  scale_out: NULL or
 * a DEVICE array of n_segments floats; index_out: NULL or a DEVICE array of one uint8 per dim-vector (n_segments * segment / dim),
 * 16-byte aligned.
 * dmxq_vq_accumulate: float64 acc[K][dim + 2]: over the vectors whose dim quotients are all finite, acc[idx] (+)= { w u_0, ...,
 * w u_{dim-1}, w, 1 } with w = (double)s * (double)s; accumulate != 0 adds to acc, 0 overwrites it.  No floating-point atomics: a row's
 * owner thread adds its vectors in a fixed slot order, workgroups write partial blocks, a second launch adds the blocks in workgroup
 * order (csrc/vq.hip's header) -- the same input gives the same bits.  workspace: DEVICE memory of dmxq_vq_workspace_bytes(...) bytes,
 * 8-byte aligned, contents free.  An empty tensor launches nothing and leaves acc as it is.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain): dtype_in != dtype_out, float32 with dim 8, a segment outside
 * dmxq_codebook_qdq's, a base that is not 16-byte aligned.  DMXQ_ERR_BAD_ARG: null pointers, negative sizes, invalid dtype / mode, dim
 * outside {2, 4, 8}, a segment that is no multiple of dim, K outside 2 .. 256, a norm that is NaN or +Inf.  No allocation, no host
 * synchronisation: capturable.
 * dmxq_vq_class: the geometry (dmxq_dynamic_geometry) the entries pick, DMXQ_DYN_NONE where they refuse; no GPU involved. */
int dmxq_vq_class(int dtype, int mode, int64_t segment, int dim, int K);
int dmxq_vq_qdq(const void* in, void* out, int dtype_in, int dtype_out, int mode, int64_t n_segments, int64_t segment, const float* table,
                int dim, int K, float norm, float* scale_out, uint8_t* index_out, void* stream);
int64_t dmxq_vq_workspace_bytes(int dtype, int mode, int64_t n_segments, int64_t segment, int dim, int K);
int dmxq_vq_accumulate(const void* in, int dtype_in, int mode, int64_t n_segments, int64_t segment, const float* table, int dim, int K,
                       float norm, double* acc, int accumulate, void* workspace, void* stream);

/* Half-Quadratic Quantization (HQQ; Badri and Shaji, 2023) in ONE launch (csrc/hqq.hip; DESIGN.md §8 "HQQ", whose text is the contract).
 * Not in the reference.  Per group of `segment` consecutive elements of the contiguous tensor, every operation fp32 in the text's order:
 *   (mn, mx) the extrema with dmxq_group_minmax's NaN rule;  s = (mx - mn) / (qmax - qmin), 1 when not finite or below 2^-126;
 *   rs = 1 / s;  z_0 = qmin - mn * rs (a float, not rounded);  then `iters` proximal steps on z under the l_p norm (lp_norm) with
 *   beta_k = beta * kappa^k, the group keeping the z whose L1 error sum |x - (q - z) s| was smallest (strictly; z_0 at a tie or a NaN);
 *   q = clamp(rint(x * rs + z_best), qmin, qmax);  out = (q - z_best) * s, one rounding to dtype_out.
 * The sums over a group are adjacent-pair trees.  scale_out, zero_out: NULL or DEVICE arrays of n_segments floats (s, z_best);
 * codes_out: NULL or a DEVICE array of one uint8 per element, 8-byte aligned: q - qmin (0 where q is NaN), qmax - qmin <= 255.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain): a segment that is no power of two from 16 to 256, dtype_in !=
 * dtype_out, a base that is not 16-byte aligned, rounding other than nearest, lp_norm other than 0.5 or 1, an integer range of 2^22 or
 * more.  DMXQ_ERR_BAD_ARG: null data pointers, negative sizes or iters, invalid dtype / rounding, qmax <= qmin, lp_norm outside (0, 1],
 * beta <= 0, kappa < 1, codes_out with a range above 255.  No workspace, no allocation, no host synchronisation: capturable.
 * dmxq_hqq_class: DMXQ_DYN_GROUP where the entry takes groups of `segment` elements of `dtype`, DMXQ_DYN_NONE otherwise; no GPU involved. */
int dmxq_hqq_class(int dtype, int64_t segment);
int dmxq_hqq_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_segments, int64_t segment, int rounding, int qmin, int qmax,
                 float lp_norm, float beta, float kappa, int iters, float* scale_out, float* zero_out, uint8_t* codes_out, void* stream);

/* Outlier-aware dynamic integer cast in ONE launch (csrc/outlier_quant.hip; DESIGN.md §8 "Outlier-aware dynamic cast", whose text is the
 * contract; SpQR, Dettmers et al. 2023; SqueezeLLM, Kim et al. 2023).  Not in the reference.  Per group of `segment` consecutive elements
 * of the contiguous tensor:
 *   rank     by the bit pattern of |x| as float32 (a NaN above Inf above every finite value), equal patterns to the LOWER index; the
 *            first k are the group's outliers;
 *   inliers  the group with +0.0 in the outliers' places through dmxq_dynamic_fixed_qdq's arithmetic, (scale, zero point) included:
 *            qparams take min(mn, 0) / max(mx, 0), so they are those of the other elements alone;
 *   outliers O(x) in their places: the input's own bits (outlier_format NULL or exp_bits == 0), or the nearest cast to the signed float
 *            format as dmxq_float_qdq computes it, rounded once to the tensor's dtype.
 * scale_out / zp_out: each NULL, or a DEVICE array of n_segments entries.  idx_out (int32) and val_out (the tensor's dtype): both NULL, or
 * DEVICE arrays of n_segments * k entries, 4-byte aligned: the outliers' positions in the group and O(x), in rank order.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain): k outside 1 .. 8, a segment that is no power of two from 16 to
 * 256, dtype_in != dtype_out, a base that is not 16-byte aligned, rounding other than nearest, fraction != 0, no clamp, precision > 22,
 * an outlier format outside 1 .. 8 exponent and 0 .. 22 mantissa bits.  DMXQ_ERR_BAD_ARG: null data pointers, negative sizes, invalid
 * dtype / rounding, qmax <= qmin, k < 0 or k >= segment, one of idx_out / val_out without the other.  No workspace, no allocation, no
 * host synchronisation: capturable.
 * dmxq_outlier_class: DMXQ_DYN_GROUP where the entry takes groups of `segment` elements of `dtype`, DMXQ_DYN_NONE otherwise; no GPU involved. */
int dmxq_outlier_class(int dtype, int64_t segment);
int dmxq_outlier_fixed_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_segments, int64_t segment, int k, int precision,
                           int fraction, int clamp, int symmetric, int rounding, int qmin, int qmax, int symmetric_qscheme,
                           const dmxq_float_fmt* outlier_format, float* scale_out, int64_t* zp_out, int32_t* idx_out, void* val_out,
                           void* stream);

/* Wanda (Sun et al., 2023): activation-aware N:M pruning calibrated on the device (csrc/wanda.hip; DESIGN.md §8 "Wanda").  Not in the
 * reference.  For a Linear weight W[rows, L] and calibration inputs X[n_tokens, L]:
 *   sumsq[j] = sum_t (double)X[t, j]^2 in float64 over every observed batch;  act_norm = (float)sqrt(sumsq) (formed by the caller);
 *   score = |(float)W| * act_norm, one fp32 multiply;  mask and y = W * mask by the rule of dmxq_nm_mask on that score.
 *
 * dmxq_channel_sumsq_accumulate: acc[c] += sum over the rows of the contiguous [rows, C] tensor of (double)x^2, c < C.  acc: DEVICE
 * float64 [C], zeroed by the caller before the first batch.  Every product is formed in double (exact for fp32 and 16-bit inputs) and
 * added by one fp64 fma; no floating-point atomics and a fixed order -- a channel's rows in index order inside a slab of rows, the
 * slabs in slab order, then one addition into acc; the slab partition depends on (rows, C) alone -- so the same batches in the same
 * order give the same bits, whatever the dtype or the alignment.  workspace: DEVICE memory of dmxq_channel_sumsq_workspace_bytes(rows, C)
 * bytes (8-byte aligned; a host query, no GPU involved; 0 for an empty tensor), overwritten by every call.  Lanes move 16-byte vectors
 * when C is a multiple of 8 (16-bit) or 4 (fp32) elements and `in` is 16-byte aligned, and single elements otherwise: same order, same
 * bits.  No allocation, no host synchronisation: capturable.  DMXQ_ERR_BAD_ARG: invalid dtype, negative sizes, null pointers. */
int64_t dmxq_channel_sumsq_workspace_bytes(int64_t rows, int64_t C);
int dmxq_channel_sumsq_accumulate(const void* in, int dtype_in, int64_t rows, int64_t C, double* acc, void* workspace, void* stream);
/* dmxq_wanda_nm: ONE pass over the contiguous weight w[rows, L]; act_norm: DEVICE float32 [L].  A lane forms the scores of 8 (M <= 8)
 * or 16 (M = 16) consecutive elements in registers, ranks every group of M along L as dmxq_nm_mask does (ascending, stable, the lower
 * index zeroed first among ties, NaN highest, -0 == +0; the K highest of a group are kept) and writes what is not NULL: score_out
 * (float32 [rows, L]), mask_out (0 / 1 in dtype_mask), y_out (w * mask in dtype_y: a real multiply, a masked negative weight gives
 * -0.0).  K = M = 0: the score only (score_out required, the other two NULL).  A zero norm scores 0 and an overflowing product Inf
 * (both tie by index), a NaN norm makes its column rank highest: no special case anywhere.
 * dmxq_wanda_class(dtype_w, L, M): 1 where the kernel takes the geometry -- M in {0, 4, 8, 16} and L a multiple of 16 -- else 0; a
 * host function, no GPU involved.  DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs the chain |w| * act_norm -> dmxq_nm_mask,
 * same bits): class 0, or a pointer that is not 16-byte aligned.  DMXQ_ERR_BAD_ARG: invalid dtypes, negative sizes, K > M, K < 1 with
 * M > 0, M > 64, L % M != 0, all three outputs NULL, null w / act_norm.  No workspace, no allocation, no host synchronisation. */
int dmxq_wanda_class(int dtype_w, int64_t L, int M);
int dmxq_wanda_nm(const void* w, int dtype_w, const float* act_norm, float* score_out, void* mask_out, int dtype_mask, void* y_out,
                  int dtype_y, int64_t rows, int64_t L, int K, int M, void* stream);

/* AWQ (Lin et al., 2023): activation-aware weight scaling searched on the device (csrc/awq.hip, csrc/wanda.hip; DESIGN.md §8 "AWQ").
 * Not in the reference.  The search evaluates, for candidate per-input-channel scale vectors s, the error D = Q(W s) / s - W of the
 * module's own weight cast against the calibration inputs' second moment.
 *
 * dmxq_channel_sumabs_accumulate: the |x| twin of dmxq_channel_sumsq_accumulate -- acc[c] += sum over the rows of (double)|x|, one
 * kernel body with the per-element term as a template argument: the same workspace query (dmxq_channel_sumsq_workspace_bytes), slab
 * partition, summation order, vector / scalar lane forms and status codes.  Capturable.
 *
 * dmxq_awq_group_error: ONE candidate in ONE launch over the contiguous weight w[rows, L] of dtype_w; s: DEVICE float32 [L].  Per
 * element, with column = element index mod L:
 *   ws = dtype_w(fp32(w) * s[column])  ->  wq = the per-group dynamic integer cast of dmxq_dynamic_fixed_qdq on ws (groups of `group`
 *   consecutive elements, nearest rounding, (qmin, qmax, symmetric_qscheme) as there; the same device code), one rounding to dtype_w
 *   ->  d = fp32(wq) / s[column] - fp32(w), one IEEE division and one subtraction in fp32.
 * d_out: float32 [rows, L], required; wq_out: dtype_w [rows, L] or NULL.  Bit for bit the four-launch chain dmxq_scale_channels
 * (multiply, dtype_w) -> dmxq_dynamic_fixed_qdq -> dmxq_scale_channels (divide, float32) -> the subtraction.  A lane owns four
 * consecutive elements (the float32 side moves as 16 bytes per lane); a group is group / 4 adjacent lanes.
 * dmxq_awq_class(dtype_w, L, group): 1 where the kernel takes the geometry -- group a power of two from 16 to 256 that divides L --
 * else 0; a host function, no GPU involved.  DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs the chain, same bits): class 0,
 * fraction != 0, no clamp, precision > 22, a pointer that is not 16-byte aligned.  DMXQ_ERR_BAD_ARG: invalid dtype, negative sizes,
 * qmax <= qmin, null w / s / d_out.  No workspace, no allocation, no host synchronisation. */
int dmxq_channel_sumabs_accumulate(const void* in, int dtype_in, int64_t rows, int64_t C, double* acc, void* workspace, void* stream);
int dmxq_awq_class(int dtype_w, int64_t L, int64_t group);
int dmxq_awq_group_error(const void* w, int dtype_w, const float* s, float* d_out, void* wq_out, int64_t rows, int64_t L, int64_t group,
                         int precision, int fraction, int clamp, int symmetric, int qmin, int qmax, int symmetric_qscheme, void* stream);

/* AWQ weight clipping (AutoAWQ's clip search after the scale) in ONE launch (csrc/awq_clip.hip; DESIGN.md §8 "AWQ clipping", whose text
 * is the contract).  Not in the reference.  w[rows, L] of dtype_w, contiguous; blocks: DEVICE float32 [L / group, group, group], the
 * diagonal blocks of the calibration inputs' second moment, used as given; ratios: DEVICE float32 [n_ratios], 1 <= n_ratios <= 32,
 * ratios[0] == 1, non-increasing in (0, 1] (the values are the caller's contract: the host never reads them).  Per group of `group`
 * consecutive columns of a row, every operation fp32 and none contracted:
 *   a = max |W| (NaN if any element is);  a group whose a is not finite and positive keeps its bits, best = 0, clip = a, NaN losses;
 *   candidate i: c = fp32(dtype_w(a * ratios[i]));  v = W > c ? c : (W < -c ? -c : W);  q = the per-group dynamic integer cast of
 *   dmxq_dynamic_fixed_qdq on v (the same device code; (qmin, qmax, symmetric_qscheme) as there);  d = fp32(q) - W;
 *   t_j = sum_l blocks[k][j][l] * d_l in index order from the first product;  loss_i = the adjacent-pair tree sum of d_j * t_j;
 *   best = the lowest i among the minimal finite losses (0 when none is finite);  y = dtype_w(v of best);  clip = c of best.
 * y_out: dtype_w [rows, L], may be w itself; best_out: NULL or uint8 [rows, L / group]; clip_out: NULL or float32 [rows, L / group];
 * losses_out: NULL or float32 [rows, L / group, n_ratios].
 * dmxq_awq_clip_class(dtype_w, L, group): 1 where the kernel takes the geometry -- group 16, 32, 64 or 128 dividing L -- else 0; a host
 * function, no GPU involved.  DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain, same bits): class 0, fraction != 0, no
 * clamp, precision > 22, a pointer that is not 16-byte aligned.  DMXQ_ERR_BAD_ARG: invalid dtype, negative sizes, qmax <= qmin,
 * n_ratios outside 1 .. 32, null w / blocks / ratios / y_out.  No workspace, no allocation, no host synchronisation, no float
 * atomics: capturable. */
int dmxq_awq_clip_class(int dtype_w, int64_t L, int64_t group);
int dmxq_awq_clip(const void* w, int dtype_w, const float* blocks, const float* ratios, int n_ratios, void* y_out, uint8_t* best_out,
                  float* clip_out, float* losses_out, int64_t rows, int64_t L, int64_t group, int precision, int fraction, int clamp,
                  int symmetric, int qmin, int qmax, int symmetric_qscheme, void* stream);

/* AdaRound (Nagel et al. 2020): the soft cast of learned weight rounding and its backward pass, each ONE streaming launch
 * (csrc/adaround.hip; DESIGN.md §8 "AdaRound").  Not in the reference.  w: the contiguous [n_segments, segment] weight (bf16 / f16 /
 * f32); V: DEVICE float32, one per element; scale: DEVICE float32 [n_segments]; zero_point: DEVICE float32 [n_segments] holding the
 * INTEGER zero points; y: dtype_out, g: dtype_g -- each the weight's dtype or float32; dV: float32.  Per element, every operation one
 * fp32 operation in this order, G = -0.1f, ZG = 1.1f - (-0.1f):
 *   v = w / s (IEEE division);  f = floorf(v);  sg = 1 / (1 + expf(-V));  hr = sg * ZG + G;
 *   h = clamp(hr, 0, 1), or with hard != 0: h = V >= 0 ? 1 : 0 (no transcendental);
 *   q = clamp((f + h) + zq, qmin, qmax);  y = (q - zq) * s, rounded once more to dtype_out.
 * Backward, the gradient of V alone (bm1 = beta - 1 and m2b = -2 * beta formed once in fp32):
 *   in01 = 0 < hr < 1;  cell = qmin <= f + zq <= qmax - 1;  dh = (sg * (1 - sg)) * ZG;  rec = (in01 && cell) ? (g * s) * dh : 0;
 *   t2 = 2 * h - 1;  a = |t2|;  p1 = powf(a, bm1);  r = 1 - p1 * a;  dreg = in01 ? reg_weight * (((m2b * p1) * sign(t2)) * dh) : 0;
 *   dV = rec + dreg (rec alone when reg_weight == 0);  reg_out[0] = sum (double)r over the tensor.
 * The sum is float64 without floating-point atomics: one partial sum per workgroup in `scratch` (dmxq_adaround_scratch_bytes(n) bytes
 * of device memory for n elements, 8-byte aligned, contents free) and a second small launch that folds them in a fixed order; the order
 * depends on the shape alone.  reg_out == NULL: no sum, scratch unused (may be NULL).  NaN / Inf: csrc/adaround.hip's header.
 * dmxq_adaround_class: how a 16-byte vector finds its segment -- SHIFT where segment / vector is a power of two, DIVIDE for any other
 * whole number of vectors, NONE where the entries refuse; dmxq_adaround_scratch_bytes: both host functions, no GPU involved.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain of torch operations): a segment that is not whole 16-byte vectors
 * of the weight, a pointer that is not 16-byte aligned (scratch, reg_out: 8-byte), dtype_out / dtype_g neither the weight's dtype nor
 * float32.  DMXQ_ERR_BAD_ARG: null pointers, negative sizes, an invalid dtype, qmax <= qmin, a scratch smaller than the query says.
 * No allocation, no host synchronisation: capturable. */
typedef enum { DMXQ_ADAROUND_NONE = 0, DMXQ_ADAROUND_SHIFT = 1, DMXQ_ADAROUND_DIVIDE = 2 } dmxq_adaround_geometry;
int dmxq_adaround_class(int dtype, int64_t segment);
int64_t dmxq_adaround_scratch_bytes(int64_t n);
int dmxq_adaround_forward(const void* w, const float* V, void* y, int dtype_w, int dtype_out, int64_t n_segments, int64_t segment, int qmin,
                          int qmax, const float* scale, const float* zero_point, int hard, void* stream);
int dmxq_adaround_backward(const void* w, const float* V, const void* g, float* dV, int dtype_w, int dtype_g, int64_t n_segments,
                           int64_t segment, int qmin, int qmax, const float* scale, const float* zero_point, float beta, float reg_weight,
                           double* reg_out /* double[1], may be NULL */, void* scratch, int64_t scratch_bytes, void* stream);

/* Two-level BLOCK-SCALED float cast (csrc/block_scaled_float.hip; DESIGN.md §8 "Block-scaled float cast"): the group scale of
 * dmxq_dynamic_float_qdq QUANTISED to a low-bit float format, under one float32 scale per tensor -- the numerics of a stored block-scaled
 * format (E2M1 elements in groups of 16 with an E4M3 group scale: "NVFP4"; E4M3 elements with quantised group scales).  Not in the
 * reference.  E = the signed element format (man_bits, exp_bits < 8, exp_bias, flush_subnormal) with largest output fmax; Sf = the scale
 * format (scale_man_bits, scale_exp_bits < 8, scale_exp_bias, scale_flush_subnormal) with largest output sfmax (scales are never
 * negative: no sign field); 0 < scale_max <= sfmax caps the scale code (448 keeps an FP[1|4|3,7] scale inside the OCP E4M3FN codes).
 * tensor_scale: NULL (t = 1) or ONE float on the DEVICE, read by the kernel (never by the host); t = 1 where it is not finite or below
 * 2^-126.  Per group of `group` consecutive elements of the contiguous tensor, in fp32:
 *   a  = max |x| (one NaN anywhere makes it NaN);  c = (a / fmax) / t, two IEEE divisions;
 *   sq = min(float_q_Sf(c), scale_max): the scale format's nearest cast, NaN / Inf saturating to sfmax -- sq is never NaN;
 *   s  = sq * t, one fp32 multiply; usable when finite and >= 2^-126;
 *   usable:  out = float_q_E(x / s) * s: IEEE quotient, the element format's nearest cast (flush flag kept, NaN / Inf saturate as in
 *            dmxq_float_qdq), one fp32 multiply, one rounding to dtype_out;
 *   else:    out = a zero with the sign bit of float_q_E(x), and the reported s is 0 (an all-zero group, or one whose scale code is 0).
 * The output holds no NaN.  scale_out / scale_q_out: NULL or DEVICE arrays of n_groups floats, s and sq of every group.
 * The kernel takes dtype_in == dtype_out (bf16 / f16 / f32), group a power of two from 16 to 256, nearest rounding in both formats and
 * 16-byte aligned bases: dmxq_dynamic_float_qdq's flat group geometry, ONE launch.  dmxq_block_scaled_float_class(dtype, group):
 * DMXQ_DYN_GROUP where it does, DMXQ_DYN_NONE otherwise; a host function, no GPU involved.
 * DMXQ_ERR_UNSUPPORTED, nothing launched (the caller runs its chain of launches, same bits): other dtype pairs, other group sizes,
 * unaligned bases, a rounding other than nearest in either format, man_bits > 22 in either format.  DMXQ_ERR_BAD_ARG: null data
 * pointers, negative sizes, invalid dtype / rounding, exp_bits outside 1 .. 7 or negative man_bits in either format, scale_max outside
 * (0, sfmax].  No workspace, no allocation, no host synchronisation: capturable.
 * dmxq_block_scaled_tensor_scale: the DYNAMIC tensor scale of the contiguous tensor in[n] into the one DEVICE float t_out --
 * t = (max |x| / fmax) / scale_max, two IEEE divisions, one NaN anywhere makes the maximum NaN, t = 1 where it is not finite or below
 * 2^-126 (n = 0: 1) -- in three small launches (the word is zeroed, one integer atomic per workgroup on the magnitude bits, one thread
 * finishes in place): exact in any order, capturable, no workspace.  DMXQ_ERR_UNSUPPORTED, nothing launched (the caller uses
 * dmxq_group_minmax over the whole tensor): n not whole 16-byte vectors, an unaligned base.  DMXQ_ERR_BAD_ARG: invalid dtype, n < 0, null
 * pointers, fmax or scale_max not positive and finite. */
int dmxq_block_scaled_float_class(int dtype, int64_t group);
int dmxq_block_scaled_tensor_scale(const void* in, int dtype_in, int64_t n, float fmax, float scale_max, float* t_out, void* stream);
int dmxq_block_scaled_float_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_groups, int64_t group, int man_bits,
                                int exp_bits, int exp_bias, int flush_subnormal, int rounding, int scale_man_bits, int scale_exp_bits,
                                int scale_exp_bias, int scale_flush_subnormal, int scale_rounding, float scale_max,
                                const float* tensor_scale, float* scale_out, float* scale_q_out, void* stream);

/* Which kernel a row function launches (csrc/row_class.hpp): what dmxq_softmax* / dmxq_layernorm* / dmxq_rmsnorm* will do for one call,
 * answered by the function their dispatch itself decides with.  A host function: no GPU involved, no HIP call, the pointers are not
 * dereferenced -- only their alignment matters (in == out, an in-place call, takes the same class as the out-of-place one).
 *   op            dmxq_row_op;  dtype_wb is read only where weight or bias is not NULL (RMSNorm: bias = NULL);
 *   cast_kind     dmxq_row_cast_kind: NONE = the plain entries (dmxq_softmax, dmxq_layernorm, dmxq_rmsnorm), anything else = the *_cast
 *                 entries (one dtype throughout).  16-bit rows take range-only casts, so every other kind is the same class there; on
 *                 float32 rows MAN16 = the output cast is active and keeps <= 16 mantissa bits (softmax then takes its FAST32 form),
 *                 GENERAL = any other pair of casts;
 *   bfp_block     0, or the block size of the *_cast_bfp entries.
 * Answer (dmxq_row_class):
 *   family        dmxq_row_family: UNSUPPORTED = the entry refuses the call (DMXQ_ERR_UNSUPPORTED: a fused form outside the
 *                 register-resident rows, a block size that is not a power-of-two number of lane-vectors of one slot); WAVE = a row per
 *                 `lpr` = 64 or 32 lanes; BLOCK = a row per 256-thread workgroup (lpr = 256); LDS_ROWS / GLOBAL_ROWS = the fallbacks, a
 *                 workgroup per row staged in LDS / read three times (epl = vpl = lpr = 0);
 *   epl, vpl, lpr elements per lane-vector, lane-vectors per lane (the kernel's template argument: 7 needed = 8), lanes per row;
 *   rag           rows of any length / alignment: unaligned 16-byte vectors with an overlapped last one (softmax);
 *   half_vec      8-byte lane-vectors (16-bit rows that are a multiple of 4 elements on 8-byte bases);
 *   fast32        float32 softmax behind a MAN16 output cast;  bfpout: the fused BFP epilogue;
 *   grid          dmxq_row_grid: PERSISTENT = as many workgroups as are resident, each looping; ONE_PASS = a workgroup per rows_per_iter
 *                 rows; MID_ONE_PASS = the BLOCK kernel's one-pass form for tensors of 26-32 MiB; MODULE_ONE_PASS = the LayerNorm module
 *                 on 16-bit rows of 768; MODULE_ROWS4 = the RMSNorm module on 16-bit rows of 4096 at 26-32 MiB (persistent, 4 rows);
 *                 CAPPED = the fallbacks' min(rows, 4096) workgroups;
 *   rows_per_iter rows one workgroup takes per iteration.
 * Returns DMXQ_OK, or DMXQ_ERR_BAD_ARG (invalid op / dtype / cast_kind, rows or cols < 1, bfp_block < 0, bfp_block without a cast, cls NULL). */
typedef enum { DMXQ_ROW_SOFTMAX = 0, DMXQ_ROW_LAYERNORM = 1, DMXQ_ROW_RMSNORM = 2 } dmxq_row_op;
typedef enum { DMXQ_ROWCAST_NONE = 0, DMXQ_ROWCAST_RANGE = 1, DMXQ_ROWCAST_GENERAL = 2, DMXQ_ROWCAST_MAN16 = 3 } dmxq_row_cast_kind;
typedef enum { DMXQ_ROWK_UNSUPPORTED = 0, DMXQ_ROWK_WAVE = 1, DMXQ_ROWK_BLOCK = 2, DMXQ_ROWK_LDS_ROWS = 3, DMXQ_ROWK_GLOBAL_ROWS = 4 } dmxq_row_family;
typedef enum { DMXQ_ROWGRID_NONE = 0, DMXQ_ROWGRID_PERSISTENT = 1, DMXQ_ROWGRID_ONE_PASS = 2, DMXQ_ROWGRID_MID_ONE_PASS = 3,
               DMXQ_ROWGRID_MODULE_ONE_PASS = 4, DMXQ_ROWGRID_MODULE_ROWS4 = 5, DMXQ_ROWGRID_CAPPED = 6 } dmxq_row_grid;
typedef struct { int family, epl, vpl, lpr, rag, half_vec, fast32, bfpout, grid, rows_per_iter; } dmxq_row_class;
int dmxq_row_class_of(int op, int dtype_in, int dtype_out, int dtype_wb, int64_t rows, int64_t cols, const void* in, const void* out,
                      const void* weight, const void* bias, int cast_kind, int64_t bfp_block, dmxq_row_class* cls);

#ifdef __cplusplus
}
#endif
#endif /* DMXQ_H */
