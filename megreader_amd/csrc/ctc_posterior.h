// The CTC posterior as mr_lexicon_transcribe, mr_ctc_beam_search and mr_ctc_align read it (include/megreader_hip.h): one
// definition of lp[t, c], of the log-space arithmetic on it and of the keys that order its values, so that the three give the
// same bits for the same input; and one set of host checks for their entry points.  (The training losses in ctc.hip and
// ctc2d.hip have their own f64 / library-precision lse: different functions, not these.)
#pragma once
#include "common.h"
#include "../../include/megreader_hip.h"

namespace mr {

typedef unsigned long long u64;

constexpr float CTC_NEG_INF = -__builtin_inff();

// The log of a probability as the header defines it: taken in f64 and rounded once, the f32 nearest to log y whichever library
// computes it -- so a caller who passes such logs gets the same bits.  (logf is within 1 ulp, not the nearest.)  0 gives -inf.
__device__ __forceinline__ float ctc_log_prob(float y) { return (float)log((double)y); }

// lp of one value as it was read: the value itself with log_probs, else its log
__device__ __forceinline__ float ctc_lp(float y, bool log_probs) { return log_probs ? y : ctc_log_prob(y); }

// lp of element i of a strided run (f32 or bf16; `stride` in elements): a class of a column, or a column of a class
template <typename PT>
__device__ __forceinline__ float ctc_lp_at(const PT* p, long long stride, int i, bool log_probs) {
  return ctc_lp(to_f32(p[(long long)i * stride]), log_probs);
}

// log(exp(a) + exp(b) [+ exp(c)]) shifted by the maximum; every term -inf gives -inf (the select drops the NaN of -inf - -inf).
// The hardware exp2 / log2: their error (a few 1e-7 absolute per step) is far below the rounding of alpha at its magnitude.
__device__ __forceinline__ float ctc_lse2(float a, float b) {
  const float m = fmaxf(a, b);
  const float r = m + __logf(__expf(a - m) + __expf(b - m));
  return m == CTC_NEG_INF ? m : r;
}
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  const float r = m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
  return m == CTC_NEG_INF ? m : r;
}

// lane l <- lane l - 1 (DPP wave_shr:1, no LDS); the lane whose `lane` is 0 keeps `first`.  `lane` may be the lane of a group of
// a wave (mr_lexicon_transcribe scores four words side by side: each group's lane 0 takes -inf).
__device__ __forceinline__ float ctc_from_lane_below(float v, float first, int lane) {
  const int got = __builtin_amdgcn_update_dpp(__float_as_int(CTC_NEG_INF), __float_as_int(v), 0x138, 0xf, 0xf, false);
  return lane == 0 ? first : __int_as_float(got);
}

// order-preserving u32 of an f32 and back.  The bits decide: -0 sorts below +0 and comes back as -0.
__device__ __forceinline__ unsigned ctc_ordered(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ctc_unordered(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// greater key = greater value, then lower index; 0 = "no candidate" (-inf never makes a key).  merge_zeros: -0 and +0 are one
// value (+0).  mr_ctc_beam_search passes true: its keys alone order a column's classes and a beam's candidates, and between a -0
// and a +0 (both log 1) the lower index has to win as between any equal values; a total it takes back out of a key is then +0.
// mr_lexicon_transcribe passes false: its best_score comes back out of the key (ctc_unordered) and is, bit for bit, the score as
// computed, the cell all_scores[n, best_index].
__device__ __forceinline__ u64 ctc_key(float v, unsigned index, bool merge_zeros) {
  return v > CTC_NEG_INF ? ((u64)ctc_ordered(merge_zeros && v == 0.f ? 0.f : v) << 32) | (u64)(0xffffffffu - index) : 0ull;
}
__device__ __forceinline__ u64 ctc_wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// ---- host: what the three entry points check alike.  Each returns MR_OK or sets the error text; an entry point calls them in
// the order it reports its conditions in, with its own checks between them. ----

#define MR_CTC_TRY(check)                  \
  do {                                     \
    const int rc__ = (check);              \
    if (rc__ != mr::MR_OK) return rc__;    \
  } while (0)

// t_max: the entry point's bound on T; 0: none (mr_lexicon_transcribe holds no per-column state)
inline int ctc_check_columns(const char* who, int T, int t_max) {
  if (t_max > 0)
    MR_CHECK_ARG(T >= 1 && T <= t_max, "%s: T=%d columns (1..%d)", who, T, t_max);
  else
    MR_CHECK_ARG(T >= 1, "%s: T=%d columns", who, T);
  return MR_OK;
}
inline int ctc_check_classes(const char* who, int C, int blank) {
  MR_CHECK_ARG(C >= 2, "%s: C=%d classes (blank and one symbol are 2)", who, C);
  MR_CHECK_ARG(blank >= 0 && blank < C, "%s: blank=%d is not a class of C=%d", who, blank, C);
  return MR_OK;
}
inline int ctc_check_dtype(const char* who, int dtype) {
  if (dtype == MR_DTYPE_F32 || dtype == MR_DTYPE_BF16) return MR_OK;
  set_error("%s: bad dtype %d (0 = float32, 1 = bfloat16)", who, dtype);
  return MR_ERR_DTYPE;
}
// need: what `sizer` (the entry point's *_ws_bytes) gives for the call's sizes; 0 stands for "above INT_MAX bytes"
inline int ctc_check_workspace(const char* who, const char* sizer, const void* ws, long long ws_bytes, long long need) {
  MR_CHECK_ARG(need > 0, "%s: these sizes need a workspace above 2 GiB (%s gives 0): split the batch", who, sizer);
  MR_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0,
               "%s: workspace %p of %lld bytes; %s asks for %lld, 8-byte aligned", who, ws, ws_bytes, sizer, need);
  return MR_OK;
}

// `...` once with PT = float and once with PT = bf16_t, run for the one `dtype` names (ctc_check_dtype has passed)
#define MR_CTC_DISPATCH(dtype, PT, ...) \
  do {                                  \
    if ((dtype) == MR_DTYPE_F32) {      \
      typedef float PT;                 \
      __VA_ARGS__;                      \
    } else {                            \
      typedef mr::bf16_t PT;            \
      __VA_ARGS__;                      \
    }                                   \
  } while (0)

}  // namespace mr
