// Lexicon-constrained reading: for every predicted id sequence the nearest word (Levenshtein) of a lexicon.
//   mr_lexicon_nearest   the rule of the lexicon benchmarks (IIIT5K / SVT / IC03 / IC13 with 50, 1 k and "full" lexicons): replace
//                        the prediction by the lexicon word with the smallest edit distance; also the membership test behind
//                        structure/measurers/sequence_recognition_measurer.py:59-64 (`in_lexicon`: distance == 0).
// Bit-parallel edit distance (Myers 1999 in Hyyro's global-distance form): the prediction (m <= 64 symbols) is the pattern, its
// match masks Peq[c] (one u64 per class) are built once per workgroup in LDS, and ONE THREAD PER CANDIDATE WORD runs the
// recurrence over the word's symbols: a whole DP column per symbol in ~15 integer operations on one 64-bit word held in registers.
// The loop reads one LDS word (Peq) and one global word (the symbol) per step; no MFMA, no LDS writes.
//
// Launch sequence of one call (all on the caller's stream): keys[n] = ~0  ->  workgroups (row n, slice k of its candidates): wave
// minimum of the packed key (distance << 32 | word index), one 64-bit atomic min per wave into keys[n]  ->  unpack into the three
// i32 outputs.  The minimum of the packed key is the smallest distance and, among those, the lowest index, whatever the order of
// the atomics: the result is deterministic.
#include <limits.h>
#include <mutex>
#include "device.h"
#include "../../include/megreader_hip.h"

namespace mr {

typedef unsigned long long u64;

enum {
  LEX_BLOCK = 256,        // threads per workgroup: 4 waves share one Peq table
  LEX_DENSE_MAX = 8192,   // classes up to which Peq is a dense table indexed by the class id (64 KiB of LDS; ChineseCharset: 5 360 =
                          // 42 KiB); wider alphabets use the compact table of the <= 64 distinct symbols of the prediction
};

__global__ __launch_bounds__(256) void lexicon_init_kernel(u64* keys, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) keys[i] = ~0ull;
}

__global__ __launch_bounds__(256) void lexicon_unpack_kernel(const u64* keys, int N, int* best_index, int* best_dist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const u64 k = keys[i];
  best_index[i] = k == ~0ull ? -1 : (int)(unsigned)(k & 0xffffffffull);
  best_dist[i] = k == ~0ull ? -1 : (int)(unsigned)(k >> 32);
}

// One column of the DP table: Pv / Mv are the vertical +1 / -1 differences, `top` selects the last row of the pattern.  The carry
// out of the add and the bits shifted out of the word vanish (pattern of 64 symbols: top is bit 63).  `| 1` on Ph makes row 0 of the
// table D[0][j] = j: the global distance, not the best substring match.
__device__ __forceinline__ void lex_step(u64 Eq, u64& Pv, u64& Mv, int& score, u64 top) {
  const u64 Xv = Eq | Mv;
  const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  u64 Ph = Mv | ~(Xh | Pv);
  u64 Mh = Pv & Xh;
  score += (Ph & top) != 0;
  score -= (Mh & top) != 0;
  Ph = (Ph << 1) | 1ull;
  Mh <<= 1;
  Pv = Mh | ~(Xv | Ph);
  Mv = Ph & Xv;
}

// Workgroup b = n * chunks + k: row n against the words lo + k*256 + tid, + chunks*256, ... of its candidate range [lo, hi).
// Dynamic LDS: u64 tab[DENSE ? C : 64], int pat[S], int csym[64].
template <bool DENSE>
__global__ __launch_bounds__(256) void lexicon_nearest_kernel(const int* preds, int S, int N, int blank, int unknown,
                                                              const int* fold, const int* lex_sym, const int* lex_off, int L,
                                                              const int* span, int C, int chunks, u64* keys, int* pred_len) {
  extern __shared__ __attribute__((aligned(16))) u64 lex_lds[];
  __shared__ int s_m, s_nd;
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  int lo = 0, hi = L;
  if (span) {
    lo = min(max(span[2 * n], 0), L);
    hi = min(max(span[2 * n + 1], lo), L);
  }
  // (workgroup-uniform) slices past the end of a short candidate range have nothing to do; slice 0 stays: it writes pred_len
  if (chunk != 0 && (long long)lo + (long long)chunk * LEX_BLOCK >= hi) return;
  const int T = DENSE ? C : 64;
  u64* tab = lex_lds;
  int* pat = (int*)(tab + T);
  int* csym = pat + S;
  if (DENSE)
    for (int i = tid; i < C; i += LEX_BLOCK) tab[i] = 0ull;
  // compact the row as mr_seq_measure does: drop blank / unknown, then fold (an id outside [0, C) stays as it is: it matches nothing)
  if (tid < 64) {
    const int* src = preds + (long long)n * S;
    int cnt = 0;
    for (int p0 = 0; p0 < S; p0 += 64) {
      const int p = p0 + lane;
      int v = p < S ? src[p] : blank;
      const bool keep = p < S && v != blank && v != unknown;
      if (keep && fold && (unsigned)v < (unsigned)C) v = fold[v];
      const u64 km = __ballot(keep);
      const int pos = cnt + __popcll(km & ((1ull << lane) - 1ull));
      if (keep) pat[pos] = v;   // pos < S
      cnt += __popcll(km);
    }
    if (lane == 0) {
      s_m = cnt;
      s_nd = 0;
      if (chunk == 0) pred_len[n] = cnt;
    }
  }
  __syncthreads();
  const int m = s_m;
  if (tid < 64 && m >= 1 && m <= 64) {
    // Peq: lane i holds pattern symbol i; mask = the positions that hold the same symbol; the first lane of each distinct symbol
    // writes the entry (no atomics)
    const int s = lane < m ? pat[lane] : -1;
    u64 mask = 0ull;
    for (int j = 0; j < m; ++j) mask |= (u64)(__shfl(s, j, 64) == s) << j;
    const bool leader = lane < m && (unsigned)s < (unsigned)C && (mask & ((1ull << lane) - 1ull)) == 0ull;
    if (DENSE) {
      if (leader) tab[s] = mask;
    } else {
      const u64 lm = __ballot(leader);
      const int rank = __popcll(lm & ((1ull << lane) - 1ull));
      if (leader) {
        csym[rank] = s;
        tab[rank] = mask;
      }
      if (lane == 0) s_nd = __popcll(lm);
    }
  }
  __syncthreads();
  const int nd = s_nd;

  u64 best = ~0ull;
  int bestd = INT_MAX;
  const long long stride = (long long)chunks * LEX_BLOCK;
  for (long long w = (long long)lo + (long long)chunk * LEX_BLOCK + tid; w < hi; w += stride) {
    const int o0 = lex_off[w];
    const int len = min(max(lex_off[w + 1] - o0, 0), MR_LEXICON_MAX_WORD);   // (the Python layer guarantees <= 64; never trusted)
    // the distance is at least the difference of the lengths: such a word cannot beat this lane's best, and an equal distance
    // loses to the lower index the lane already holds (it visits its words in rising order)
    if (abs(len - m) >= bestd) continue;
    const int* sym = lex_sym + o0;
    int d;
    if (m == 0 || len == 0) {
      d = max(m, len);
    } else if (m <= 64) {
      u64 Pv = ~0ull, Mv = 0ull;
      const u64 top = 1ull << (m - 1);
      d = m;
      // lanes hold words of different lengths: the wave runs to its longest, short lanes masked off.  One load and one lookup per
      // step: loading four symbols ahead of four steps measured 9 % SLOWER (the loop waits on instruction issue, not on memory)
      for (int i = 0; i < len; ++i) {
        const int c = sym[i];
        u64 Eq = 0ull;
        if ((unsigned)c < (unsigned)C) {
          if (DENSE) {
            Eq = tab[c];
          } else {
            for (int k = 0; k < nd; ++k)
              if (csym[k] == c) Eq = tab[k];
          }
        }
        lex_step(Eq, Pv, Mv, d, top);
      }
    } else {
      // the prediction is longer than a machine word: the word (<= 64 symbols) is the pattern, the prediction the text, Eq made on
      // the fly.  Slow and exact.  (A prediction symbol is never `unknown`, so an `unknown` in the word matches nothing here too.)
      u64 Pv = ~0ull, Mv = 0ull;
      const u64 top = 1ull << (len - 1);
      d = len;
      for (int t = 0; t < m; ++t) {
        const int p = pat[t];
        u64 Eq = 0ull;
        if ((unsigned)p < (unsigned)C)
          for (int j = 0; j < len; ++j) Eq |= (u64)(sym[j] == p) << j;
        lex_step(Eq, Pv, Mv, d, top);
      }
    }
    if (d < bestd) {
      bestd = d;
      best = ((u64)(unsigned)d << 32) | (u64)(unsigned)w;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(best, o, 64);
    best = other < best ? other : best;
  }
  if (lane == 0 && best != ~0ull) atomicMin(keys + n, best);
}

// The packed keys of one call: 8 bytes per row in a buffer the library owns per device.  It grows (never shrinks, and a buffer that
// was handed out is never freed: a captured graph keeps its address) on a call outside stream capture; inside a capture a call
// that needs more rows than any call before it on this device is refused.
static u64* lexicon_keys(int N, hipStream_t stream) {
  static std::mutex mu;
  static u64* buf[MR_MAX_DEVICES] = {nullptr};
  static long long cap[MR_MAX_DEVICES] = {0};
  const int dev = current_device();
  if (dev < 0) {
    set_error("mr_lexicon_nearest: no current device with an index below %d", MR_MAX_DEVICES);
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(mu);
  if (cap[dev] >= N) return buf[dev];
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    set_error("mr_lexicon_nearest: N=%d rows need a larger key buffer than the %lld rows allocated so far, and the stream is "
              "capturing: call once with at least this N before the capture", N, cap[dev]);
    return nullptr;
  }
  long long want = cap[dev] > 0 ? 2 * cap[dev] : 8192;
  while (want < N) want *= 2;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)want * sizeof(u64)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("mr_lexicon_nearest: hipMalloc of %lld key rows failed", want);
    return nullptr;
  }
  buf[dev] = (u64*)p;
  cap[dev] = want;
  return buf[dev];
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_lexicon_nearest(const int* preds, int S, int N, int blank, int unknown, const int* fold, const int* lex_sym,
                       const int* lex_off, int L, const int* span, int C, int* best_index, int* best_dist, int* pred_len,
                       hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && S >= 0 && L >= 0, "mr_lexicon_nearest: bad shape N=%d S=%d L=%d", N, S, L);
  MR_CHECK_ARG(S <= MR_SEQ_MEASURE_MAX, "mr_lexicon_nearest: S=%d exceeds MR_SEQ_MEASURE_MAX=%d ids per row", S,
               MR_SEQ_MEASURE_MAX);
  MR_CHECK_ARG(C >= 2, "mr_lexicon_nearest: C=%d classes (blank and unknown alone are 2)", C);
  if (N == 0) return MR_OK;
  MR_CHECK_ARG(best_index && best_dist && pred_len && (S == 0 || preds) && (L == 0 || (lex_sym && lex_off)),
               "mr_lexicon_nearest: null pointer");
  // a row's candidates are spread over enough workgroups to fill the chip when N is small (4 workgroups of 256 per CU), never
  // more than one per 256 words
  const int fill = cdiv(4 * num_cus(), N);
  const int chunks = max(1, min(fill, cdiv(L, LEX_BLOCK)));
  MR_CHECK_ARG((long long)N * chunks <= INT_MAX, "mr_lexicon_nearest: N=%d rows x %d slices exceed the grid", N, chunks);
  const bool dense = C <= LEX_DENSE_MAX;
  const size_t lds = (size_t)(dense ? C : 64) * sizeof(u64) + (size_t)S * sizeof(int) + 64 * sizeof(int);
  const size_t lds_max = (size_t)LEX_DENSE_MAX * sizeof(u64) + (size_t)MR_SEQ_MEASURE_MAX * sizeof(int) + 64 * sizeof(int);
  const int rc = dense ? ensure_dynamic_lds(lexicon_nearest_kernel<true>, lds_max)
                       : ensure_dynamic_lds(lexicon_nearest_kernel<false>, lds_max);
  if (rc != MR_OK) return rc;
  u64* keys = lexicon_keys(N, stream);
  if (!keys) return MR_ERR_LAUNCH;
  hipLaunchKernelGGL(lexicon_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, keys, N);
  if (dense)
    hipLaunchKernelGGL(lexicon_nearest_kernel<true>, dim3(N * chunks), dim3(LEX_BLOCK), lds, stream, preds, S, N, blank,
                       unknown, fold, lex_sym, lex_off, L, span, C, chunks, keys, pred_len);
  else
    hipLaunchKernelGGL(lexicon_nearest_kernel<false>, dim3(N * chunks), dim3(LEX_BLOCK), lds, stream, preds, S, N, blank,
                       unknown, fold, lex_sym, lex_off, L, span, C, chunks, keys, pred_len);
  hipLaunchKernelGGL(lexicon_unpack_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, keys, N, best_index, best_dist);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
