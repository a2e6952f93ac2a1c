// Forced CTC alignment: the most probable alignment (Viterbi) of a GIVEN string to a CTC posterior, traced back, with the columns,
// the summed log-probability and the peak column of every symbol.  The rule is written out in include/megreader_hip.h
// (mr_ctc_align); this file is one kernel, one wave per row.
//
// The layout is that of the alpha recursion in lexicon.hip with `max` for `lse`: lane i holds symbol i and two positions of the
// blank-extended string, B_i (the blank before the symbol, position 2i) and Y_i (the symbol, position 2i + 1).  One column:
//   B_i' = lp[t, blank] + max(B_i, Y_{i-1})        Y_i' = lp[t, sym_i] + max(Y_i, B_i, Y_{i-1} if sym_i != sym_{i-1})
// so ONE value crosses lanes per column (a DPP wave shift).  The blank after the last symbol is B_K.  A string of 64 symbols or
// more does not fit 64 lanes: lane l then holds the symbols l, l + 64, .. in NS register slots (2 up to 127 symbols, 5 up to
// MR_CTC_ALIGN_MAX_SYMBOLS), and lane 0 of slot j takes Y from lane 63 of slot j - 1.  Nothing of the recursion lives in LDS.
// A lane loads its symbols' values a few columns ahead of the recursion and takes their logs (the f64 log is most of the work
// of a column); the blank's are loaded one column per lane and broadcast.  Only these K + 1 classes are ever read: one string per
// row touches (K + 1) * T cells, so staging the row's [C, T] table first, as mr_lexicon_transcribe does for its many words, would
// take MORE logs, not fewer.
//
// Back-pointers: 4 bits per (column, symbol) -- 2 for Y (0 stay, 1 from B_i, 2 from Y_{i-1}), 1 for B (0 stay, 1 from Y_{i-1}) --
// packed per lane into 32-bit words of 8 / 4 / 1 columns (NS = 1 / 2 / 5), [word][lane]: in LDS when the row's words fit 16 KiB
// (512 columns of a string below 64 symbols), else in the caller's workspace.  A lane only ever reads back the words it wrote
// itself, so no fence is needed either way, a wave's access is one 256-byte line, and the loads of the back-trace do not depend
// on the path: the next word is in flight while the walk (wave-uniform, T steps in scalar registers, the lane that owns the
// position hands its bits over by a readlane) consumes this one.  (Measured on 256 rows x 129 columns x 25 symbols: LDS in the
// place of the workspace 3 % of the call, the scalar walk and the loads one chunk ahead 3 %, chunk loads without a branch each
// and whole chunks without a test per column 4 %; the f64 logs are 41 % of that call.)  The walk leaves pos[t] on lane t % 64 (stored 64 columns at a time)
// and the first / last column of symbol i on its own lane; the span sums and peaks are then lane-parallel over the symbols.
#include <limits.h>
#include "device.h"
#include "ctc_posterior.h"
#include "../../include/megreader_hip.h"

namespace mr {

enum { CTCA_LDS_WORDS = 4096 };   // back-pointer words (16 KiB) a row may keep in LDS

// register slots of a lane for a string of K symbols (K + 1 pairs of positions), and 32-bit back-pointer words per row
__host__ __device__ inline int ctca_slots(int K) { return K < 64 ? 1 : K < 128 ? 2 : 5; }
__host__ __device__ inline long long ctca_row_words(int T, int K) {
  const int ns = ctca_slots(K), cpw = ns == 1 ? 8 : ns == 2 ? 4 : 1;   // columns per word
  return (long long)((T + cpw - 1) / cpw) * 64;
}

// A row that is unalignable or has no alignment of non-zero probability
__device__ __forceinline__ void ctca_fill_dead(int T, int S, float* score, int* pos, int* begin, int* end, float* sym_lp,
                                               int* peak) {
  const int lane = threadIdx.x;
  for (int t = lane; t < T; t += 64) pos[t] = -1;
  for (int i = lane; i < S; i += 64) {
    begin[i] = -1; end[i] = -1; peak[i] = -1; sym_lp[i] = CTC_NEG_INF;
  }
  if (lane == 0) *score = CTC_NEG_INF;
}

// The row's recursion, back-trace and outputs with NS slots per lane (K < 64 * NS); every pointer is the row's own.  The target
// was checked: K in [0, S], every symbol a class other than blank.  false (and nothing written): the best score is -inf.
template <typename PT, int NS>
__device__ bool ctca_row(const PT* row, long long sc, long long st, int T, bool log_probs, int blank, const int* tgt, int K, int S,
                         unsigned* bp, float* score, int* pos, int* begin, int* end, float* sym_lp, int* peak) {
  enum { CPW = NS == 1 ? 8 : NS == 2 ? 4 : 1, BITS = 32 / CPW, AHEAD = NS == 1 ? 16 : NS == 2 ? 8 : 4 };
  const int lane = threadIdx.x;
  bool live[NS], hop[NS];
  const PT* ps[NS];
  const PT* pb = row + (long long)blank * sc;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int i = lane + 64 * j;
    live[j] = i < K;
    const int c = live[j] ? tgt[i] : blank;                 // (idle slots read the blank's values and drop them)
    hop[j] = live[j] && i >= 1 && c != tgt[i - 1];          // the s - 2 term: from the symbol before, over the blank
    ps[j] = row + (long long)c * sc;
  }
  float B[NS], Y[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) B[j] = Y[j] = CTC_NEG_INF;
  unsigned word = 0u;
  // the values of AHEAD columns: the symbols' per slot, the blank's one column per lane
  float v[NS][AHEAD], lb;
  // (columns past the end read the last column again and are dropped: no branch per load, so the loads of a chunk issue
  // back to back)
  auto load = [&](int t0, float (&dst)[NS][AHEAD], float& dst_b) {
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int u = 0; u < AHEAD; ++u) dst[j][u] = to_f32(ps[j][(long long)min(t0 + u, T - 1) * st]);
    dst_b = to_f32(pb[(long long)min(t0 + lane, T - 1) * st]);
  };
  load(0, v, lb);
  for (int t0 = 0; t0 < T; t0 += AHEAD) {
    const int nt = min((int)AHEAD, T - t0);
    // the next columns are in flight while these take their logs and run: a row is one wave, nothing else hides the latency
    float vn[NS][AHEAD], lbn;
    const bool more = t0 + AHEAD < T;   // (wave-uniform)
    if (more) load(t0 + AHEAD, vn, lbn);
    if (!log_probs) {
#pragma unroll
      for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) v[j][u] = ctc_log_prob(v[j][u]);
      lb = ctc_log_prob(lb);
    }
    // column t0 + u; u is a constant after unrolling, and t0 a multiple of CPW: which columns close a word is known at compile time
    auto column = [&](int u) {
      {
        const float lpb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lb), u));
        if (u == 0 && t0 == 0) {
          if (lane == 0) {
            B[0] = lpb;
            Y[0] = live[0] ? v[0][u] : CTC_NEG_INF;
          }
        } else {
          float Yb[NS];   // Y_{i-1} of the column before, for every slot, before any is overwritten
#pragma unroll
          for (int j = 0; j < NS; ++j) {
            float first = CTC_NEG_INF;
            if (j > 0) first = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Y[j > 0 ? j - 1 : 0]), 63));
            Yb[j] = ctc_from_lane_below(Y[j], first, lane);
          }
          unsigned codes = 0u;
#pragma unroll
          for (int j = 0; j < NS; ++j) {
            // strict comparisons: among equal candidates the smallest step stays
            float mb = B[j];
            unsigned cb = 0u;
            if (Yb[j] > mb) { mb = Yb[j]; cb = 1u; }
            float my = Y[j];
            unsigned cy = 0u;
            if (B[j] > my) { my = B[j]; cy = 1u; }
            if (hop[j] && Yb[j] > my) { my = Yb[j]; cy = 2u; }
            B[j] = lpb + mb;
            Y[j] = live[j] ? v[j][u] + my : CTC_NEG_INF;
            codes |= (cy | (cb << 2)) << (4 * j);
          }
          word |= codes << (BITS * (u & (CPW - 1)));
        }
        if ((u & (CPW - 1)) == CPW - 1) {
          bp[(long long)((t0 + u) / CPW) * 64 + lane] = word;
          word = 0u;
        }
      }
    };
    if (nt == AHEAD) {   // (wave-uniform) whole chunks run without a test per column
#pragma unroll
      for (int u = 0; u < AHEAD; ++u) column(u);
    } else {
#pragma unroll
      for (int u = 0; u < AHEAD; ++u)
        if (u < nt) column(u);
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) v[j][u] = vn[j][u];
      lb = lbn;
    }
  }
  if (T % CPW) bp[(long long)((T - 1) / CPW) * 64 + lane] = word;   // the columns of the last, partial word
  // the end position: the blank after the last symbol (B_K), or the last symbol
  float bsel = B[0], ysel = Y[0];
#pragma unroll
  for (int j = 1; j < NS; ++j) {
    if ((K >> 6) == j) bsel = B[j];
    if (K >= 1 && ((K - 1) >> 6) == j) ysel = Y[j];
  }
  const float dB = __shfl(bsel, K & 63, 64);
  const float dY = K >= 1 ? __shfl(ysel, (K - 1) & 63, 64) : CTC_NEG_INF;
  // (the same on every lane; readfirstlane tells the compiler so, and the walk below stays in scalar registers)
  int s = __builtin_amdgcn_readfirstlane(K == 0 ? 0 : (dB >= dY ? 2 * K : 2 * K - 1));
  const float best = (K == 0 || dB >= dY) ? dB : dY;
  if (!(best > CTC_NEG_INF)) return false;

  // back-trace: one path, walked by the scalar unit; the lanes watch it for what is theirs
  int bg[NS], en[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) bg[j] = en[j] = -1;
  int ch = (T - 1) / CPW;
  unsigned w = bp[(long long)ch * 64 + lane];
  unsigned wn = ch > 0 ? bp[(long long)(ch - 1) * 64 + lane] : 0u;
  int mypos = -1;
  for (int t = T - 1;; --t) {
    const int i = s >> 1;
    if (lane == (t & 63)) mypos = s;
    if ((s & 1) && lane == (i & 63)) {
#pragma unroll
      for (int j = 0; j < NS; ++j)
        if ((i >> 6) == j) {
          if (en[j] < 0) en[j] = t + 1;
          bg[j] = t;
        }
    }
    if ((t & 63) == 0 && t + lane < T) pos[t + lane] = mypos;
    if (t == 0) break;
    if (t / CPW != ch) {
      ch = t / CPW;
      w = wn;
      wn = ch > 0 ? bp[(long long)(ch - 1) * 64 + lane] : 0u;
    }
    const unsigned ww = (unsigned)__builtin_amdgcn_readlane((int)w, i & 63);
    const unsigned nib = (ww >> (BITS * (t & (CPW - 1)) + 4 * (i >> 6))) & 15u;
    const int step = (s & 1) ? (int)(nib & 3u) : (int)((nib >> 2) & 1u);
    s = max(s - step, 0);
  }

  // the symbols' spans, lane-parallel
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int i = lane + 64 * j;
    if (i < K) {
      float acc = CTC_NEG_INF, top = CTC_NEG_INF;
      int pk = -1;
      for (int t = bg[j]; t < en[j]; ++t) {
        const float lp = ctc_lp_at(ps[j], st, t, log_probs);
        if (t == bg[j]) {
          acc = lp; top = lp; pk = t;
        } else {
          acc = acc + lp;
          if (lp > top) { top = lp; pk = t; }
        }
      }
      begin[i] = bg[j]; end[i] = en[j]; sym_lp[i] = acc; peak[i] = pk;
    }
  }
  for (int i = K + lane; i < S; i += 64) {
    begin[i] = -1; end[i] = -1; peak[i] = -1; sym_lp[i] = CTC_NEG_INF;
  }
  if (lane == 0) *score = best;
  return true;
}

template <typename PT>
__global__ __launch_bounds__(64) void ctc_align_kernel(const PT* pred, long long sn, long long sc, long long st, int C, int T,
                                                       int log_probs, int blank, int unknown, const int* targets, int S,
                                                       const int* target_len, float* score, int* pos, int* begin, int* end,
                                                       float* sym_lp, int* peak, unsigned* ws, long long row_words) {
  const int lane = threadIdx.x, n = blockIdx.x;
  const int* tgt = targets + (long long)n * S;
  const int K = target_len[n];
  bool ok = K >= 0 && K <= S;
  if (ok) {
    bool bad = false;
    int twins = 0;
    for (int i0 = 0; i0 < K; i0 += 64) {   // (K is wave-uniform)
      const int i = i0 + lane;
      const int c = i < K ? tgt[i] : -1;
      bad = bad || (i < K && (c == blank || c == unknown || (unsigned)c >= (unsigned)C));
      const bool twin = i >= 1 && i < K && c == tgt[i - 1];   // an adjacent equal pair needs a blank between
      twins += __popcll(__ballot(twin));
    }
    ok = __ballot(bad) == 0ull && K + twins <= T;
  }
  const PT* row = pred + (long long)n * sn;
  __shared__ unsigned bp_lds[CTCA_LDS_WORDS];
  // (by the row's own K: neither the choice nor the result depends on S or on the other rows)
  unsigned* bp = ok && ctca_row_words(T, K) <= CTCA_LDS_WORDS ? bp_lds : ws + (long long)n * row_words;
  float* o_score = score + n;
  int* o_pos = pos + (long long)n * T;
  int* o_begin = begin + (long long)n * S;
  int* o_end = end + (long long)n * S;
  float* o_lp = sym_lp + (long long)n * S;
  int* o_peak = peak + (long long)n * S;
  bool done = false;
  if (ok) {   // (wave-uniform)
    const bool lg = log_probs != 0;
    const int ns = ctca_slots(K);
    if (ns == 1)
      done = ctca_row<PT, 1>(row, sc, st, T, lg, blank, tgt, K, S, bp, o_score, o_pos, o_begin, o_end, o_lp, o_peak);
    else if (ns == 2)
      done = ctca_row<PT, 2>(row, sc, st, T, lg, blank, tgt, K, S, bp, o_score, o_pos, o_begin, o_end, o_lp, o_peak);
    else
      done = ctca_row<PT, 5>(row, sc, st, T, lg, blank, tgt, K, S, bp, o_score, o_pos, o_begin, o_end, o_lp, o_peak);
  }
  if (!done) ctca_fill_dead(T, S, o_score, o_pos, o_begin, o_end, o_lp, o_peak);
}

// 0: arguments the entry point refuses, or more than INT_MAX bytes.  A row's words are sized for a string of S symbols.
static long long ctca_ws_bytes(long long N, int T, int S) {
  if (N < 1 || T < 1 || T > MR_SEQ_MEASURE_MAX || S < 0 || S > MR_CTC_ALIGN_MAX_SYMBOLS) return 0;
  const long long bytes = N * ctca_row_words(T, S) * (long long)sizeof(unsigned);
  return bytes <= INT_MAX ? bytes : 0;
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_ctc_align_ws_bytes(int N, int T, int S) { return (int)ctca_ws_bytes(N, T, S); }

int mr_ctc_align(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T, int log_probs,
                 int blank, int unknown, const int* targets, int S, const int* target_len, float* score, int* pos, int* begin,
                 int* end, float* sym_lp, int* peak, void* ws, long long ws_bytes, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0, "mr_ctc_align: N=%d rows", N);
  MR_CHECK_ARG(S >= 0 && S <= MR_CTC_ALIGN_MAX_SYMBOLS, "mr_ctc_align: S=%d symbols per row (0..MR_CTC_ALIGN_MAX_SYMBOLS=%d)", S,
               MR_CTC_ALIGN_MAX_SYMBOLS);
  MR_CTC_TRY(ctc_check_columns("mr_ctc_align", T, MR_SEQ_MEASURE_MAX));
  MR_CTC_TRY(ctc_check_classes("mr_ctc_align", C, blank));
  MR_CTC_TRY(ctc_check_dtype("mr_ctc_align", dtype));
  if (N == 0) return MR_OK;
  MR_CTC_TRY(ctc_check_workspace("mr_ctc_align", "mr_ctc_align_ws_bytes", ws, ws_bytes, ctca_ws_bytes(N, T, S)));
  MR_CHECK_ARG(pred && target_len && score && pos && (S == 0 || (targets && begin && end && sym_lp && peak)),
               "mr_ctc_align: null pointer");
  const long long row_words = ctca_row_words(T, S);
  MR_CTC_DISPATCH(dtype, PT,
                  hipLaunchKernelGGL(ctc_align_kernel<PT>, dim3((unsigned)N), dim3(64), 0, stream, (const PT*)pred, sn, sc, st, C,
                                     T, log_probs, blank, unknown, targets, S, target_len, score, pos, begin, end, sym_lp, peak,
                                     (unsigned*)ws, row_words));
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
