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
//
//   mr_lexicon_transcribe   lexicon-based transcription as the CRNN paper defines it (Shi et al., section 2.3.2): among the words
//                           within edit distance delta of the greedy string, the one with the greatest CTC probability
//                           p(word | y), the sum over all alignments.  The rule is written out in include/megreader_hip.h.
// The candidate pass is the distance loop above (one thread per word); a wave ballots its lanes with d <= delta and then scores
// those words, all 64 lanes on one word, or 16 lanes on each of four words of at most 15 symbols (the lexicons of the benchmarks
// hold few longer ones, and a wave that scores one short word leaves most of its lanes idle): lane i holds symbol i of the word
// and two positions of the blank-extended word, B_i (the blank before the symbol) and Y_i (the symbol).  One step of the alpha recursion, all in f32 logs:
//   B_i' = lp[t, blank] + lse(B_i, Y_{i-1})        Y_i' = lp[t, sym_i] + lse(Y_i, B_i, Y_{i-1} if sym_i != sym_{i-1})
// so ONE value crosses lanes per column (a DPP wave shift, no LDS).  The blank after the last symbol is B_K on lane K; a word of 64
// symbols has no lane 64 and keeps it in a third register E on lane 63 (a wave-uniform branch).  A lane loads its symbol's
// log-probabilities 16 columns ahead of the recursion, the blank's are loaded one per lane and broadcast.  Where the row's whole
// [C, T] table fits 32 KiB (the 38 x 32 of the English CRNN does; the 5 360 classes of the Chinese one do not) the workgroup takes
// its logs once into LDS and the recursions read that; otherwise they read global memory (four 16-byte loads per 16 columns where
// the layout allows: [N, C, 1, T] f32) and take the logs of what they read.  The per-row maximum of (ordered score bits << 32 | ~index) goes through the same key
// buffer with a 64-bit atomic max: the greatest score and, among bit-equal scores, the lowest index, whatever the order.
#include <limits.h>
#include <mutex>
#include "device.h"
#include "ctc_posterior.h"
#include "../../include/megreader_hip.h"

namespace mr {

enum {
  LEX_BLOCK = 256,        // threads per workgroup: 4 waves share one Peq table
  LEX_STAGE_MAX = 8192,   // f32 entries (32 KiB of LDS) up to which mr_lexicon_transcribe stages a row's log-probabilities
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

// The distance of one word (len <= 64 symbols at sym) to the compacted row: m symbols in pat, their match masks in tab / csym / nd
// as lex_prepare leaves them.  One thread per word.
template <bool DENSE>
__device__ __forceinline__ int lex_word_distance(const int* sym, int len, int m, const u64* tab, const int* pat, const int* csym,
                                                 int nd, int C) {
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
  return d;
}

// What every workgroup of the two search kernels does first.  Dynamic LDS: u64 tab[DENSE ? C : 64], int pat[S], int csym[64].
// Compacts row n as mr_seq_measure does -- drop blank / unknown, then fold (an id outside [0, C) stays as it is: it matches
// nothing) -- into pat, builds the match masks of its m symbols when 1 <= m <= 64, and returns m; nd: the distinct symbols of the
// compact table.  Ends behind a barrier.
template <bool DENSE>
__device__ __forceinline__ int lex_prepare(const int* src, int S, int blank, int unknown, const int* fold, int C, u64* tab,
                                           int* pat, int* csym, int& nd) {
  __shared__ int s_m, s_nd;
  const int tid = threadIdx.x, lane = tid & 63;
  if (DENSE)
    for (int i = tid; i < C; i += LEX_BLOCK) tab[i] = 0ull;
  if (tid < 64) {
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
  nd = s_nd;
  return m;
}

// Workgroup b = n * chunks + k: row n against the words lo + k*256 + tid, + chunks*256, ... of its candidate range [lo, hi).
template <bool DENSE>
__global__ __launch_bounds__(256) void lexicon_nearest_kernel(const int* preds, int S, int N, int blank, int unknown,
                                                              const int* fold, const int* lex_sym, const int* lex_off, int L,
                                                              const int* span, int C, int chunks, u64* keys, int* pred_len) {
  extern __shared__ __attribute__((aligned(16))) u64 lex_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  int lo = 0, hi = L;
  if (span) {
    lo = min(max(span[2 * n], 0), L);
    hi = min(max(span[2 * n + 1], lo), L);
  }
  // (workgroup-uniform) slices past the end of a short candidate range have nothing to do; slice 0 stays: it writes pred_len
  if (chunk != 0 && (long long)lo + (long long)chunk * LEX_BLOCK >= hi) return;
  u64* tab = lex_lds;
  int* pat = (int*)(tab + (DENSE ? C : 64));
  int* csym = pat + S;
  int nd;
  const int m = lex_prepare<DENSE>(preds + (long long)n * S, S, blank, unknown, fold, C, tab, pat, csym, nd);
  if (chunk == 0 && tid == 0) pred_len[n] = m;

  u64 best = ~0ull;
  int bestd = INT_MAX;
  const long long stride = (long long)chunks * LEX_BLOCK;
  for (long long w = (long long)lo + (long long)chunk * LEX_BLOCK + tid; w < hi; w += stride) {
    const int o0 = lex_off[w];
    const int len = min(max(lex_off[w + 1] - o0, 0), MR_LEXICON_MAX_WORD);   // (the Python layer guarantees <= 64; never trusted)
    // the distance is at least the difference of the lengths: such a word cannot beat this lane's best, and an equal distance
    // loses to the lower index the lane already holds (it visits its words in rising order)
    if (abs(len - m) >= bestd) continue;
    const int d = lex_word_distance<DENSE>(lex_sym + o0, len, m, tab, pat, csym, nd, C);
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

// ---- mr_lexicon_transcribe ----

// score(n, l) by W = 64 or 16 lanes: row = pred + n*sn, the word's K symbols at sym -- per lane, the same for the W lanes of a
// group; K < 0: the group has no word.  With W = 16 the wave scores four words of at most 15 symbols side by side (positions
// 0..2K on lanes 0..K of the group); the lanes do the same arithmetic either way, so a score does not depend on W.  A pure
// function of the row's values and the word's symbols: nothing here depends on the word's index or on the grid.  Every lane of
// a group returns its score.  LEX_AHEAD columns are loaded (and their logs taken) ahead of the recursion; `vec`: 16-byte loads
// are possible (f32, st == 1, every class row 16-byte aligned).  lpt: the row's log-probabilities staged in LDS by the workgroup
// ([C][T | 1] f32, see lexicon_transcribe_kernel), or null: read them from `row`.  Either way the same f32 values enter the same
// arithmetic.
enum { LEX_AHEAD = 16 };
template <typename PT, int W>
__device__ float lex_ctc_score(const PT* row, long long sc, long long st, int T, bool log_probs, bool vec, const float* lpt,
                               int blank, int unknown, int C, const int* sym, int K) {
  const int lane = threadIdx.x & 63, gl = lane & (W - 1), g0 = lane & ~(W - 1);
  const int c = gl < K ? sym[gl] : -1;
  const int below = __shfl_up(c, 1, 64);
  const bool twin = gl >= 1 && gl < K && c == below;           // an adjacent equal pair needs a blank between
  const bool bad = gl < K && (c == unknown || (unsigned)c >= (unsigned)C);
  const u64 group = W == 64 ? ~0ull : ((1ull << (W & 63)) - 1ull) << g0;
  const bool dead = K < 0 || (__ballot(bad) & group) != 0ull || K + __popcll(__ballot(twin) & group) > T;
  if (__ballot(!dead) == 0ull) return CTC_NEG_INF;
  const bool live = gl < K && !dead;
  const bool hop = live && gl >= 1 && c != below;              // the s - 2 term: from the symbol before, over the blank
  const PT* ps = row + (long long)(live ? c : blank) * sc;     // (idle lanes read the blank's values and drop them)
  const PT* pb = row + (long long)blank * sc;
  const float* ls = lpt ? lpt + (live ? c : blank) * (T | 1) : nullptr;
  const float* lb_row = lpt ? lpt + blank * (T | 1) : nullptr;
  // the state before column 0: all mass "before the first blank"
  float B = gl == 0 ? 0.f : CTC_NEG_INF, Y = CTC_NEG_INF, E = CTC_NEG_INF;
  for (int t0 = 0; t0 < T; t0 += LEX_AHEAD) {
    const int nt = min((int)LEX_AHEAD, T - t0);
    float v[LEX_AHEAD], lb;
    bool wide = false;
    if constexpr (sizeof(PT) == 4) wide = vec && nt == LEX_AHEAD;
    if (lpt) {
#pragma unroll
      for (int j = 0; j < LEX_AHEAD; ++j) v[j] = j < nt ? ls[t0 + j] : 0.f;
      lb = lane < nt ? lb_row[t0 + lane] : 0.f;
    } else if (wide) {
      if constexpr (sizeof(PT) == 4) {
#pragma unroll
        for (int j = 0; j < LEX_AHEAD; j += 4) {
          const f32x4 q = *(const f32x4*)((const float*)ps + t0 + j);
          v[j] = q[0]; v[j + 1] = q[1]; v[j + 2] = q[2]; v[j + 3] = q[3];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < LEX_AHEAD; ++j) v[j] = j < nt ? to_f32(ps[(long long)(t0 + j) * st]) : 1.f;
    }
    if (!lpt) lb = lane < nt ? to_f32(pb[(long long)(t0 + lane) * st]) : 1.f;
    if (!lpt && !log_probs) {
#pragma unroll
      for (int j = 0; j < LEX_AHEAD; ++j) v[j] = ctc_log_prob(v[j]);
      lb = ctc_log_prob(lb);
    }
#pragma unroll
    for (int j = 0; j < LEX_AHEAD; ++j) {
      if (j < nt) {   // (wave-uniform)
        const float lpb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lb), j));
        const float lps = live ? v[j] : CTC_NEG_INF;
        const float Yb = ctc_from_lane_below(Y, CTC_NEG_INF, gl);   // the first lane of a word's group takes -inf
        if constexpr (W == 64) {
          if (K == MR_LEXICON_MAX_WORD) E = lpb + ctc_lse2(E, Y);   // (K is wave-uniform here)
        }
        const float nB = lpb + ctc_lse2(B, Yb);
        Y = lps + ctc_lse3(Y, B, hop ? Yb : CTC_NEG_INF);
        B = nB;
      }
    }
  }
  // the last symbol and the blank after it
  const int Kc = max(K, 0);
  const float first = __shfl(B, g0, 64);
  const float last = __shfl(Y, g0 + max(Kc - 1, 0), 64);
  float tail;
  if constexpr (W == 64) {
    const float after = __shfl(E, 63, 64), on_lane_k = __shfl(B, Kc & 63, 64);
    tail = K == MR_LEXICON_MAX_WORD ? after : on_lane_k;
  } else {
    tail = __shfl(B, g0 + min(Kc, W - 1), 64);
  }
  const float score = Kc == 0 ? first : ctc_lse2(tail, last);
  return dead ? CTC_NEG_INF : score;
}

// One scored candidate: its cell of the table, and the lane's best key (the score's bits as they are: ctc_posterior.h)
__device__ __forceinline__ void lex_post(int w, float score, float* table, u64& best) {
  if (table) table[w] = score;
  best = max(best, ctc_key(score, (unsigned)w, false));
}

// Up to four words of one row by one wave: the 16 lanes of group q hold word w at lex_sym + o, K symbols (K < 0: none).  Four at
// once when all have at most 15 symbols, else one after another on all 64 lanes.
template <typename PT>
__device__ __forceinline__ void lex_score_four(const PT* row, long long sc, long long st, int T, bool log_probs, bool vec,
                                               const float* lpt, int blank, int unknown, int C, const int* lex_sym, int o, int K,
                                               int w, float* table, u64& best) {
  const int lane = threadIdx.x & 63;
  if (__ballot(K > 15) == 0ull) {
    const float score = lex_ctc_score<PT, 16>(row, sc, st, T, log_probs, vec, lpt, blank, unknown, C, lex_sym + o, K);
    if ((lane & 15) == 0 && K >= 0) lex_post(w, score, table, best);
  } else {
    for (int q = 0; q < 4; ++q) {
      const int Kq = __builtin_amdgcn_readlane(K, 16 * q);
      if (Kq < 0) continue;   // (wave-uniform)
      const int oq = __builtin_amdgcn_readlane(o, 16 * q), wq = __builtin_amdgcn_readlane(w, 16 * q);
      const float score = lex_ctc_score<PT, 64>(row, sc, st, T, log_probs, vec, lpt, blank, unknown, C, lex_sym + oq, Kq);
      if (lane == 0) lex_post(wq, score, table, best);
    }
  }
}

// keys[n] = 0 ("no finite score"); n_cand[n] = the whole span without a distance bound, else 0 for the kernel's atomic adds
__global__ __launch_bounds__(256) void lexicon_transcribe_init_kernel(u64* keys, int N, const int* span, int L, int max_distance,
                                                                      int* n_cand) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  keys[i] = 0ull;
  int lo = 0, hi = L;
  if (span) {
    lo = min(max(span[2 * i], 0), L);
    hi = min(max(span[2 * i + 1], lo), L);
  }
  n_cand[i] = max_distance < 0 ? hi - lo : 0;
}

__global__ __launch_bounds__(256) void lexicon_fill_kernel(float* p, long long count, float value) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) p[i] = value;
}

// Workgroup b = n * chunks + k, as lexicon_nearest_kernel.  With a distance bound a thread takes the distance of one word, the wave
// ballots the lanes within the bound and scores those words four at a time; without one the waves of the row's workgroups take
// the words of the span four by four (16 per workgroup and trip).  `stage`: C * (T | 1) <= LEX_STAGE_MAX -- the workgroup first takes the logs of
// its row once, into an LDS table [C][T | 1] f32 behind the others (the odd pitch spreads the classes over the banks), and the
// recursions read that instead of global memory: one log per (class, column) and not one per (word, symbol, column).  A wide
// alphabet does not fit and is not staged: a word touches at most 64 of its classes.
template <bool DENSE, typename PT>
__global__ __launch_bounds__(256) void lexicon_transcribe_kernel(const PT* pred, long long sn, long long sc, long long st, int T,
                                                                 int log_probs, int vec, int stage, const int* preds, int S, int N, int blank,
                                                                 int unknown, const int* fold, const int* lex_sym,
                                                                 const int* lex_off, int L, const int* span, int C,
                                                                 int max_distance, int chunks, u64* keys, int* pred_len,
                                                                 int* n_cand, float* all_scores) {
  extern __shared__ __attribute__((aligned(16))) u64 lex_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  int lo = 0, hi = L;
  if (span) {
    lo = min(max(span[2 * n], 0), L);
    hi = min(max(span[2 * n + 1], lo), L);
  }
  const long long first = max_distance < 0 ? (long long)chunk * 16 : (long long)chunk * LEX_BLOCK;
  if (chunk != 0 && lo + first >= hi) return;   // (workgroup-uniform) slice 0 stays: it writes pred_len
  u64* tab = lex_lds;
  int* pat = (int*)(tab + (DENSE ? C : 64));
  int* csym = pat + S;
  const PT* row = pred + (long long)n * sn;
  float* lpt = stage ? (float*)(csym + 64) : nullptr;
  if (stage) {   // (the barriers of lex_prepare stand between these writes and the reads)
    const int pitch = T | 1;
    for (int i = tid; i < C * T; i += LEX_BLOCK) {
      const int c = i / T, t = i - c * T;
      lpt[c * pitch + t] = ctc_lp(to_f32(row[(long long)c * sc + (long long)t * st]), log_probs != 0);
    }
  }
  int nd;
  const int m = lex_prepare<DENSE>(preds + (long long)n * S, S, blank, unknown, fold, C, tab, pat, csym, nd);
  if (chunk == 0 && tid == 0) pred_len[n] = m;

  float* table = all_scores ? all_scores + (long long)n * L : nullptr;
  const int g = lane >> 4;
  u64 best = 0ull;
  if (max_distance < 0) {
    for (long long w0 = lo + first + 4 * wave; w0 < hi; w0 += (long long)chunks * 16) {
      const long long w = w0 + g;
      int o = 0, K = -1;
      if (w < hi) {
        o = lex_off[w];
        K = min(max(lex_off[w + 1] - o, 0), MR_LEXICON_MAX_WORD);
      }
      lex_score_four<PT>(row, sc, st, T, log_probs != 0, vec != 0, lpt, blank, unknown, C, lex_sym, o, K, (int)w, table, best);
    }
  } else {
    int count = 0;
    // (wave-uniform bounds: the wave's 64 words start at w0)
    for (long long w0 = lo + first + 64 * wave; w0 < hi; w0 += (long long)chunks * LEX_BLOCK) {
      const long long w = w0 + lane;
      int o0 = 0, len = 0;
      bool cand = w < hi;
      if (cand) {
        o0 = lex_off[w];
        len = min(max(lex_off[w + 1] - o0, 0), MR_LEXICON_MAX_WORD);
        cand = abs(len - m) <= max_distance &&
               lex_word_distance<DENSE>(lex_sym + o0, len, m, tab, pat, csym, nd, C) <= max_distance;
      }
      u64 todo = __ballot(cand);
      count += __popcll(todo);
      while (todo) {
        // group q takes the q-th candidate left
        int j = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jq = todo ? __ffsll((long long)todo) - 1 : -1;
          todo &= todo - 1ull;   // (0 stays 0)
          if (g == q) j = jq;
        }
        const int o = __shfl(o0, max(j, 0), 64);
        const int Kj = __shfl(len, max(j, 0), 64);
        const int K = j < 0 ? -1 : Kj;
        lex_score_four<PT>(row, sc, st, T, log_probs != 0, vec != 0, lpt, blank, unknown, C, lex_sym, o, K, (int)w0 + j, table,
                           best);
      }
    }
    if (lane == 0 && count) atomicAdd(n_cand + n, count);
  }
  const u64 top = ctc_wave_max(best);
  if (lane == 0 && top != 0ull) atomicMax(keys + n, top);
}

// One thread per row: the winner out of the key, and its edit distance to the row.  The word (<= 64 symbols) is the pattern, the
// row's ids are compacted and folded on the fly: exact for any row length, and one word per row is little work.
__global__ __launch_bounds__(256) void lexicon_transcribe_unpack_kernel(const u64* keys, int N, const int* preds, int S, int blank,
                                                                        int unknown, const int* fold, const int* lex_sym,
                                                                        const int* lex_off, int C, int* best_index,
                                                                        float* best_score, int* best_dist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const u64 k = keys[i];
  if (k == 0ull) {
    best_index[i] = -1;
    best_score[i] = CTC_NEG_INF;
    best_dist[i] = -1;
    return;
  }
  const int w = (int)(0xffffffffu - (unsigned)(k & 0xffffffffull));
  best_index[i] = w;
  best_score[i] = ctc_unordered((unsigned)(k >> 32));
  const int o0 = lex_off[w];
  const int len = min(max(lex_off[w + 1] - o0, 0), MR_LEXICON_MAX_WORD);
  const int* sym = lex_sym + o0;
  const int* src = preds + (long long)i * S;
  u64 Pv = ~0ull, Mv = 0ull;
  const u64 top = len ? 1ull << (len - 1) : 0ull;
  int d = len, m = 0;
  for (int t = 0; t < S; ++t) {
    int p = src[t];
    if (p == blank || p == unknown) continue;
    if (fold && (unsigned)p < (unsigned)C) p = fold[p];
    ++m;
    if (len == 0) continue;
    u64 Eq = 0ull;
    if ((unsigned)p < (unsigned)C)
      for (int j = 0; j < len; ++j) Eq |= (u64)(sym[j] == p) << j;
    lex_step(Eq, Pv, Mv, d, top);
  }
  best_dist[i] = len ? d : m;
}

// The packed keys of one call: 8 bytes per row in a buffer the library owns per device.  It grows (never shrinks, and a buffer that
// was handed out is never freed: a captured graph keeps its address) on a call outside stream capture; inside a capture a call
// that needs more rows than any call before it on this device is refused.
static u64* lexicon_keys(const char* who, int N, hipStream_t stream) {
  static std::mutex mu;
  static u64* buf[MR_MAX_DEVICES] = {nullptr};
  static long long cap[MR_MAX_DEVICES] = {0};
  const int dev = current_device();
  if (dev < 0) {
    set_error("%s: no current device with an index below %d", who, MR_MAX_DEVICES);
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(mu);
  if (cap[dev] >= N) return buf[dev];
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    set_error("%s: N=%d rows need a larger key buffer than the %lld rows allocated so far, and the stream is "
              "capturing: call once with at least this N before the capture", who, N, cap[dev]);
    return nullptr;
  }
  long long want = cap[dev] > 0 ? 2 * cap[dev] : 8192;
  while (want < N) want *= 2;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)want * sizeof(u64)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: hipMalloc of %lld key rows failed", who, want);
    return nullptr;
  }
  buf[dev] = (u64*)p;
  cap[dev] = want;
  return buf[dev];
}

template <typename PT>
static int launch_transcribe(bool dense, const PT* pred, long long sn, long long sc, long long st, int T, int log_probs,
                             const int* preds, int S, int N, int blank, int unknown, const int* fold, const int* lex_sym,
                             const int* lex_off, int L, const int* span, int C, int max_distance, int chunks, int stage, size_t lds,
                             size_t lds_max, u64* keys, int* pred_len, int* n_cand, float* all_scores, hipStream_t stream) {
  const auto kernel = dense ? lexicon_transcribe_kernel<true, PT> : lexicon_transcribe_kernel<false, PT>;
  const int rc = ensure_dynamic_lds(kernel, lds_max);
  if (rc != MR_OK) return rc;
  // 16-byte loads of 16 columns of one class: f32, columns contiguous, and every (n, c) row 16-byte aligned
  const int vec = sizeof(PT) == 4 && st == 1 && sn % 4 == 0 && sc % 4 == 0 && (uintptr_t)pred % 16 == 0;
  hipLaunchKernelGGL(kernel, dim3(N * chunks), dim3(LEX_BLOCK), lds, stream, pred, sn, sc, st, T, log_probs, vec, stage, preds, S, N,
                     blank, unknown, fold, lex_sym, lex_off, L, span, C, max_distance, chunks, keys, pred_len, n_cand, all_scores);
  return MR_OK;
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
  u64* keys = lexicon_keys("mr_lexicon_nearest", N, stream);
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

int mr_lexicon_transcribe(int dtype, const void* pred, long long sn, long long sc, long long st, int T, int log_probs,
                          const int* preds, int S, int N, int blank, int unknown, const int* fold, const int* lex_sym,
                          const int* lex_off, int L, const int* span, int C, int max_distance, int* best_index,
                          float* best_score, int* best_dist, int* pred_len, int* n_cand, float* all_scores,
                          hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && S >= 0 && L >= 0, "mr_lexicon_transcribe: bad shape N=%d S=%d L=%d", N, S, L);
  MR_CTC_TRY(ctc_check_columns("mr_lexicon_transcribe", T, 0));
  MR_CHECK_ARG(S <= MR_SEQ_MEASURE_MAX, "mr_lexicon_transcribe: S=%d exceeds MR_SEQ_MEASURE_MAX=%d ids per row", S,
               MR_SEQ_MEASURE_MAX);
  MR_CTC_TRY(ctc_check_classes("mr_lexicon_transcribe", C, blank));
  MR_CTC_TRY(ctc_check_dtype("mr_lexicon_transcribe", dtype));
  if (N == 0) return MR_OK;
  MR_CHECK_ARG(pred && best_index && best_score && best_dist && pred_len && n_cand && (S == 0 || preds) &&
                   (L == 0 || (lex_sym && lex_off)),
               "mr_lexicon_transcribe: null pointer");
  // as mr_lexicon_nearest fills the chip; without a distance bound a workgroup's four waves take sixteen words at a time
  const int per = max_distance < 0 ? 16 : LEX_BLOCK;
  const int fill = cdiv(4 * num_cus(), N);
  const int chunks = max(1, min(fill, cdiv(L, per)));
  MR_CHECK_ARG((long long)N * chunks <= INT_MAX, "mr_lexicon_transcribe: N=%d rows x %d slices exceed the grid", N, chunks);
  const bool dense = C <= LEX_DENSE_MAX;
  const int stage = (long long)C * (T | 1) <= LEX_STAGE_MAX;
  const size_t lds = (size_t)(dense ? C : 64) * sizeof(u64) + (size_t)S * sizeof(int) + 64 * sizeof(int) +
                     (stage ? (size_t)C * (T | 1) * sizeof(float) : 0);
  const size_t lds_max = (size_t)LEX_DENSE_MAX * sizeof(u64) + (size_t)MR_SEQ_MEASURE_MAX * sizeof(int) + 64 * sizeof(int) +
                         (size_t)LEX_STAGE_MAX * sizeof(float);
  u64* keys = lexicon_keys("mr_lexicon_transcribe", N, stream);
  if (!keys) return MR_ERR_LAUNCH;
  hipLaunchKernelGGL(lexicon_transcribe_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, keys, N, span, L, max_distance,
                     n_cand);
  if (all_scores && L > 0) {
    const long long count = (long long)N * L;
    hipLaunchKernelGGL(lexicon_fill_kernel, dim3((unsigned)min(cdivll(count, 256), 65536ll)), dim3(256), 0, stream, all_scores,
                       count, CTC_NEG_INF);
  }
  int rc;
  MR_CTC_DISPATCH(dtype, PT, rc = launch_transcribe(dense, (const PT*)pred, sn, sc, st, T, log_probs, preds, S, N, blank, unknown,
                                                    fold, lex_sym, lex_off, L, span, C, max_distance, chunks, stage, lds, lds_max,
                                                    keys, pred_len, n_cand, all_scores, stream));
  if (rc != MR_OK) return rc;
  hipLaunchKernelGGL(lexicon_transcribe_unpack_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, keys, N, preds, S, blank, unknown,
                     fold, lex_sym, lex_off, C, best_index, best_score, best_dist);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
