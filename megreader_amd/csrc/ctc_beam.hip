// CTC prefix beam search (Graves; Hannun et al., "First-pass large vocabulary continuous speech recognition using bi-directional
// recurrent DNNs", Algorithm 1): the n most probable strings of a CTC posterior with their log-probabilities, by the posterior
// alone (mr_ctc_beam_search) or ranked with a character n-gram model (mr_ctc_beam_search_lm).  The rules are written out in
// include/megreader_hip.h; this file is two kernels, the second with a compile-time flag for the model.
//
//   ctc_beam_columns_kernel   one wave per column (n, t): the top_classes symbols of the column by (lp descending, id ascending)
//                             into the workspace lists sym_id / sym_lp [N, T, Kc] (-1 / -inf past the eligible ones).  A lane keeps
//                             the best key of its classes (lane, lane + 64, ...); a round takes the wave maximum and only the lane
//                             that owned it looks for its next one.  The column's logs are taken once and kept in LDS (one f32 per
//                             class, a lane rescans only what it wrote) up to CTCB_STAGE_MAX classes; a wider alphabet
//                             takes them again from global memory on a rescan: slow, exact.
//   ctc_beam_rows_kernel<LM>  one wave per row, sequential in t.  Lane i holds beam entry i (pb, pnb, total, last, length, node,
//                             parent node) in registers, mirrored in LDS for the other lanes.  Per column: the stay candidates by
//                             their own lanes, the B * Kc extensions spread over the lanes, one 64-bit key (ordered total << 32 |
//                             ~index) per candidate in LDS; B rounds of wave maximum pick the survivors in descending order (the
//                             same descent as above), so the beam is always sorted and there is no barrier between waves anywhere.
//                             LM = true adds, and LM = false compiles none of: a model state and an f32 sum lm per beam entry,
//                             total + lm as what a key orders, one lookup in the model (a read-only automaton) per extension, the
//                             end-of-string term and a last ranking of the survivors by total + lm, the two outputs more.  The
//                             masses, the columns and the trie are the same either way.
// Strings are a persistent parent-pointer trie per row in the caller's workspace: an open-addressing table keyed by the exact pair
// (parent node, symbol), whose slot index IS the node id.  A prefix that left the beam and comes back finds its old node, so "the
// extension p + c is beam entry q" is `q.parent == p.node && q.last == c` -- exact, no string hash.  An extension can only meet a
// stay (two extensions of distinct prefixes differ), and a stay at most one extension: lane q looks for its parent among the beam
// and for its last symbol among the column's, adds that extension's mass to its own pnb' and strikes the extension's key out.
// Only the <= B survivors that are new are looked up or created (64-bit compare-and-swap, probes read past the L1); node ids depend
// on the probing order and never reach an output.  The strings are unwound once at the end.
#include <limits.h>
#include "device.h"
#include "ctc_posterior.h"
#include "../../include/megreader_hip.h"

namespace mr {

enum {
  CTCB_STAGE_MAX = 8192,   // classes up to which the column kernel keeps the column's logs in LDS (32 KiB)
  CTCB_AHEAD = 8,          // loads a lane of the column kernel issues before it takes the first log
};
constexpr bool CTCB_MERGE_ZEROS = true;   // ctc_key: -0 and +0 are one value in every key of this file (ctc_posterior.h says why)

template <typename PT>
__global__ __launch_bounds__(64) void ctc_beam_columns_kernel(const PT* pred, long long sn, long long sc, long long st, int C,
                                                              int T, int log_probs, int blank, int unknown, int Kc, int staged,
                                                              int* sym_id, float* sym_lp) {
  extern __shared__ float ctcb_col[];   // staged: C f32; lane l writes classes l, l + 64, ...
  const int lane = threadIdx.x;
  const long long column = blockIdx.x;
  const int n = (int)(column / T), t = (int)(column - (long long)n * T);
  const PT* col = pred + (long long)n * sn + (long long)t * st;
  u64 mine = 0ull;
  // eight loads in flight per lane: with a class's T values contiguous a wave's load touches 64 cache lines, and one at a time
  // the pass waits out the memory latency C / 64 times
  for (int c0 = lane; c0 < C; c0 += 64 * CTCB_AHEAD) {
    float v[CTCB_AHEAD];
#pragma unroll
    for (int u = 0; u < CTCB_AHEAD; ++u) {
      const int c = c0 + 64 * u;
      v[u] = c < C ? to_f32(col[(long long)c * sc]) : 1.f;
    }
#pragma unroll
    for (int u = 0; u < CTCB_AHEAD; ++u) {
      const int c = c0 + 64 * u;
      if (c < C) {
        const float lp = ctc_lp(v[u], log_probs != 0);
        if (staged) ctcb_col[c] = lp;
        const u64 k = (c != blank && c != unknown) ? ctc_key(lp, (unsigned)c, CTCB_MERGE_ZEROS) : 0ull;
        mine = k > mine ? k : mine;
      }
    }
  }
  u64 got = 0ull;
  for (int j = 0; j < Kc; ++j) {
    const u64 w = ctc_wave_max(mine);
    if (w == 0ull) break;   // (wave-uniform) fewer eligible classes than Kc
    if (lane == j) got = w;
    if (mine == w) {        // keys are distinct: one lane.  Its next best below w
      u64 m = 0ull;
      for (int c = lane; c < C; c += 64) {
        const float lp = staged ? ctcb_col[c] : ctc_lp_at(col, sc, c, log_probs != 0);
        const u64 k = (c != blank && c != unknown) ? ctc_key(lp, (unsigned)c, CTCB_MERGE_ZEROS) : 0ull;
        if (k < w && k > m) m = k;
      }
      mine = m;
    }
  }
  __syncthreads();   // lane j reads the log of its winner, which another lane staged
  if (lane < Kc) {
    const int c = (int)(0xffffffffu - (unsigned)(got & 0xffffffffull));
    // the value as it was read, not the one rebuilt from the key (which made -0 a +0)
    const float lp = got ? (staged ? ctcb_col[c] : ctc_lp_at(col, sc, c, log_probs != 0)) : CTC_NEG_INF;
    sym_id[column * Kc + lane] = got ? c : -1;
    sym_lp[column * Kc + lane] = lp;
  }
}

// node of the pair (parent node, symbol) in the row's table: found, or created in the first empty slot of its probe sequence.
// Node id = slot + 1 (0 is the root, the empty string); an entry is (parent << 32) | (symbol + 1), 0 = empty.  The table holds more
// than twice the nodes a row can create, so a probe sequence ends; the loop is bounded all the same.
__device__ __forceinline__ int ctcb_find_or_create(u64* tab, unsigned slots, int parent, int sym) {
  const u64 entry = ((u64)(unsigned)parent << 32) | (u64)(unsigned)(sym + 1);
  unsigned h = ((unsigned)parent * 0x9E3779B1u) ^ ((unsigned)(sym + 1) * 0x85EBCA6Bu);
  h = (h ^ (h >> 15)) % slots;
  for (unsigned probe = 0; probe < slots; ++probe) {
    u64 cur = __hip_atomic_load(tab + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) {
      cur = atomicCAS(tab + h, 0ull, entry);
      if (cur == 0ull) return (int)h + 1;
    }
    if (cur == entry) return (int)h + 1;
    h = h + 1 == slots ? 0u : h + 1;
  }
  return 0;
}

// ---- the character n-gram model of mr_ctc_beam_search_lm ----

// the model as the header lays it out: a finite automaton, its arcs in an open-addressing table keyed by (state, symbol)
struct CtcbModel {
  const u64* keys;
  const float* arc_lp;
  const int* arc_next;
  const float* bow;
  const int* backoff;
  const float* end_lp;
  int states;
  unsigned slots;
  int max_probe, start_state, order;
  float alpha, beta;
  int end;
};

// g(sym | state) and the state after sym: at most `order` levels (the state, then its backoff chain) of at most max_probe
// probes each; the bows are added first, then the arc's value.  -inf: no arc down to state 0.  Plain loads: the model is read only.
// A level is one memory round trip where its first two slots decide it (a table at most half full: nearly always): the two keys,
// the first slot's value and next state, and the state's bow and backoff are loaded together, before any of them is looked at,
// so neither a hit nor a miss waits for a second load behind the first.
__device__ __forceinline__ float ctcb_lm_step(const CtcbModel& lm, int state, int sym, int& next) {
  float acc = 0.f;
  next = 0;
  for (int level = 0; level < lm.order; ++level) {
    if ((unsigned)state >= (unsigned)lm.states) break;
    const u64 entry = ((u64)(unsigned)state << 32) | (u64)(unsigned)(sym + 1);
    unsigned h = ((unsigned)state * 0x9E3779B1u) ^ ((unsigned)(sym + 1) * 0x85EBCA6Bu);
    h = (h ^ (h >> 15)) % lm.slots;
    const unsigned h1 = h + 1 == lm.slots ? 0u : h + 1;
    const u64 k0 = lm.keys[h], k1 = lm.keys[h1];
    const float v0 = lm.arc_lp[h], bow = lm.bow[state];
    const int n0 = lm.arc_next[h], backoff = lm.backoff[state];   // -1 behind state 0: the range check above ends the chain
    if (k0 == entry) {
      next = n0;
      return __fadd_rn(acc, v0);
    }
    if (k0 != 0ull && lm.max_probe > 1) {
      h = h1;
      u64 cur = k1;
      for (int probe = 1;;) {
        if (cur == entry) {
          next = lm.arc_next[h];
          return __fadd_rn(acc, lm.arc_lp[h]);
        }
        if (cur == 0ull || ++probe >= lm.max_probe) break;
        h = h + 1 == lm.slots ? 0u : h + 1;
        cur = lm.keys[h];
      }
    }
    acc = __fadd_rn(acc, bow);
    state = backoff;
  }
  return CTC_NEG_INF;
}

// lm(p + c) from lm(p) and g: every operation rounded on its own
__device__ __forceinline__ float ctcb_lm_add(const CtcbModel& lm, float sum, float g) {
  return __fadd_rn(sum, __fadd_rn(__fmul_rn(lm.alpha, g), lm.beta));
}

// a total as mr_ctc_beam_search takes it back out of a key: -0 is +0
__device__ __forceinline__ float ctcb_plus_zero(float v) { return v == 0.f ? 0.f : v; }

// The row kernel.  LM: with the model -- two more values per beam entry, the model state and the f32 sum lm, mirrored in LDS like
// the others.  The masses are computed the same either way; with the model the candidate keys order total + lm, so a survivor's
// total is taken again from its masses (the same operations, the same bits) where the plain search reads it back out of the key.
// The lanes that build the extension keys look the model up, one lookup per (p, j), independent of each other; the <= B lanes whose
// survivor is an extension repeat theirs for the new state instead of keeping 4 096 states in LDS.
template <typename PT, bool LM>
__global__ __launch_bounds__(64) void ctc_beam_rows_kernel(const PT* pred, long long sn, long long sc, long long st, int C, int T,
                                                           int log_probs, int blank, int B, int K, int Kc, const int* sym_id,
                                                           const float* sym_lp, u64* tables, unsigned slots, CtcbModel lm, int* ids,
                                                           int* lengths, float* scores, float* ctc_scores, float* lm_scores,
                                                           int* count) {
  // candidate keys: [0, 64) the stay of beam entry q; 64 + p * kc + j the extension of entry p by the column's j-th symbol
  __shared__ u64 keys[MR_CTC_BEAM_MAX + MR_CTC_BEAM_MAX * MR_CTC_BEAM_TOP_MAX];
  __shared__ float b_pb[64], b_pnb[64], b_tot[64], s_pb[64], s_pnb[64], c_lp[64];
  __shared__ int b_last[64], b_len[64], b_node[64], b_par[64], c_id[64];
  __shared__ float b_lm[LM ? 64 : 1];   // without the model nothing refers to these two: they take no LDS
  __shared__ int b_state[LM ? 64 : 1];
  const int lane = threadIdx.x, n = blockIdx.x;
  u64* tab = tables + (long long)n * slots;
  for (unsigned i = lane; i < slots; i += 64) tab[i] = 0ull;
  // beam entry `lane`: the start state is the empty prefix alone
  float pb = lane == 0 ? 0.f : CTC_NEG_INF, pnb = CTC_NEG_INF, tot = pb, lms = 0.f;
  int last = -1, len = 0, node = 0, par = -1, nb = 1, state = LM ? lm.start_state : 0;
  // what the extension of entry p by symbol c grows out of: a repeat of p's last symbol only out of the paths that end in a blank
  const auto from = [&](int p, int c) { return (b_len[p] > 0 && b_last[p] == c) ? b_pb[p] : b_tot[p]; };
  __syncthreads();   // the zeroed table has landed before the first compare-and-swap
  for (int t = 0; t < T; ++t) {
    const PT* col = pred + (long long)n * sn + (long long)t * st;
    const long long list = ((long long)n * T + t) * Kc;
    const int cid = lane < Kc ? sym_id[list + lane] : -1;
    const float clp = lane < Kc ? sym_lp[list + lane] : CTC_NEG_INF;
    const float lpb = ctc_lp_at(col, sc, blank, log_probs != 0);
    const int kc = __popcll(__ballot(cid >= 0));   // the eligible ones come first
    b_pb[lane] = pb; b_pnb[lane] = pnb; b_tot[lane] = tot;
    b_last[lane] = last; b_len[lane] = len; b_node[lane] = node; b_par[lane] = par;
    if constexpr (LM) { b_lm[lane] = lms; b_state[lane] = state; }
    c_id[lane] = cid; c_lp[lane] = clp;
    __syncthreads();
    // stay: lane q, with the one extension that spells the same string (so its state and lm are the same too)
    u64 key = 0ull;
    int merged = -1;
    if (lane < nb) {
      const float npb = tot + lpb;
      float npnb = CTC_NEG_INF;
      if (len > 0) {
        int jl = -1;
        for (int j = 0; j < kc; ++j)
          if (c_id[j] == last) jl = j;
        npnb = pnb + (jl >= 0 ? c_lp[jl] : ctc_lp_at(col, sc, last, log_probs != 0));   // the same bits either way
        if (jl >= 0) {
          int p = -1;
          for (int i = 0; i < nb; ++i)
            if (b_node[i] == par) p = i;
          if (p >= 0) {
            npnb = ctc_lse2(npnb, from(p, last) + c_lp[jl]);
            merged = p * kc + jl;
          }
        }
      }
      s_pb[lane] = npb; s_pnb[lane] = npnb;
      float ranked = ctc_lse2(npb, npnb);
      if constexpr (LM) ranked = __fadd_rn(ranked, lms);
      key = ctc_key(ranked, (unsigned)lane, CTCB_MERGE_ZEROS);
    }
    keys[lane] = key;
    const int ne = nb * kc;
    for (int e = lane; e < ne; e += 64) {
      const int p = e / kc, j = e - p * kc;
      float ranked = from(p, c_id[j]) + c_lp[j];
      if constexpr (LM) {
        int next;
        const float g = ctcb_lm_step(lm, b_state[p], c_id[j], next);
        ranked = g > CTC_NEG_INF ? __fadd_rn(ranked, ctcb_lm_add(lm, b_lm[p], g)) : CTC_NEG_INF;
      }
      keys[64 + e] = ctc_key(ranked, (unsigned)(64 + e), CTCB_MERGE_ZEROS);
    }
    __syncthreads();
    if (merged >= 0) keys[64 + merged] = 0ull;
    __syncthreads();
    // keep: the B greatest in descending order; lane r takes the r-th
    u64 mine = keys[lane];
    for (int e = lane; e < ne; e += 64) mine = keys[64 + e] > mine ? keys[64 + e] : mine;
    u64 got = 0ull;
    int kept = 0;
    for (int r = 0; r < B; ++r) {
      const u64 w = ctc_wave_max(mine);
      if (w == 0ull) break;   // (wave-uniform) nothing finite is left
      if (lane == r) got = w;
      ++kept;
      if (mine == w) {
        u64 m = keys[lane] < w ? keys[lane] : 0ull;
        for (int e = lane; e < ne; e += 64) {
          const u64 k = keys[64 + e];
          if (k < w && k > m) m = k;
        }
        mine = m;
      }
    }
    nb = kept;
    if (lane < nb) {
      const int idx = (int)(0xffffffffu - (unsigned)(got & 0xffffffffull));
      if constexpr (!LM) tot = ctc_unordered((unsigned)(got >> 32));   // the key holds the total itself (-0 as +0)
      if (idx < 64) {
        pb = s_pb[idx]; pnb = s_pnb[idx]; last = b_last[idx]; len = b_len[idx]; node = b_node[idx]; par = b_par[idx];
        if constexpr (LM) {
          state = b_state[idx]; lms = b_lm[idx];
          tot = ctcb_plus_zero(ctc_lse2(pb, pnb));
        }
      } else {
        const int e = idx - 64, p = e / kc, j = e - p * kc;
        if constexpr (LM) tot = ctcb_plus_zero(from(p, c_id[j]) + c_lp[j]);
        pb = CTC_NEG_INF; pnb = tot; last = c_id[j]; len = b_len[p] + 1; par = b_node[p];
        if constexpr (LM) lms = ctcb_lm_add(lm, b_lm[p], ctcb_lm_step(lm, b_state[p], last, state));
        node = ctcb_find_or_create(tab, slots, par, last);
      }
    } else {
      pb = pnb = tot = CTC_NEG_INF; last = -1; len = 0; node = 0; par = -1;
      if constexpr (LM) { state = 0; lms = 0.f; }
    }
    __syncthreads();   // every read of the old beam is done before the next column overwrites it
  }
  // entry `lane` is returned in place `rank` if `have`; `alive` entries are left.  Without the model the beam is in order already
  int rank = lane, alive = nb;
  bool have = lane < nb && lane < K;
  float score = tot;
  if constexpr (LM) {
    // the end of the string, then the survivors' ranks by total + lm: at most 64 keys, one per lane, each lane counts the greater
    if (lm.end != 0 && lane < nb && (unsigned)state < (unsigned)lm.states)
      lms = __fadd_rn(lms, __fmul_rn(lm.alpha, lm.end_lp[state]));
    score = lane < nb ? __fadd_rn(tot, lms) : CTC_NEG_INF;
    keys[lane] = ctc_key(score, (unsigned)lane, CTCB_MERGE_ZEROS);
    __syncthreads();
    rank = alive = 0;
    for (int i = 0; i < 64; ++i) {
      rank += keys[i] > keys[lane] ? 1 : 0;
      alive += keys[i] != 0ull ? 1 : 0;
    }
    have = keys[lane] != 0ull && rank < K;
    __syncthreads();   // b_len is read as the ranks' lengths below, the keys are done with
  }
  const int returned = min(alive, K);
  if (lane < K) b_len[lane] = 0;
  __syncthreads();
  if (have) b_len[rank] = len;
  if (lane < K && lane >= returned) {
    lengths[(long long)n * K + lane] = 0;
    scores[(long long)n * K + lane] = CTC_NEG_INF;
    if constexpr (LM) {
      ctc_scores[(long long)n * K + lane] = CTC_NEG_INF;
      lm_scores[(long long)n * K + lane] = CTC_NEG_INF;
    }
  }
  if (have) {
    lengths[(long long)n * K + rank] = len;
    scores[(long long)n * K + rank] = score;
    if constexpr (LM) {
      ctc_scores[(long long)n * K + rank] = tot;
      lm_scores[(long long)n * K + rank] = lms;
    }
  }
  if (lane == 0) count[n] = returned;
  __syncthreads();
  int* out = ids + (long long)n * K * T;
  for (long long i = lane; i < (long long)K * T; i += 64) {
    const int k = (int)(i / T), tt = (int)(i - (long long)k * T);
    if (tt >= b_len[k]) out[i] = blank;
  }
  if (have) {
    int nd = node;
    for (int i = len - 1; i >= 0 && nd > 0; --i) {
      const u64 entry = __hip_atomic_load(tab + (nd - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[(long long)rank * T + i] = (int)(unsigned)(entry & 0xffffffffull) - 1;
      nd = (int)(unsigned)(entry >> 32);
    }
  }
}

// nodes a row can create are at most T * beam; the table is kept under half full
static inline long long ctcb_slots(int T, int beam) { return 2ll * T * beam + 64; }

static long long ctcb_ws_bytes(long long N, int T, int beam, int top_classes) {
  if (N < 1 || T < 1 || T > MR_SEQ_MEASURE_MAX || beam < 1 || beam > MR_CTC_BEAM_MAX || top_classes < 1 ||
      top_classes > MR_CTC_BEAM_TOP_MAX)
    return 0;
  const long long lists = N * T * top_classes * (long long)(sizeof(int) + sizeof(float));
  const long long tables = N * ctcb_slots(T, beam) * (long long)sizeof(u64);
  return lists + tables <= INT_MAX ? lists + tables : 0;
}

// Both entry points: the checks in the order they are reported, the workspace, the two launches.  lm: the model, or null for the
// search by the posterior alone, which neither looks at ctc_scores and lm_scores nor writes them
static int ctcb_search(const char* who, int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T,
                       int log_probs, int blank, int unknown, int beam, int nbest, int top_classes, const CtcbModel* lm, int* ids,
                       int* lengths, float* scores, float* ctc_scores, float* lm_scores, int* count, void* ws, long long ws_bytes,
                       hipStream_t stream) {
  MR_CHECK_ARG(N >= 0, "%s: N=%d rows", who, N);
  MR_CTC_TRY(ctc_check_columns(who, T, MR_SEQ_MEASURE_MAX));
  MR_CTC_TRY(ctc_check_classes(who, C, blank));
  MR_CHECK_ARG(beam >= 1 && beam <= MR_CTC_BEAM_MAX, "%s: beam=%d (1..MR_CTC_BEAM_MAX=%d)", who, beam, MR_CTC_BEAM_MAX);
  MR_CHECK_ARG(nbest >= 1 && nbest <= beam, "%s: nbest=%d (1..beam=%d)", who, nbest, beam);
  MR_CHECK_ARG(top_classes >= 1 && top_classes <= MR_CTC_BEAM_TOP_MAX, "%s: top_classes=%d (1..MR_CTC_BEAM_TOP_MAX=%d)", who,
               top_classes, MR_CTC_BEAM_TOP_MAX);
  if (lm) {
    MR_CHECK_ARG(lm->order >= 1 && lm->order <= MR_NGRAM_ORDER_MAX, "%s: order=%d (1..MR_NGRAM_ORDER_MAX=%d)", who, lm->order,
                 MR_NGRAM_ORDER_MAX);
    MR_CHECK_ARG(lm->states >= 1 && (int)lm->slots >= 1 && lm->max_probe >= 1, "%s: states=%d slots=%d max_probe=%d (each >= 1)",
                 who, lm->states, (int)lm->slots, lm->max_probe);
    MR_CHECK_ARG(lm->start_state >= 0 && lm->start_state < lm->states, "%s: start_state=%d is not one of %d states", who,
                 lm->start_state, lm->states);
    MR_CHECK_ARG(lm->alpha - lm->alpha == 0.f && lm->beta - lm->beta == 0.f, "%s: alpha=%g beta=%g must be finite", who,
                 (double)lm->alpha, (double)lm->beta);
    MR_CHECK_ARG(lm->keys && lm->arc_lp && lm->arc_next && lm->bow && lm->backoff && lm->end_lp, "%s: null model pointer", who);
  }
  MR_CTC_TRY(ctc_check_dtype(who, dtype));
  if (N == 0) return MR_OK;
  MR_CTC_TRY(ctc_check_workspace(who, "mr_ctc_beam_ws_bytes", ws, ws_bytes, ctcb_ws_bytes(N, T, beam, top_classes)));
  MR_CHECK_ARG(pred && ids && lengths && scores && count && (!lm || (ctc_scores && lm_scores)), "%s: null pointer", who);
  MR_CHECK_ARG((long long)N * T <= INT_MAX, "%s: N=%d rows x T=%d columns exceed the grid", who, N, T);
  const long long cells = (long long)N * T * top_classes;
  int* sym_id = (int*)ws;
  float* sym_lp = (float*)(sym_id + cells);
  u64* tables = (u64*)(sym_lp + cells);
  const unsigned slots = (unsigned)ctcb_slots(T, beam);
  const int staged = C <= CTCB_STAGE_MAX;
  const size_t lds = staged ? (size_t)C * sizeof(float) : 0;
  const int Kc = top_classes;
  MR_CTC_DISPATCH(dtype, PT,
                  hipLaunchKernelGGL(ctc_beam_columns_kernel<PT>, dim3((unsigned)(N * T)), dim3(64), lds, stream, (const PT*)pred,
                                     sn, sc, st, C, T, log_probs, blank, unknown, Kc, staged, sym_id, sym_lp);
                  if (lm)
                    hipLaunchKernelGGL((ctc_beam_rows_kernel<PT, true>), dim3(N), dim3(64), 0, stream, (const PT*)pred, sn, sc, st,
                                       C, T, log_probs, blank, beam, nbest, Kc, sym_id, sym_lp, tables, slots, *lm, ids, lengths,
                                       scores, ctc_scores, lm_scores, count);
                  else
                    hipLaunchKernelGGL((ctc_beam_rows_kernel<PT, false>), dim3(N), dim3(64), 0, stream, (const PT*)pred, sn, sc, st,
                                       C, T, log_probs, blank, beam, nbest, Kc, sym_id, sym_lp, tables, slots, CtcbModel{}, ids,
                                       lengths, scores, nullptr, nullptr, count));
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_ctc_beam_ws_bytes(int N, int T, int beam, int top_classes) { return (int)ctcb_ws_bytes(N, T, beam, top_classes); }

int mr_ctc_beam_search(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T, int log_probs,
                       int blank, int unknown, int beam, int nbest, int top_classes, int* ids, int* lengths, float* scores,
                       int* count, void* ws, long long ws_bytes, hipStream_t stream) {
  return ctcb_search("mr_ctc_beam_search", dtype, pred, sn, sc, st, N, C, T, log_probs, blank, unknown, beam, nbest, top_classes,
                     nullptr, ids, lengths, scores, nullptr, nullptr, count, ws, ws_bytes, stream);
}

int mr_ctc_beam_search_lm(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T, int log_probs,
                          int blank, int unknown, int beam, int nbest, int top_classes, const unsigned long long* lm_keys,
                          const float* lm_arc_lp, const int* lm_arc_next, const float* lm_bow, const int* lm_backoff,
                          const float* lm_end_lp, int states, int slots, int max_probe, int start_state, int order, float alpha,
                          float beta, int end, int* ids, int* lengths, float* scores, float* ctc_scores, float* lm_scores,
                          int* count, void* ws, long long ws_bytes, hipStream_t stream) {
  const CtcbModel lm = {lm_keys, lm_arc_lp, lm_arc_next, lm_bow, lm_backoff, lm_end_lp, states, (unsigned)slots, max_probe,
                        start_state, order, alpha, beta, end};
  return ctcb_search("mr_ctc_beam_search_lm", dtype, pred, sn, sc, st, N, C, T, log_probs, blank, unknown, beam, nbest,
                     top_classes, &lm, ids, lengths, scores, ctc_scores, lm_scores, count, ws, ws_bytes, stream);
}

}  // extern "C"
