// CTC prefix beam search (Graves; Hannun et al., "First-pass large vocabulary continuous speech recognition using bi-directional
// recurrent DNNs", Algorithm 1, without the language model): the n most probable strings of a CTC posterior with their
// log-probabilities.  The rule is written out in include/megreader_hip.h (mr_ctc_beam_search); this file is two kernels.
//
//   ctc_beam_columns_kernel   one wave per column (n, t): the top_classes symbols of the column by (lp descending, id ascending)
//                             into the workspace lists sym_id / sym_lp [N, T, Kc] (-1 / -inf past the eligible ones).  A lane keeps
//                             the best key of its classes (lane, lane + 64, ...); a round takes the wave maximum and only the lane
//                             that owned it looks for its next one.  The column's logs are taken once and kept in LDS (one f32 per
//                             class, a lane rescans only what it wrote) up to CTCB_STAGE_MAX classes; a wider alphabet
//                             takes them again from global memory on a rescan: slow, exact.
//   ctc_beam_kernel           one wave per row, sequential in t.  Lane i holds beam entry i (pb, pnb, total, last, length, node,
//                             parent node) in registers, mirrored in LDS for the other lanes.  Per column: the stay candidates by
//                             their own lanes, the B * Kc extensions spread over the lanes, one 64-bit key (ordered total << 32 |
//                             ~index) per candidate in LDS; B rounds of wave maximum pick the survivors in descending order (the
//                             same descent as above), so the beam is always sorted and there is no barrier between waves anywhere.
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

template <typename PT>
__global__ __launch_bounds__(64) void ctc_beam_kernel(const PT* pred, long long sn, long long sc, long long st, int C, int T,
                                                      int log_probs, int blank, int B, int K, int Kc, const int* sym_id,
                                                      const float* sym_lp, u64* tables, unsigned slots, int* ids, int* lengths,
                                                      float* scores, int* count) {
  // candidate keys: [0, 64) the stay of beam entry q; 64 + p * kc + j the extension of entry p by the column's j-th symbol
  __shared__ u64 keys[MR_CTC_BEAM_MAX + MR_CTC_BEAM_MAX * MR_CTC_BEAM_TOP_MAX];
  __shared__ float b_pb[64], b_pnb[64], b_tot[64], s_pb[64], s_pnb[64], c_lp[64];
  __shared__ int b_last[64], b_len[64], b_node[64], b_par[64], c_id[64];
  const int lane = threadIdx.x, n = blockIdx.x;
  u64* tab = tables + (long long)n * slots;
  for (unsigned i = lane; i < slots; i += 64) tab[i] = 0ull;
  // beam entry `lane`: the start state is the empty prefix alone
  float pb = lane == 0 ? 0.f : CTC_NEG_INF, pnb = CTC_NEG_INF, tot = pb;
  int last = -1, len = 0, node = 0, par = -1, nb = 1;
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
    c_id[lane] = cid; c_lp[lane] = clp;
    __syncthreads();
    // stay: lane q, with the one extension that spells the same string
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
            const float from = (b_len[p] > 0 && b_last[p] == last) ? b_pb[p] : b_tot[p];
            npnb = ctc_lse2(npnb, from + c_lp[jl]);
            merged = p * kc + jl;
          }
        }
      }
      s_pb[lane] = npb; s_pnb[lane] = npnb;
      key = ctc_key(ctc_lse2(npb, npnb), (unsigned)lane, CTCB_MERGE_ZEROS);
    }
    keys[lane] = key;
    const int ne = nb * kc;
    for (int e = lane; e < ne; e += 64) {
      const int p = e / kc, j = e - p * kc;
      const float from = (b_len[p] > 0 && b_last[p] == c_id[j]) ? b_pb[p] : b_tot[p];
      keys[64 + e] = ctc_key(from + c_lp[j], (unsigned)(64 + e), CTCB_MERGE_ZEROS);
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
      tot = ctc_unordered((unsigned)(got >> 32));
      if (idx < 64) {
        pb = s_pb[idx]; pnb = s_pnb[idx]; last = b_last[idx]; len = b_len[idx]; node = b_node[idx]; par = b_par[idx];
      } else {
        const int e = idx - 64, p = e / kc, j = e - p * kc;
        pb = CTC_NEG_INF; pnb = tot; last = c_id[j]; len = b_len[p] + 1; par = b_node[p];
        node = ctcb_find_or_create(tab, slots, par, last);
      }
    } else {
      pb = pnb = tot = CTC_NEG_INF; last = -1; len = 0; node = 0; par = -1;
    }
    __syncthreads();   // every read of the old beam is done before the next column overwrites it
  }
  // the K best are lanes 0 .. K-1 already
  const bool have = lane < nb && lane < K;
  b_len[lane] = have ? len : 0;
  if (lane < K) {
    lengths[(long long)n * K + lane] = have ? len : 0;
    scores[(long long)n * K + lane] = have ? tot : CTC_NEG_INF;
  }
  if (lane == 0) count[n] = min(nb, K);
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
      out[(long long)lane * T + i] = (int)(unsigned)(entry & 0xffffffffull) - 1;
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

}  // namespace mr

using namespace mr;

extern "C" {

int mr_ctc_beam_ws_bytes(int N, int T, int beam, int top_classes) { return (int)ctcb_ws_bytes(N, T, beam, top_classes); }

int mr_ctc_beam_search(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T, int log_probs,
                       int blank, int unknown, int beam, int nbest, int top_classes, int* ids, int* lengths, float* scores,
                       int* count, void* ws, long long ws_bytes, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0, "mr_ctc_beam_search: N=%d rows", N);
  MR_CTC_TRY(ctc_check_columns("mr_ctc_beam_search", T, MR_SEQ_MEASURE_MAX));
  MR_CTC_TRY(ctc_check_classes("mr_ctc_beam_search", C, blank));
  MR_CHECK_ARG(beam >= 1 && beam <= MR_CTC_BEAM_MAX, "mr_ctc_beam_search: beam=%d (1..MR_CTC_BEAM_MAX=%d)", beam,
               MR_CTC_BEAM_MAX);
  MR_CHECK_ARG(nbest >= 1 && nbest <= beam, "mr_ctc_beam_search: nbest=%d (1..beam=%d)", nbest, beam);
  MR_CHECK_ARG(top_classes >= 1 && top_classes <= MR_CTC_BEAM_TOP_MAX,
               "mr_ctc_beam_search: top_classes=%d (1..MR_CTC_BEAM_TOP_MAX=%d)", top_classes, MR_CTC_BEAM_TOP_MAX);
  MR_CTC_TRY(ctc_check_dtype("mr_ctc_beam_search", dtype));
  if (N == 0) return MR_OK;
  MR_CTC_TRY(ctc_check_workspace("mr_ctc_beam_search", "mr_ctc_beam_ws_bytes", ws, ws_bytes,
                                 ctcb_ws_bytes(N, T, beam, top_classes)));
  MR_CHECK_ARG(pred && ids && lengths && scores && count, "mr_ctc_beam_search: null pointer");
  MR_CHECK_ARG((long long)N * T <= INT_MAX, "mr_ctc_beam_search: N=%d rows x T=%d columns exceed the grid", N, T);
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
                  hipLaunchKernelGGL(ctc_beam_kernel<PT>, dim3(N), dim3(64), 0, stream, (const PT*)pred, sn, sc, st, C, T,
                                     log_probs, blank, beam, nbest, Kc, sym_id, sym_lp, tables, slots, ids, lengths, scores,
                                     count));
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
