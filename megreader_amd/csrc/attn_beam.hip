// Beam search over the attention decoder (decoders/attention_decoder.py: AttentionDecoder.read with beam > 1).  The hypotheses of
// image n are the rows n * B + b of the per-step kernels (mr_gemm_nt, mr_attn_fwd2, mr_gru_fwd2), which take any number of rows;
// what a beam adds per decode step is ONE selection launch, mr_attn_beam_step, and behind the loop the trace of the parents,
// mr_attn_beam_trace.  The rules are written out in include/megreader_hip.h; this file is two kernels.
//
// attn_beam_step_kernel: a workgroup of 256 per image.
//   1. a wave per hypothesis row: the log-sum-exp of its logits in f32 (maximum, then the sum of exp in ascending c per lane and
//      the wave's tree) -- a candidate's value is score[b] + ((logit - max) - log sum);
//   2. B rounds of selection as in ctc_beam.hip: a thread holds the best 64-bit key (ordered value over 2^32 - 1 - index) of its
//      candidates e = b * C + c (e = tid, tid + 256, ..), a round takes the workgroup's maximum (wave maxima through LDS, one
//      barrier a round) and only the thread that owned it looks for its next best below.  Keys are distinct, so the order is
//      total: the greater value, then the smaller index;
//   3. the state of the new slots, the fed words, and the gather of the parents' h' rows into the buffer the next step reads.
// The logits of an image (B * C values) are read from global memory in 1 and again in every rescan of 2: they stay in the
// vector L1 / L2, and looping over the classes is what takes any C.
//
// attn_beam_trace_kernel: a thread per (image, returned hypothesis) follows the parents back.
#include <limits.h>
#include "ctc_posterior.h"
#include "../../include/megreader_hip.h"

namespace mr {

enum { AB_THREADS = 256, AB_WAVES = AB_THREADS / 64 };

// value of candidate (b, c): the hypothesis' score plus the log-probability of the class; a finished hypothesis offers its blank
// at its own score; -inf (no key) for everything that is no candidate
template <typename T>
__device__ __forceinline__ float ab_value(const T* rows, long long ldl, int b, int c, int blank, const float* sc, const int* fin,
                                          const float* mx, const float* ls) {
  if (!(sc[b] > CTC_NEG_INF)) return CTC_NEG_INF;                 // a dead slot (or a NaN score)
  if (fin[b]) return c == blank ? sc[b] : CTC_NEG_INF;
  if (!(mx[b] > CTC_NEG_INF)) return CTC_NEG_INF;                 // every logit -inf
  return sc[b] + ((to_f32(rows[(long long)b * ldl + c]) - mx[b]) - ls[b]);
}

// the best key of this thread's candidates that is below `below`
template <typename T>
__device__ __forceinline__ u64 ab_best_below(const T* rows, long long ldl, int B, int C, int blank, const float* sc,
                                             const int* fin, const float* mx, const float* ls, int tid, u64 below) {
  u64 best = 0ull;
  const unsigned total = (unsigned)B * (unsigned)C;
  unsigned b = (unsigned)tid / (unsigned)C, c = (unsigned)tid % (unsigned)C;
  const unsigned db = AB_THREADS / (unsigned)C, dc = AB_THREADS % (unsigned)C;
  for (unsigned e = tid; e < total; e += AB_THREADS) {
    const u64 k = ctc_key(ab_value(rows, ldl, (int)b, (int)c, blank, sc, fin, mx, ls), e, true);
    if (k < below && k > best) best = k;
    b += db;
    c += dc;
    if (c >= (unsigned)C) { c -= C; ++b; }
  }
  return best;
}

template <typename T>
__global__ __launch_bounds__(AB_THREADS) void attn_beam_step_kernel(const T* __restrict__ logits, long long ldl,
                                                                    const T* __restrict__ hprime, T* __restrict__ h_next, int H,
                                                                    float* score, int* finished, int* length, int* parent,
                                                                    int* word, long long* feed, int s, int N, int B, int C,
                                                                    int blank) {
  __shared__ float sc[MR_ATTN_BEAM_MAX], mx[MR_ATTN_BEAM_MAX], ls[MR_ATTN_BEAM_MAX], nsc[MR_ATTN_BEAM_MAX];
  __shared__ int fin[MR_ATTN_BEAM_MAX], len[MR_ATTN_BEAM_MAX], npar[MR_ATTN_BEAM_MAX], nword[MR_ATTN_BEAM_MAX];
  __shared__ u64 wmax[2][AB_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long r0 = (long long)n * B;
  const T* rows = logits + r0 * ldl;
  if (tid < B) {
    // step 0: the start state (h0 = 0, fed `blank`) in slot 0 and nothing else, whatever the buffers hold
    sc[tid] = s == 0 ? (tid == 0 ? 0.f : CTC_NEG_INF) : score[r0 + tid];
    fin[tid] = s == 0 ? 0 : finished[r0 + tid];
    len[tid] = s == 0 ? 0 : length[r0 + tid];
  }
  __syncthreads();
  for (int b = wave; b < B; b += AB_WAVES) {
    if (!(sc[b] > CTC_NEG_INF) || fin[b]) continue;              // (wave-uniform: its logits are not read)
    const T* row = rows + (long long)b * ldl;
    float m = CTC_NEG_INF;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, to_f32(row[c]));
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(to_f32(row[c]) - m);
    sum = wave_sum(sum);
    if (lane == 0) {
      mx[b] = m;
      ls[b] = logf(sum);
    }
  }
  __syncthreads();

  u64 mine = ab_best_below(rows, ldl, B, C, blank, sc, fin, mx, ls, tid, ~0ull);
  for (int j = 0; j < B; ++j) {
    const u64 wm = ctc_wave_max(mine);
    if (lane == 0) wmax[j & 1][wave] = wm;
    __syncthreads();
    u64 w = wmax[j & 1][0];
#pragma unroll
    for (int i = 1; i < AB_WAVES; ++i) w = wmax[j & 1][i] > w ? wmax[j & 1][i] : w;
    if (w != 0ull && mine == w) {                                // keys are distinct: one thread
      const unsigned e = 0xffffffffu - (unsigned)(w & 0xffffffffull);
      const int b = (int)(e / (unsigned)C), c = (int)(e % (unsigned)C);
      npar[j] = b;
      nword[j] = c;
      nsc[j] = ab_value(rows, ldl, b, c, blank, sc, fin, mx, ls);  // (the value as computed, not the key's: -0 stays -0)
      mine = ab_best_below(rows, ldl, B, C, blank, sc, fin, mx, ls, tid, w);
    } else if (w == 0ull && tid == 0) {                          // fewer candidates than slots: a dead slot
      npar[j] = 0;
      nword[j] = blank;
      nsc[j] = CTC_NEG_INF;
    }
  }
  __syncthreads();

  if (tid < B) {
    const int p = npar[tid], c = nword[tid];
    const bool dead = !(nsc[tid] > CTC_NEG_INF);
    const bool was = fin[p] != 0;
    const long long o = ((long long)s * N + n) * B + tid;
    parent[o] = p;
    word[o] = c;
    score[r0 + tid] = nsc[tid];
    finished[r0 + tid] = dead ? 0 : (was || c == blank) ? 1 : 0;
    length[r0 + tid] = dead ? 0 : was ? len[p] : c == blank ? s : s + 1;
    feed[r0 + tid] = c;
  }
  // h_next[n * B + j] = h'[n * B + parent[j]]: 16-byte pieces where the rows allow, else elements
  const long long row_bytes = (long long)H * (long long)sizeof(T);
  if (row_bytes % 16 == 0 && (((uintptr_t)hprime | (uintptr_t)h_next) & 15) == 0) {
    const int pieces = (int)(row_bytes / 16);
    for (int i = tid; i < B * pieces; i += AB_THREADS) {
      const int j = i / pieces, q = i - j * pieces;
      ((uint4*)(h_next + (r0 + j) * H))[q] = ((const uint4*)(hprime + (r0 + npar[j]) * H))[q];
    }
  } else {
    for (int i = tid; i < B * H; i += AB_THREADS) {
      const int j = i / H, q = i - j * H;
      h_next[(r0 + j) * H + q] = hprime[(r0 + npar[j]) * H + q];
    }
  }
}

__global__ __launch_bounds__(64) void attn_beam_trace_kernel(const int* __restrict__ parent, const int* __restrict__ word,
                                                             const float* __restrict__ score, const int* __restrict__ finished,
                                                             const int* __restrict__ length, int S, int N, int B, int nbest,
                                                             int blank, int* __restrict__ ids, int* __restrict__ lengths,
                                                             float* __restrict__ scores, int* __restrict__ count,
                                                             int* __restrict__ path) {
  const long long i = blockIdx.x * 64ll + threadIdx.x;
  if (i >= (long long)N * nbest) return;
  const int n = (int)(i / nbest), j = (int)(i % nbest);
  const long long r0 = (long long)n * B;
  const float sc = score[r0 + j];
  const bool live = sc > CTC_NEG_INF;
  int* id = ids + i * S;
  int* pa = path + i * (S + 1);
  scores[i] = live ? sc : CTC_NEG_INF;
  lengths[i] = live ? (finished[r0 + j] ? length[r0 + j] : S) : 0;
  if (j == 0) {                                                  // slots are in descending order: the live ones come first
    int k = 0;
    for (int q = 0; q < nbest; ++q) k += score[r0 + q] > CTC_NEG_INF ? 1 : 0;
    count[n] = k;
  }
  if (!live) {
    for (int s = 0; s < S; ++s) id[s] = blank;
    for (int s = 0; s <= S; ++s) pa[s] = 0;
    return;
  }
  int cur = j;
  pa[S] = cur;
  for (int s = S - 1; s >= 0; --s) {
    const long long o = ((long long)s * N + n) * B + cur;
    id[s] = word[o];
    cur = parent[o];
    pa[s] = cur;
  }
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_attn_beam_step(int dtype, const void* logits, long long ldl, const void* hprime, void* h_next, int H, float* score,
                      int* finished, int* length, int* parent, int* word, long long* feed, int s, int S, int N, int B, int C,
                      int blank, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && H >= 1 && S >= 1 && s >= 0 && s < S, "mr_attn_beam_step: bad shape N=%d H=%d, step %d of S=%d", N, H, s, S);
  MR_CHECK_ARG(B >= 1 && B <= MR_ATTN_BEAM_MAX, "mr_attn_beam_step: beam=%d (1..MR_ATTN_BEAM_MAX=%d)", B, MR_ATTN_BEAM_MAX);
  MR_CHECK_ARG(C >= 1 && C <= INT_MAX / MR_ATTN_BEAM_MAX && ldl >= C, "mr_attn_beam_step: C=%d classes with ldl=%lld", C, ldl);
  MR_CHECK_ARG(blank >= 0 && blank < C, "mr_attn_beam_step: blank=%d is not a class of C=%d", blank, C);
  MR_CTC_TRY(ctc_check_dtype("mr_attn_beam_step", dtype));
  if (N == 0) return MR_OK;
  MR_CHECK_ARG(logits && hprime && h_next && hprime != h_next && score && finished && length && parent && word && feed,
               "mr_attn_beam_step: null pointer (or h_next == hprime: the gather is not in place)");
  MR_CTC_DISPATCH(dtype, PT,
                  hipLaunchKernelGGL(attn_beam_step_kernel<PT>, dim3((unsigned)N), dim3(AB_THREADS), 0, stream,
                                     (const PT*)logits, ldl, (const PT*)hprime, (PT*)h_next, H, score, finished, length, parent,
                                     word, feed, s, N, B, C, blank));
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_attn_beam_trace(const int* parent, const int* word, const float* score, const int* finished, const int* length, int S,
                       int N, int B, int nbest, int blank, int* ids, int* lengths, float* scores, int* count, int* path,
                       hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && S >= 1, "mr_attn_beam_trace: bad shape N=%d S=%d", N, S);
  MR_CHECK_ARG(B >= 1 && B <= MR_ATTN_BEAM_MAX && nbest >= 1 && nbest <= B,
               "mr_attn_beam_trace: beam=%d (1..MR_ATTN_BEAM_MAX=%d), nbest=%d (1..beam)", B, MR_ATTN_BEAM_MAX, nbest);
  MR_CHECK_ARG((long long)N * nbest * ((long long)S + 1) <= INT_MAX, "mr_attn_beam_trace: N=%d nbest=%d S=%d; split the batch", N,
               nbest, S);
  if (N == 0) return MR_OK;
  MR_CHECK_ARG(parent && word && score && finished && length && ids && lengths && scores && count && path,
               "mr_attn_beam_trace: null pointer");
  hipLaunchKernelGGL(attn_beam_trace_kernel, dim3((unsigned)cdivll((long long)N * nbest, 64)), dim3(64), 0, stream, parent, word,
                     score, finished, length, S, N, B, nbest, blank, ids, lengths, scores, count, path);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
