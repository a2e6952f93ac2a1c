// Replay read of the attention decoder (decoders/attention_decoder.py: AttentionDecoder.read): what the greedy loop, or a beam
// hypothesis, leaves behind is its words and its hidden states H_all [S+1][N][H].  Given those, the attention map and the output
// distribution of step s depend on H_all[s] and H_all[s + 1] alone -- not on any other step -- so the scores and the maps of all
// S steps are ONE parallel pass behind the loop and the persistent decode kernel stays as it is.  The rules are written out in
// include/megreader_hip.h (mr_attn_read); this file is two kernels.
//
// attn_read_kernel: a workgroup of 256 owns one image n and SG consecutive steps.  The kernel is bound by its S*N*T*H tanh
// evaluations and by the eproj traffic, so eproj[n] is read ONCE per workgroup: the SG rows of hproj (as f32) and v sit in LDS, a
// wave takes a position t, its lanes 16-byte slices of eproj[n][t], and every slice loaded serves the SG steps.  SG is the
// largest of 8, 4, 2, 1 whose hproj rows and energies [SG][T] fit the LDS budget (T = 4096, H = 512: 2).  Then, a wave per step,
// the softmax over the T energies, the moments of the map in two passes (mean, then the deviations from it: a sum of squares
// minus a squared mean cancels to 1e-4 of a cell in f32) and the log-softmax of the step's logits at the emitted word.
// tanh is att_tanh (common.h: exp2 / rcp), as everywhere in the attention kernels.
//
// attn_read_score_kernel: a thread per row; the length (first blank) and the sum of sym_lp in ascending s.
#include <limits.h>
#include "ctc_posterior.h"
#include "../../include/megreader_hip.h"

namespace mr {

enum { AR_THREADS = 256, AR_WAVES = AR_THREADS / 64, AR_LDS_BUDGET = 64 * 1024 };

template <typename T> struct ArVec;
template <> struct ArVec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float* f) {
    const f32x4 v = *(const f32x4*)p;
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
  }
};
template <> struct ArVec<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float* f) {
    const bf16x8 v = *(const bf16x8*)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
  }
};

// floats of dynamic LDS: v [Hp] | hproj rows [SG][Hp] | energies [SG][T]   (Hp = H rounded up to 4: 16-byte rows)
static inline long long ar_lds_floats(int sg, int H, int T) {
  const long long Hp = ((long long)H + 3) / 4 * 4;
  return Hp + (long long)sg * Hp + (long long)sg * T;
}

template <typename T, int SG, bool VECTOR>
__global__ __launch_bounds__(AR_THREADS) void attn_read_kernel(const T* __restrict__ hproj, long long ldh,
                                                               const T* __restrict__ eproj, const float* __restrict__ v,
                                                               const T* __restrict__ logits, long long ldl,
                                                               const int* __restrict__ words, long long ldp, int N, int S,
                                                               int Tn, int H, int C, int width, int chunks,
                                                               float* __restrict__ att, float* __restrict__ sym_lp,
                                                               float* __restrict__ moments) {
  constexpr int VEC = ArVec<T>::N;
  extern __shared__ __attribute__((aligned(16))) float ar_lds[];
  const int Hp = (H + 3) / 4 * 4;
  float* vs = ar_lds;
  float* hp = vs + Hp;
  float* en = hp + SG * Hp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = (int)(blockIdx.x / (unsigned)chunks);
  const int s0 = (int)(blockIdx.x % (unsigned)chunks) * SG;
  const int sg = min(SG, S - s0);                     // steps of this workgroup that exist

  for (int j = tid; j < Hp; j += AR_THREADS) vs[j] = j < H ? v[j] : 0.f;
  for (int i = 0; i < SG; ++i) {
    const T* row = hproj + ((long long)(s0 + min(i, sg - 1)) * N + n) * ldh;     // (a step past S: the last one again, dropped)
    for (int j = tid; j < Hp; j += AR_THREADS) hp[i * Hp + j] = j < H ? to_f32(row[j]) : 0.f;
  }
  __syncthreads();

  // energies: en[i][t] = sum_h v[h] * tanh(hproj[s0 + i][n][h] + eproj[n][t][h]), per lane in ascending h, then the wave's tree
  const T* ebase = eproj + (long long)n * Tn * H;
  for (int t = wave; t < Tn; t += AR_WAVES) {
    const T* ep = ebase + (long long)t * H;
    float acc[SG];
#pragma unroll
    for (int i = 0; i < SG; ++i) acc[i] = 0.f;
    if (VECTOR) {
      for (int j = lane * VEC; j < H; j += 64 * VEC) {
        float e[VEC];
        ArVec<T>::load(ep + j, e);
#pragma unroll
        for (int q = 0; q < VEC; q += 4) {
          const f32x4 vv = *(const f32x4*)(vs + j + q);
#pragma unroll
          for (int i = 0; i < SG; ++i) {
            const f32x4 a = *(const f32x4*)(hp + i * Hp + j + q);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[i] += vv[u] * att_tanh(a[u] + e[q + u]);
          }
        }
      }
    } else {
      for (int j = lane; j < H; j += 64) {
        const float e = to_f32(ep[j]), vv = vs[j];
#pragma unroll
        for (int i = 0; i < SG; ++i) acc[i] += vv * att_tanh(hp[i * Hp + j] + e);
      }
    }
#pragma unroll
    for (int i = 0; i < SG; ++i) {
      const float s = wave_sum(acc[i]);
      if (lane == 0) en[i * Tn + t] = s;
    }
  }
  __syncthreads();

  // a wave per step: softmax over t, the map's moments, the word's log-probability
  for (int i = wave; i < sg; i += AR_WAVES) {
    const int s = s0 + i;
    float* e = en + i * Tn;
    float mx = -INFINITY;
    for (int t = lane; t < Tn; t += 64) mx = fmaxf(mx, e[t]);
    mx = wave_max(mx);
    float sm = 0.f;
    for (int t = lane; t < Tn; t += 64) {
      const float ex = expf(e[t] - mx);
      e[t] = ex;                                       // (a lane reads back only what it wrote)
      sm += ex;
    }
    sm = wave_sum(sm);
    float* arow = att ? att + ((long long)n * S + s) * Tn : nullptr;
    float cx = 0.f, cy = 0.f;
    for (int t = lane; t < Tn; t += 64) {
      const float a = e[t] / sm;
      e[t] = a;
      if (arow) arow[t] = a;
      cx += a * ((float)(t % width) + 0.5f);
      cy += a * ((float)(t / width) + 0.5f);
    }
    cx = wave_sum(cx);
    cy = wave_sum(cy);
    float vx = 0.f, vy = 0.f;
    for (int t = lane; t < Tn; t += 64) {
      const float a = e[t];
      const float dx = ((float)(t % width) + 0.5f) - cx, dy = ((float)(t / width) + 0.5f) - cy;
      vx += a * (dx * dx);
      vy += a * (dy * dy);
    }
    vx = wave_sum(vx);
    vy = wave_sum(vy);
    // log_softmax(logits[s][n])[word]: the maximum, then the sum of exp in ascending c per lane and the wave's tree
    const T* lrow = logits + ((long long)s * N + n) * ldl;
    const int word = words[(long long)n * ldp + s];
    float lm = -INFINITY;
    for (int c = lane; c < C; c += 64) lm = fmaxf(lm, to_f32(lrow[c]));
    lm = wave_max(lm);
    float ls = 0.f;
    for (int c = lane; c < C; c += 64) ls += expf(to_f32(lrow[c]) - lm);
    ls = wave_sum(ls);
    if (lane == 0) {
      float* m = moments + ((long long)n * S + s) * 4;
      m[0] = cx;
      m[1] = cy;
      m[2] = sqrtf(vx);
      m[3] = sqrtf(vy);
      // a word that is no class (-1: the decode kernel's mark of a timed-out row) has no probability
      sym_lp[(long long)n * S + s] = (word >= 0 && word < C) ? (to_f32(lrow[word]) - lm) - logf(ls) : -INFINITY;
    }
  }
}

__global__ __launch_bounds__(64) void attn_read_score_kernel(const int* __restrict__ words, long long ldp,
                                                             const float* __restrict__ sym_lp, int N, int S, int blank,
                                                             int* __restrict__ length, float* __restrict__ score) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const int* w = words + (long long)n * ldp;
  int len = S;
  for (int s = 0; s < S; ++s)
    if (w[s] == blank) { len = s; break; }
  const int last = min(len, S - 1);                    // the terminating blank belongs to the string's probability
  const float* lp = sym_lp + (long long)n * S;
  float sum = lp[0];
  for (int s = 1; s <= last; ++s) sum += lp[s];
  length[n] = len;
  score[n] = sum;
}

template <typename T, bool VECTOR>
static void ar_launch(int sg, unsigned blocks, size_t lds, hipStream_t stream, const T* hproj, long long ldh, const T* eproj,
                      const float* v, const T* logits, long long ldl, const int* words, long long ldp, int N, int S, int Tn, int H,
                      int C, int width, int chunks, float* att, float* sym_lp, float* moments) {
#define AR_CASE(SG_)                                                                                                          \
  case SG_:                                                                                                                   \
    hipLaunchKernelGGL((attn_read_kernel<T, SG_, VECTOR>), dim3(blocks), dim3(AR_THREADS), lds, stream, hproj, ldh, eproj, v, \
                       logits, ldl, words, ldp, N, S, Tn, H, C, width, chunks, att, sym_lp, moments);                         \
    break;
  switch (sg) {
    AR_CASE(8)
    AR_CASE(4)
    AR_CASE(2)
    default:
    AR_CASE(1)
  }
#undef AR_CASE
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_attn_read(int dtype, const void* hproj, long long ldh, const void* eproj, const float* v, const void* logits,
                 long long ldl, const int* words, long long ldp, int blank, int N, int S, int T, int H, int C, int height,
                 int width, float* att, float* sym_lp, float* moments, int* length, float* score, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && S >= 1 && H >= 1 && C >= 1, "mr_attn_read: bad shape N=%d S=%d H=%d C=%d", N, S, H, C);
  MR_CHECK_ARG(T >= 1 && T <= MR_ATTN_READ_MAX_T, "mr_attn_read: T=%d positions (1..MR_ATTN_READ_MAX_T=%d)", T,
               MR_ATTN_READ_MAX_T);
  MR_CHECK_ARG(height >= 1 && width >= 1 && (long long)height * width == T, "mr_attn_read: the grid %d x %d is not T=%d positions",
               height, width, T);
  MR_CHECK_ARG(blank >= 0 && blank < C, "mr_attn_read: blank=%d is not a class of C=%d", blank, C);
  MR_CHECK_ARG(ldh >= H && ldl >= C && ldp >= S, "mr_attn_read: leading dimensions ldh=%lld ldl=%lld ldp=%lld below H=%d C=%d S=%d",
               ldh, ldl, ldp, H, C, S);
  MR_CTC_TRY(ctc_check_dtype("mr_attn_read", dtype));
  MR_CHECK_ARG(ar_lds_floats(1, H, T) * 4 <= AR_LDS_BUDGET, "mr_attn_read: H=%d with T=%d does not fit the %d bytes of LDS of a step",
               H, T, (int)AR_LDS_BUDGET);
  if (N == 0) return MR_OK;
  MR_CHECK_ARG(hproj && eproj && v && logits && words && sym_lp && moments && length && score, "mr_attn_read: null pointer");
  int sg = 8;
  while (sg > 1 && (ar_lds_floats(sg, H, T) * 4 > AR_LDS_BUDGET || sg / 2 >= S)) sg /= 2;
  const int chunks = cdiv(S, sg);
  const long long blocks = (long long)N * chunks;
  MR_CHECK_ARG(blocks <= INT_MAX, "mr_attn_read: N=%d S=%d make %lld workgroups; split the batch", N, S, blocks);
  const size_t lds = (size_t)ar_lds_floats(sg, H, T) * 4;
  const int vec = dtype == MR_DTYPE_F32 ? 4 : 8;
  const bool vector = H % vec == 0 && ((uintptr_t)eproj & 15) == 0;
  MR_CTC_DISPATCH(dtype, PT, {
    if (vector)
      ar_launch<PT, true>(sg, (unsigned)blocks, lds, stream, (const PT*)hproj, ldh, (const PT*)eproj, v, (const PT*)logits, ldl,
                          words, ldp, N, S, T, H, C, width, chunks, att, sym_lp, moments);
    else
      ar_launch<PT, false>(sg, (unsigned)blocks, lds, stream, (const PT*)hproj, ldh, (const PT*)eproj, v, (const PT*)logits, ldl,
                           words, ldp, N, S, T, H, C, width, chunks, att, sym_lp, moments);
  });
  MR_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_read_score_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, stream, words, ldp, sym_lp, N, S, blank,
                     length, score);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
