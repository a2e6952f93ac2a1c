// Reading a 2D-CTC head (decoders/ctc_decoder2d.py: eval returns classify [N, C, H, W] and mask [N, 1, H, W]) with the readers of
// a 1-D CTC posterior.  The rules are written out in include/megreader_hip.h (mr_ctc2d_marginal, mr_ctc2d_char_rows); this file is
// two kernels.
//
// mr_ctc2d_marginal: out[n, c, w] = sum_h (or max_h) of classify[n, c, h, w] * mask[n, 0, h, w].  Bandwidth-bound: classify is read
// once, the mask once per workgroup tile.  A workgroup of 256 owns a tile of 32 classes x 32 columns of one sample; a thread owns 4
// cells, and per chunk of 8 heights puts its 32 loads in flight before the mask tile (8 heights x 32 columns, loaded by the same 256
// threads, one value each) arrives in LDS.  Two thread mappings, chosen on the host from the strides:
//   class-fast   lane -> class (the project's own head: an NHWC buffer viewed as NCHW, cc == 1); 32 lanes read 128 contiguous bytes.
//                The results cross a 32 x 33 LDS tile so that the STORES are column-fast like the other mapping's.
//   column-fast  lane -> column (a contiguous NCHW tensor, cw == 1, and any other strides: correct, not necessarily fast).
// Either way the stores run along w: `out` is handed over as [N, C, W] with W contiguous, the layout mr_lexicon_transcribe,
// mr_ctc_beam_search and mr_ctc_align read fastest (a class's columns side by side, as the 1-D eval head's [N, C, 1, T]).
// The arithmetic is fixed -- a rounded product, then a rounded sum / fmaxf in ascending h, nothing fused or reassociated -- so the
// result does not depend on the mapping, the tile or the launch.
//
// mr_ctc2d_char_rows: the most probable height of every column of a forced alignment, and the band of heights of every symbol.
// One wave per row, a lane per column; only the class the alignment gives the column is read (S + 1 classes per row, whatever C is).
#include <limits.h>
#include "device.h"
#include "ctc_posterior.h"
#include "../../include/megreader_hip.h"

// Every product and sum of this file is rounded on its own.  hipcc contracts a * b + c into an fma by default, and HIP's
// __fmul_rn / __fadd_rn do not prevent it: they are inline functions of a header compiled with contraction on, fused after
// inlining (seen in the ISA).  So, as in image_sample.hip, contraction is off for this file and the two are its own.
#pragma clang fp contract(off)

namespace mr {

__device__ __forceinline__ float c2r_mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float c2r_add_rn(float a, float b) { return a + b; }

enum { C2R_TILE = 32, C2R_HC = 8, C2R_ITEMS = 4 };   // tile edge (classes and columns), heights per chunk, cells per thread

template <typename PT, bool CFAST>
__global__ __launch_bounds__(256) void ctc2d_marginal_kernel(const PT* cl, long long cn, long long cc, long long ch, long long cw,
                                                             const PT* mk, long long mn, long long mh, long long mw, int C, int H,
                                                             int W, int tiles_c, int tiles_w, int reduce, int log_out, float* out,
                                                             long long on, long long oc, long long ow) {
  __shared__ float smask[C2R_HC][C2R_TILE];
  __shared__ float stile[C2R_TILE][C2R_TILE + 1];
  const int t = threadIdx.x, a = t & 31, b = t >> 5;
  unsigned blk = blockIdx.x;
  const int tw = (int)(blk % (unsigned)tiles_w);
  blk /= (unsigned)tiles_w;
  const int tc = (int)(blk % (unsigned)tiles_c);
  const int n = (int)(blk / (unsigned)tiles_c);
  const int c0 = tc * C2R_TILE, w0 = tw * C2R_TILE;
  const PT* base = cl + (long long)n * cn;
  // cell i of this thread, within the tile
  int lc[C2R_ITEMS], lw[C2R_ITEMS];
  bool live[C2R_ITEMS];
  const PT* p[C2R_ITEMS];
  float acc[C2R_ITEMS];
#pragma unroll
  for (int i = 0; i < C2R_ITEMS; ++i) {
    lc[i] = CFAST ? a : b + 8 * i;
    lw[i] = CFAST ? b + 8 * i : a;
    live[i] = c0 + lc[i] < C && w0 + lw[i] < W;
    p[i] = base + (long long)(c0 + lc[i]) * cc + (long long)(w0 + lw[i]) * cw;   // (not dereferenced unless live)
    acc[i] = 0.f;
  }
  const int mh_l = t >> 5, mw_l = t & 31;   // the mask value this thread brings per chunk
  const PT* pm = mk + (long long)n * mn + (long long)(w0 + mw_l) * mw;
  for (int h0 = 0; h0 < H; h0 += C2R_HC) {
    const int nh = min((int)C2R_HC, H - h0);
    float v[C2R_ITEMS][C2R_HC];
#pragma unroll
    for (int i = 0; i < C2R_ITEMS; ++i)
#pragma unroll
      for (int u = 0; u < C2R_HC; ++u) v[i][u] = live[i] && u < nh ? to_f32(p[i][(long long)(h0 + u) * ch]) : 0.f;
    smask[mh_l][mw_l] = mh_l < nh && w0 + mw_l < W ? to_f32(pm[(long long)(h0 + mh_l) * mh]) : 0.f;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < C2R_HC; ++u)
      if (u < nh) {
#pragma unroll
        for (int i = 0; i < C2R_ITEMS; ++i) {
          const float prod = c2r_mul_rn(v[i][u], smask[u][lw[i]]);
          acc[i] = h0 + u == 0 ? prod : reduce ? fmaxf(acc[i], prod) : c2r_add_rn(acc[i], prod);
        }
      }
    __syncthreads();
  }
  if (log_out) {
#pragma unroll
    for (int i = 0; i < C2R_ITEMS; ++i) acc[i] = ctc_log_prob(acc[i]);
  }
  float* o = out + (long long)n * on;
  if (CFAST) {
#pragma unroll
    for (int i = 0; i < C2R_ITEMS; ++i) stile[lc[i]][lw[i]] = acc[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < C2R_ITEMS; ++i) {
      const int c = c0 + b + 8 * i, w = w0 + a;
      if (c < C && w < W) o[(long long)c * oc + (long long)w * ow] = stile[b + 8 * i][a];
    }
  } else {
#pragma unroll
    for (int i = 0; i < C2R_ITEMS; ++i)
      if (live[i]) o[(long long)(c0 + lc[i]) * oc + (long long)(w0 + lw[i]) * ow] = acc[i];
  }
}

// One wave per row.  Columns: the class of column w is the one its position names; the arg-max over h of the rounded product, the
// lowest h among equal values.  Then the symbols' bands from the row's own `rows` (written and read back by this workgroup).
template <typename PT>
__global__ __launch_bounds__(64) void ctc2d_char_rows_kernel(const PT* cl, long long cn, long long cc, long long ch, long long cw,
                                                             const PT* mk, long long mn, long long mh, long long mw, int C, int H,
                                                             int W, int blank, const int* targets, int S, const int* target_len,
                                                             const int* pos, const int* begin, const int* end, int* rows,
                                                             int* row_lo, int* row_hi) {
  const int lane = threadIdx.x, n = blockIdx.x;
  const int* tgt = targets + (long long)n * S;
  const int K = min(max(target_len[n], 0), S);
  int* r = rows + (long long)n * W;
  for (int w = lane; w < W; w += 64) {
    const int s = pos[(long long)n * W + w];
    int c = -1;
    if (s >= 0 && s <= 2 * K) c = (s & 1) ? tgt[s >> 1] : blank;   // (odd s <= 2K: s >> 1 < K <= S)
    int best_h = -1;
    if (c >= 0 && c < C) {
      const PT* pc = cl + (long long)n * cn + (long long)c * cc + (long long)w * cw;
      const PT* pm = mk + (long long)n * mn + (long long)w * mw;
      float best = 0.f;
      for (int h0 = 0; h0 < H; h0 += C2R_HC) {
        float v[C2R_HC], m[C2R_HC];
#pragma unroll
        for (int u = 0; u < C2R_HC; ++u) {
          const int h = min(h0 + u, H - 1);   // (past the end: the last height again, dropped below)
          v[u] = to_f32(pc[(long long)h * ch]);
          m[u] = to_f32(pm[(long long)h * mh]);
        }
#pragma unroll
        for (int u = 0; u < C2R_HC; ++u) {
          const float prod = c2r_mul_rn(v[u], m[u]);
          if (h0 + u < H && (h0 + u == 0 || prod > best)) { best = prod; best_h = h0 + u; }
        }
      }
    }
    r[w] = best_h;
  }
  __syncthreads();   // the row's heights are read back below by other lanes
  for (int i = lane; i < S; i += 64) {
    int lo = -1, hi = -1;
    if (i < K) {
      const int b = begin[(long long)n * S + i], e = end[(long long)n * S + i];
      if (b >= 0 && e <= W && b < e) {
        lo = hi = r[b];
        for (int w = b + 1; w < e; ++w) {
          const int h = r[w];
          lo = min(lo, h);
          hi = max(hi, h);
        }
      }
    }
    row_lo[(long long)n * S + i] = lo;
    row_hi[(long long)n * S + i] = hi;
  }
}

// Whether the farthest element of a tensor of these sizes and element strides lies within a 64-bit offset.
static bool c2r_span_fits(const long long* sizes, const long long* strides, int k) {
  long long far = 0;
  for (int i = 0; i < k; ++i) {
    if (sizes[i] <= 1) continue;
    long long step = strides[i] < 0 ? -strides[i] : strides[i], part;
    if (strides[i] == LLONG_MIN || __builtin_mul_overflow(step, sizes[i] - 1, &part) || __builtin_add_overflow(far, part, &far))
      return false;
  }
  return far <= LLONG_MAX / 8;   // (bytes of any element type here)
}

static int c2r_check_inputs(const char* who, long long cn, long long cc, long long ch, long long cw, long long mn, long long mh,
                            long long mw, int N, int C, int H, int W) {
  const long long cs[4] = {N, C, H, W}, cst[4] = {cn, cc, ch, cw}, ms[3] = {N, H, W}, mst[3] = {mn, mh, mw};
  MR_CHECK_ARG(c2r_span_fits(cs, cst, 4) && c2r_span_fits(ms, mst, 3),
               "%s: sizes N=%d C=%d H=%d W=%d times the strides do not fit a 64-bit offset", who, N, C, H, W);
  return MR_OK;
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_ctc2d_marginal(int dtype, const void* classify, long long cn, long long cc, long long ch, long long cw, const void* mask,
                      long long mn, long long mh, long long mw, int N, int C, int H, int W, int reduce, int log_out, float* out,
                      long long on, long long oc, long long ow, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && C >= 0 && H >= 0 && W >= 0, "mr_ctc2d_marginal: bad shape N=%d C=%d H=%d W=%d", N, C, H, W);
  MR_CHECK_ARG(reduce == 0 || reduce == 1, "mr_ctc2d_marginal: reduce=%d (0 = sum, 1 = max)", reduce);
  MR_CHECK_ARG(log_out == 0 || log_out == 1, "mr_ctc2d_marginal: log_out=%d (0 or 1)", log_out);
  MR_CTC_TRY(ctc_check_dtype("mr_ctc2d_marginal", dtype));
  if (N == 0 || C == 0 || W == 0) return MR_OK;   // `out` has no element
  MR_CTC_TRY(c2r_check_inputs("mr_ctc2d_marginal", cn, cc, ch, cw, mn, mh, mw, N, C, H, W));
  const long long os[3] = {N, C, W}, ost[3] = {on, oc, ow};
  MR_CHECK_ARG(c2r_span_fits(os, ost, 3), "mr_ctc2d_marginal: the strides of out do not fit a 64-bit offset");
  MR_CHECK_ARG(out && (H == 0 || (classify && mask)), "mr_ctc2d_marginal: null pointer");
  const int tiles_c = cdiv(C, C2R_TILE), tiles_w = cdiv(W, C2R_TILE);
  const long long blocks = (long long)N * tiles_c * tiles_w;
  MR_CHECK_ARG(blocks <= INT_MAX, "mr_ctc2d_marginal: N=%d C=%d W=%d make %lld workgroups; split the batch", N, C, W, blocks);
  // the fast axis of classify: the class (the head's NHWC buffer) or, for everything else, the column
  const bool cfast = cc == 1 && cw != 1;
  MR_CTC_DISPATCH(dtype, PT, {
    if (cfast)
      hipLaunchKernelGGL((ctc2d_marginal_kernel<PT, true>), dim3((unsigned)blocks), dim3(256), 0, stream, (const PT*)classify, cn,
                         cc, ch, cw, (const PT*)mask, mn, mh, mw, C, H, W, tiles_c, tiles_w, reduce, log_out, out, on, oc, ow);
    else
      hipLaunchKernelGGL((ctc2d_marginal_kernel<PT, false>), dim3((unsigned)blocks), dim3(256), 0, stream, (const PT*)classify, cn,
                         cc, ch, cw, (const PT*)mask, mn, mh, mw, C, H, W, tiles_c, tiles_w, reduce, log_out, out, on, oc, ow);
  });
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_ctc2d_char_rows(int dtype, const void* classify, long long cn, long long cc, long long ch, long long cw, const void* mask,
                       long long mn, long long mh, long long mw, int N, int C, int H, int W, int blank, const int* targets, int S,
                       const int* target_len, const int* pos, const int* begin, const int* end, int* rows, int* row_lo,
                       int* row_hi, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0, "mr_ctc2d_char_rows: N=%d rows", N);
  MR_CHECK_ARG(C >= 1 && H >= 1 && W >= 1, "mr_ctc2d_char_rows: bad shape C=%d H=%d W=%d", C, H, W);
  MR_CHECK_ARG(S >= 0 && S <= MR_CTC_ALIGN_MAX_SYMBOLS, "mr_ctc2d_char_rows: S=%d symbols per row (0..MR_CTC_ALIGN_MAX_SYMBOLS=%d)",
               S, MR_CTC_ALIGN_MAX_SYMBOLS);
  MR_CHECK_ARG(blank >= 0 && blank < C, "mr_ctc2d_char_rows: blank=%d is not a class of C=%d", blank, C);
  MR_CTC_TRY(ctc_check_dtype("mr_ctc2d_char_rows", dtype));
  if (N == 0) return MR_OK;
  MR_CTC_TRY(c2r_check_inputs("mr_ctc2d_char_rows", cn, cc, ch, cw, mn, mh, mw, N, C, H, W));
  MR_CHECK_ARG(classify && mask && target_len && pos && rows && (S == 0 || (targets && begin && end && row_lo && row_hi)),
               "mr_ctc2d_char_rows: null pointer");
  MR_CTC_DISPATCH(dtype, PT,
                  hipLaunchKernelGGL(ctc2d_char_rows_kernel<PT>, dim3((unsigned)N), dim3(64), 0, stream, (const PT*)classify, cn,
                                     cc, ch, cw, (const PT*)mask, mn, mh, mw, C, H, W, blank, targets, S, target_len, pos, begin,
                                     end, rows, row_lo, row_hi));
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
