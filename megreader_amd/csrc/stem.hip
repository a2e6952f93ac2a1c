// Fused first stage of the CRNN backbone: Conv2d(Cin -> 64, 3x3, stride 1, pad 1) + bias + ReLU + MaxPool2d(2, 2).
// (reference backbones/crnn.py:17-19 + 48-55: cnn.conv0 / relu0 / pooling0 on the 3-channel 32x128 crop.)
//
// Why a dedicated kernel: with Cin = 3 the layer is pure HBM traffic.  As separate ops it writes the 64-channel
// full-resolution activation (134 MB at batch 256), reads it back to pool, and in backward writes / re-reads the
// equally large sparse gradient.  Fused, the forward reads the fp32 NCHW image (12.6 MB) and writes only the pooled
// activation (33.5 MB) plus a one-byte code per pooled element; the backward reads the pooled gradient, the codes
// and the image, and produces dW / db directly -- the full-resolution tensors never exist.
//
// Mapping, generic kernels (f32, and bf16 at widths the MFMA kernels do not take): one wavefront lane = one output
// channel (Cout == 64 == wavefront width), so each lane keeps its 9*Cin filter taps (forward) or 9*Cin + 1 gradient
// accumulators (backward) in registers for the whole kernel.  A workgroup owns one pooled output row ("strip") at a
// time: the 4 input rows it needs are staged in LDS, already rounded to the compute dtype, and the 4x4xCin patch of
// each pooled pixel is read from LDS with wave-uniform addresses (hardware broadcast, no bank conflicts).  Arithmetic
// is f32 FMA on compute-dtype-rounded operands: the same products the MFMA path forms, summed in a different order.
//
// Mapping, bf16 MFMA kernels (W/2 a multiple of 16; second half of this file): a workgroup owns a RUN of up to
// STEM_RUN consecutive strips of one image.  Every input row of the run is fetched once, with 16-byte loads, into an
// LDS row of its own; the two rows the next strip adds are requested before the current strip is computed and written
// to LDS after it, so there is one LDS-only barrier per strip and the memory latency lies behind the MFMA and arg-max
// work.  Filter fragments, bias and gather offsets are set up once per workgroup.  The backward reads a pixel's
// gradients and codes with 8- and 4-byte loads that need no lane exchange, sums whole runs per workgroup (at most
// STEM_BWD_GROUPS_MFMA partial sets, half of them at the CRNN's batch) and leaves the final sum to the small reduce
// launch; there is no ticket, so the workspace needs no initialisation.
//
// Code byte per pooled element: bits 0-1 = position of the first maximum in the 2x2 window (row-major, the order
// nn.MaxPool2d scans), bit 2 = the maximum is > 0 (ReLU passes gradient).
#include <type_traits>

#include "common.h"
#include "../../include/megreader_hip.h"

namespace mr {

constexpr int STEM_COUT = 64;
constexpr int STEM_BWD_GROUPS = 1024;  // workgroups (= partial sums) of the generic backward main kernel, at most
constexpr int STEM_BWD_GROUPS_MFMA = 512;  // ... of the MFMA one (each sums whole runs of strips)
constexpr int STEM_RUN = 8;                      // MFMA kernels: pooled rows per workgroup run (half a 32-row image)
constexpr int STEM_PADL = 4;                     // MFMA kernels: LDS columns left of image column 0
constexpr int STEM_LDS_ROWS_BYTES = 48 * 1024;   // MFMA kernels: most LDS the rows of one run may take

template <typename T> __device__ __forceinline__ float round_as(float v) { return to_f32(from_f32<T>(v)); }

// patch[r][col + 1][c], r = 0..3 <-> input rows 2*ph - 1 + r, col = -1..W (zero outside the image)
template <typename T, int CIN>
__device__ __forceinline__ void stem_stage_patch(float* patch, const float* __restrict__ x, int n, int ph, int H,
                                                 int W) {
  const int PW = W + 2;
  for (int r = 0; r < 4; ++r) {
    const int row = 2 * ph - 1 + r;
    const bool rv = row >= 0 && row < H;
    for (int j = threadIdx.x; j < CIN * W; j += blockDim.x) {
      const int c = j / W, col = j - c * W;
      const float v = rv ? x[((long long)(n * CIN + c) * H + row) * W + col] : 0.f;
      patch[(r * PW + col + 1) * CIN + c] = round_as<T>(v);
    }
  }
  if (threadIdx.x < 4 * 2 * CIN) {
    const int r = threadIdx.x / (2 * CIN), rem = threadIdx.x - r * 2 * CIN;
    const int side = rem / CIN, c = rem - side * CIN;
    patch[(r * PW + (side ? W + 1 : 0)) * CIN + c] = 0.f;
  }
}

template <typename T, int CIN>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       long long wsk, long long wsc, long long wsr, long long wss,
                                                       const float* __restrict__ bias, T* __restrict__ y,
                                                       unsigned char* __restrict__ code, int N, int H, int W) {
  extern __shared__ float patch[];
  constexpr int KT = 9 * CIN;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const int Ho = H / 2, Wo = W / 2, PW = W + 2;
  float wr[KT];  // [dr][ds][c]
#pragma unroll
  for (int dr = 0; dr < 3; ++dr)
#pragma unroll
    for (int ds = 0; ds < 3; ++ds)
#pragma unroll
      for (int c = 0; c < CIN; ++c)
        wr[(dr * 3 + ds) * CIN + c] = round_as<T>(w[lane * wsk + c * wsc + dr * wsr + ds * wss]);
  const float b = bias ? bias[lane] : 0.f;
  const int per = (Wo + nwv - 1) / nwv;
  for (int strip = blockIdx.x; strip < N * Ho; strip += gridDim.x) {
    const int n = strip / Ho, ph = strip - n * Ho;
    __syncthreads();
    stem_stage_patch<T, CIN>(patch, x, n, ph, H, W);
    __syncthreads();
    const int pw1 = min(Wo, (wv + 1) * per);
    for (int pw = wv * per; pw < pw1; ++pw) {
      float P[4][4 * CIN];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4 * CIN; ++i) P[r][i] = patch[(r * PW + 2 * pw) * CIN + i];
      float best = 0.f;
      int q = 0;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int a = qq >> 1, bq = qq & 1;
        float acc = b;
#pragma unroll
        for (int dr = 0; dr < 3; ++dr)
#pragma unroll
          for (int i = 0; i < 3 * CIN; ++i) acc = fmaf(wr[dr * 3 * CIN + i], P[a + dr][bq * CIN + i], acc);
        if (qq == 0 || acc > best) {  // strict > keeps the first maximum
          best = acc;
          q = qq;
        }
      }
      const bool pos = best > 0.f;
      const long long o = ((long long)strip * Wo + pw) * STEM_COUT + lane;
      y[o] = from_f32<T>(pos ? best : 0.f);
      if (code) code[o] = (unsigned char)(q | (pos ? 4 : 0));
    }
  }
}

// partial[g][k][o], k = 0..9*CIN-1 filter taps ([dr][ds][c]) and k = 9*CIN the bias gradient
template <typename T, int CIN>
__global__ __launch_bounds__(256) void stem_bwd_kernel(const T* __restrict__ dy, const unsigned char* __restrict__ code,
                                                       const float* __restrict__ x, float* __restrict__ partial, int N,
                                                       int H, int W) {
  extern __shared__ float patch[];
  constexpr int KT = 9 * CIN;
  __shared__ float red[4][KT + 1][STEM_COUT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const int Ho = H / 2, Wo = W / 2, PW = W + 2;
  float acc[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = 0.f;
  float accb = 0.f;
  const int per = (Wo + nwv - 1) / nwv;
  for (int strip = blockIdx.x; strip < N * Ho; strip += gridDim.x) {
    const int n = strip / Ho, ph = strip - n * Ho;
    __syncthreads();
    stem_stage_patch<T, CIN>(patch, x, n, ph, H, W);
    __syncthreads();
    const int pw1 = min(Wo, (wv + 1) * per);
    for (int pw = wv * per; pw < pw1; ++pw) {
      const long long o = ((long long)strip * Wo + pw) * STEM_COUT + lane;
      const int cd = code[o];
      const float g = (cd & 4) ? to_f32(dy[o]) : 0.f;
      const int q = cd & 3;
      float P[4][4 * CIN];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4 * CIN; ++i) P[r][i] = patch[(r * PW + 2 * pw) * CIN + i];
      accb += g;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int a = qq >> 1, bq = qq & 1;
        const float gq = (q == qq) ? g : 0.f;
#pragma unroll
        for (int dr = 0; dr < 3; ++dr)
#pragma unroll
          for (int i = 0; i < 3 * CIN; ++i)
            acc[dr * 3 * CIN + i] = fmaf(gq, P[a + dr][bq * CIN + i], acc[dr * 3 * CIN + i]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KT; ++k) red[wv][k][lane] = acc[k];
  red[wv][KT][lane] = accb;
  __syncthreads();
  for (int i = threadIdx.x; i < (KT + 1) * STEM_COUT; i += blockDim.x) {
    const int k = i / STEM_COUT, o = i - k * STEM_COUT;
    float s = 0.f;
    for (int v = 0; v < nwv; ++v) s += red[v][k][o];
    partial[(long long)blockIdx.x * (KT + 1) * STEM_COUT + i] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// bf16 MFMA variants (Wo % 16 == 0).  The 3x3xCin filter is a K = 9*Cin <= 27 (padded to 32) reduction: exactly one
// v_mfma_f32_16x16x32_bf16 per 16 pixels x 16 channels.  Operand fragments are gathered from the bf16 LDS patch:
// k = (dr*3 + ds)*Cin + c lives at patch offset dr*ROW + (ds*Cin + c) from the pixel's top-left element.
//
// A workgroup owns a RUN of consecutive pooled rows (strips) of one image.  All 2*run + 2 input rows of the run have
// their own LDS row, so every input row is fetched from memory once per run and no LDS row is ever rewritten: the only
// hazard is read-after-write, one LDS-only barrier per strip.  The two new rows of strip s + 1 (a "row pair") are
// requested from memory before strip s is computed and written to LDS after it, so their latency overlaps the MFMA
// and arg-max work.  LDS row = [STEM_PADL columns | W columns | 4 columns][Cin] bf16: column -1 and column W are
// zero, and every group of 4 columns starts 8-byte aligned.
// ------------------------------------------------------------------------------------------------------------------
template <int CIN, int NIT> struct StemRowPair {   // 256 threads x NIT groups of 4 columns cover both rows: NIT >= W / 512
  f32x4 v[NIT][CIN];
};

// Request row pair: image rows row0, row0 + 1 (clamped into the image; rows outside it are zeroed by the store).
// Thread task j = (row of the pair, group of 4 columns): one 16-byte load per channel (4 dword loads when x is not
// 16-byte aligned).  Threads past the last task repeat it, here and in the store (same value to the same address),
// so that neither has a branch: every wave waits for its loads where it stores them, after the strip's arithmetic.
template <int CIN, int NIT, bool A16>
__device__ __forceinline__ void stem_rows_load(StemRowPair<CIN, NIT>& p, const float* __restrict__ x, int n, int H,
                                               int W, int row0) {
  const int W4 = W >> 2, nt = 2 * W4;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int j = min((int)threadIdx.x + it * 256, nt - 1);
    const int rr = j >= W4 ? 1 : 0, g = j - rr * W4;
    const int row = min(max(row0 + rr, 0), H - 1);
    const float* src = x + ((long long)n * CIN * H + row) * W + 4 * g;
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
      const float* s = src + (long long)c * H * W;
      if (A16) p.v[it][c] = *(const f32x4*)s;
      else p.v[it][c] = f32x4{s[0], s[1], s[2], s[3]};
    }
  }
}

// Round the requested pair to bf16 and write it to LDS rows lrow0, lrow0 + 1 (8-byte writes, channels interleaved).
template <int CIN, int NIT>
__device__ __forceinline__ void stem_rows_store(bf16_t* patch, const StemRowPair<CIN, NIT>& p, int H, int W, int row0,
                                                int lrow0) {
  const int W4 = W >> 2, nt = 2 * W4, PW = W + 8;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int j = min((int)threadIdx.x + it * 256, nt - 1);
    const int rr = j >= W4 ? 1 : 0, g = j - rr * W4;
    const bool rv = row0 + rr >= 0 && row0 + rr < H;
    bf16x4 o[CIN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
        const int e = i * CIN + c;
        o[e >> 2][e & 3] = (bf16_t)(rv ? p.v[it][c][i] : 0.f);
      }
    bf16x4* dst = (bf16x4*)(patch + ((lrow0 + rr) * PW + STEM_PADL + 4 * g) * CIN);
#pragma unroll
    for (int c = 0; c < CIN; ++c) dst[c] = o[c];
  }
}

// Columns -1 and W of the first `rows` LDS rows.
template <int CIN>
__device__ __forceinline__ void stem_zero_pads(bf16_t* patch, int rows, int W) {
  const int PW = W + 8;
  for (int j = threadIdx.x; j < rows * 2 * CIN; j += blockDim.x) {
    const int r = j / (2 * CIN), rem = j - r * 2 * CIN;
    const int side = rem / CIN, c = rem - side * CIN;
    patch[(r * PW + (side ? STEM_PADL + W : STEM_PADL - 1)) * CIN + c] = (bf16_t)0.f;
  }
}

// Filter bank packed for the MFMA forward: bf16 [64 channels][32 k], k = (dr*3 + ds)*Cin + c, zero for k >= 9*Cin.
// Produced once per optimizer step (MR_PREP_STEM job of mr_prep_batch, or mr_stem_pack).
template <int CIN>
__global__ void stem_pack_kernel(const float* __restrict__ w, long long wsk, long long wsc, long long wsr,
                                 long long wss, bf16_t* __restrict__ wpack) {
  constexpr int KT = 9 * CIN;
  for (int i = threadIdx.x; i < STEM_COUT * 32; i += blockDim.x) {
    const int ch = i >> 5, k = i & 31;
    const int dr = k / (3 * CIN), rem = k - dr * 3 * CIN, ds = rem / CIN, c = rem - ds * CIN;
    wpack[i] = (bf16_t)(k < KT ? w[ch * wsk + c * wsc + dr * wsr + ds * wss] : 0.f);
  }
}

// Forward.  Workgroup blockIdx.x = (image n, run of `run` strips); filter fragments, bias and gather offsets are set
// up once per workgroup.  Per strip a wave takes 16 pooled pixels: 4 window positions x 4 channel tiles = 16 MFMAs.
// MFMA row r of channel tile ct is channel (r>>2)*16 + ct*4 + (r&3), so that a lane (pixel l15, row group lg) ends up
// with the 16 CONSECUTIVE channels lg*16 .. lg*16+15 of its pixel for all four window positions: max / arg-max / ReLU
// happen in registers and the lane writes 32 contiguous bytes of y and 16 of codes (none when code is null).
// The kernel is VALU-bound (arg-max bookkeeping), so everything else is kept off the vector ALU: the filter bank
// arrives pre-packed (4 fragment loads per lane), staging is division-free.
template <int CIN, int NIT, bool A16, int WFIX>
__global__ __launch_bounds__(256, 2) void stem_fwd_mfma_kernel(const float* __restrict__ x,
                                                            const bf16_t* __restrict__ wpack,
                                                            const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                            unsigned char* __restrict__ code, int H, int Wd, int run) {
  extern __shared__ float patch_raw[];
  bf16_t* patch = (bf16_t*)patch_raw;
  constexpr int KT = 9 * CIN;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
  const int W = WFIX ? WFIX : Wd;
  const int Ho = H / 2, Wo = W / 2, PW = W + 8, ROW = PW * CIN;
  const int upi = (Ho + run - 1) / run;  // runs per image
  const int n = blockIdx.x / upi, ph0 = (blockIdx.x - n * upi) * run;
  const int ns = min(run, Ho - ph0);
  bf16x8 wf[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int ch = (l15 >> 2) * 16 + ct * 4 + (l15 & 3);
    wf[ct] = *(const bf16x8*)(wpack + ch * 32 + 8 * lg);
  }
  f32x4 bv[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
    bv[ct] = bias ? *(const f32x4*)(bias + lg * 16 + ct * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  int koff[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = 8 * lg + i;
    const int dr = k / (3 * CIN), rem = k - dr * 3 * CIN;
    koff[i] = k < KT ? dr * ROW + rem : 0;
  }
  // rows 2*ph0 - 1 .. 2*ph0 + 2 of the first strip: both pairs in flight together (requested after the filter and bias
  // loads: memory returns in order, so those have arrived once the rows have)
  StemRowPair<CIN, NIT> pa, pb;
  stem_rows_load<CIN, NIT, A16>(pa, x, n, H, W, 2 * ph0 - 1);
  stem_rows_load<CIN, NIT, A16>(pb, x, n, H, W, 2 * ph0 + 1);
  stem_zero_pads<CIN>(patch, 2 * ns + 2, W);
  stem_rows_store<CIN, NIT>(patch, pa, H, W, 2 * ph0 - 1, 0);
  stem_rows_store<CIN, NIT>(patch, pb, H, W, 2 * ph0 + 1, 2);
  lds_barrier();

  auto do_pass = [&](int s, int pw0) {
    {
      const long long strip = (long long)n * Ho + ph0 + s;
      const int pw = pw0 + l15;
      bf16x8 xf[4];
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int base = ((2 * s + (qq >> 1)) * PW + STEM_PADL - 1 + 2 * pw + (qq & 1)) * CIN;
#pragma unroll
        for (int i = 0; i < 8; ++i) xf[qq][i] = patch[base + koff[i]];
      }
      uint2 yo[4];     // 4 channels of bf16 each
      unsigned co[4];  // 4 code bytes each
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        bf16x4 yv;
        unsigned cw = 0;
        f32x4 acc[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          acc[qq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ct], xf[qq], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // first maximum of the window, in scan order
          // (compare + select instead of fmaxf: no NaN canonicalisation, and the compares are needed anyway)
          const float a0 = acc[0][r], a1 = acc[1][r], a2 = acc[2][r], a3 = acc[3][r];
          const bool c1 = a1 > a0, c2 = a3 > a2;
          const float m01 = c1 ? a1 : a0, m23 = c2 ? a3 : a2;
          const bool c3 = m23 > m01;
          const int q = c3 ? (c2 ? 3 : 2) : (c1 ? 1 : 0);
          const float best = (c3 ? m23 : m01) + bv[ct][r];
          const bool pos = best > 0.f;
          yv[r] = (bf16_t)(pos ? best : 0.f);
          cw |= (unsigned)(pos ? (q | 4) : q) << (8 * r);
        }
        // The tile's results are made here, in vector registers: left to itself the compiler keeps the 48 compare masks of
        // a pass alive until the stores, which is more than the scalar registers hold.
        yo[ct] = __builtin_bit_cast(uint2, yv);
        co[ct] = cw;
        asm volatile("" : "+v"(yo[ct].x), "+v"(yo[ct].y), "+v"(co[ct]));
      }
      const long long o = (strip * Wo + pw) * STEM_COUT + lg * 16;
      *(uint4*)(y + o) = uint4{yo[0].x, yo[0].y, yo[1].x, yo[1].y};
      *(uint4*)(y + o + 8) = uint4{yo[2].x, yo[2].y, yo[3].x, yo[3].y};
      if (code) *(uint4*)(code + o) = uint4{co[0], co[1], co[2], co[3]};
    }
  };
  // One strip; `more`: another follows.  A compile-time flag and, with WFIX, one pass per wave: the compiler can then
  // count the result stores issued behind the row loads and wait for the loads alone.
  auto do_strip = [&](int s, auto more_c) {
    constexpr bool more = decltype(more_c)::value;
    const int nrow0 = 2 * (ph0 + s) + 3;  // first image row of the pair that strip s + 1 adds
    if (more) {
      stem_rows_load<CIN, NIT, A16>(pa, x, n, H, W, nrow0);
      __builtin_amdgcn_sched_barrier(0);  // the requests go out before the strip's arithmetic, not in the middle of it
    }
    if (WFIX == 128) do_pass(s, wv * 16);
    else
      for (int pw0 = wv * 16; pw0 < Wo; pw0 += 64) do_pass(s, pw0);
    if (more) {
      stem_rows_store<CIN, NIT>(patch, pa, H, W, nrow0, 2 * s + 4);
      lds_barrier();
    }
  };
  int s = 0;
  for (; s + 1 < ns; ++s) do_strip(s, std::true_type{});
  do_strip(s, std::false_type{});
}

// Backward.  dW[ch][k] = sum over (pooled pixel, window position) of G[ch] * X[k]: per 8 pooled pixels one
// 32-deep reduction step (8 pixels x 4 positions).  Lane group lg owns pixels 2*lg, 2*lg+1 and all 4 positions.
// MFMA row l15 of channel tile mt is channel 4*l15 + mt, so the 4 gradient values a lane needs of one pixel are 8
// contiguous bytes of dy and 4 of codes: one load each, and the 16 lanes of a group read a pixel's whole 128-byte
// line; no lane exchange is needed (a 16-byte load would hold channels of tiles the lane does not feed).  An extra
// im2col column k = 9*Cin of ones yields the bias gradient in the same MFMAs.  The gradient / code loads of a chunk
// are issued one chunk ahead, across strips of a run (the first one before the rows are staged), so they overlap the
// staging and the MFMAs.  Fragments are assembled with 32-bit integer ops on the raw bf16 bits.
// Work: runs of strips as in the forward (same LDS rows and prefetch); a workgroup takes runs blockIdx.x,
// blockIdx.x + gridDim.x, ... and writes ONE partial set at the end.  The per-wave accumulators are summed through
// the LDS the patch occupied.
template <int CIN, int NIT, bool A16, int WFIX>
__global__ __launch_bounds__(256, 2) void stem_bwd_mfma_kernel(const bf16_t* __restrict__ dy,
                                                            const unsigned char* __restrict__ code,
                                                            const float* __restrict__ x, float* __restrict__ partial,
                                                            int N, int H, int Wd, int run) {
  extern __shared__ float patch_raw[];
  bf16_t* patch = (bf16_t*)patch_raw;
  const unsigned short* patch16 = (const unsigned short*)patch_raw;
  constexpr int KT = 9 * CIN;
  float (*red)[KT + 1][STEM_COUT] = (float (*)[KT + 1][STEM_COUT])patch_raw;  // [4 waves], after the last strip
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
  const int W = WFIX ? WFIX : Wd;
  const int Ho = H / 2, Wo = W / 2, PW = W + 8, ROW = PW * CIN;
  const int upi = (Ho + run - 1) / run;
  // X-fragment gather offsets of this lane: k = l15 + 16*nt, reduction slot i -> pixel 2*lg + (i>>2), position i&3.
  // Lanes of the bias column (k == 9*Cin) use all-ones, lanes beyond it zeros: value = (raw & xand) | xor_.
  int xoff[2][8];
  unsigned xand[2], xor_[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int k = l15 + 16 * nt;
    const int dr = k / (3 * CIN), rem = k - dr * 3 * CIN;
    xand[nt] = k < KT ? 0xFFFFFFFFu : 0u;
    xor_[nt] = k == KT ? 0x3F803F80u : 0u;  // bf16 1.0 in both halves
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int px = 2 * lg + (i >> 2), qq = i & 3;
      xoff[nt][i] = k < KT ? ((qq >> 1) * PW + STEM_PADL - 1 + 2 * px + (qq & 1)) * CIN + dr * ROW + rem : 0;
    }
  }
  f32x4 acc[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint2 gd[2];
  unsigned gc[2];
  auto load_chunk = [&](long long strip, int pw0) {
    const long long o = ((strip * Wo + pw0 + 2 * lg) * STEM_COUT + 4 * l15);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      gd[h] = *(const uint2*)(dy + o + h * STEM_COUT);
      gc[h] = *(const unsigned*)(code + o + h * STEM_COUT);
    }
  };
  const bool active = wv * 8 < Wo;
  stem_zero_pads<CIN>(patch, 2 * min(run, Ho) + 2, W);

  for (int u = blockIdx.x; u < N * upi; u += gridDim.x) {
    const int n = u / upi, ph0 = (u - n * upi) * run;
    const int ns = min(run, Ho - ph0);
    const long long strip0 = (long long)n * Ho + ph0;
    if (active) load_chunk(strip0, wv * 8);
    {
      StemRowPair<CIN, NIT> pa, pb;
      stem_rows_load<CIN, NIT, A16>(pa, x, n, H, W, 2 * ph0 - 1);
      stem_rows_load<CIN, NIT, A16>(pb, x, n, H, W, 2 * ph0 + 1);
      stem_rows_store<CIN, NIT>(patch, pa, H, W, 2 * ph0 - 1, 0);
      stem_rows_store<CIN, NIT>(patch, pb, H, W, 2 * ph0 + 1, 2);
    }
    lds_barrier();
    StemRowPair<CIN, NIT> pa;
    // one chunk of 8 pixels; next: 0 = nothing to request, 1 = the strip's next chunk, 2 = the next strip's first
    auto do_chunk = [&](int s, int pw0, int next) {
      {
        // G fragment: dword d of (mt) holds reduction slots 2d, 2d+1 = pixel h = d>>1, positions 2(d&1), 2(d&1)+1
        u32x4 gf[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const unsigned cd = gc[h] >> (8 * mt);
            const unsigned dw2 = (mt >> 1) ? gd[h].y : gd[h].x;
            const unsigned g16 = (mt & 1) ? (dw2 >> 16) : (dw2 & 0xFFFFu);
            const unsigned g = (cd & 4u) ? g16 : 0u;
            const unsigned sh = g << ((cd & 1u) * 16u);   // low half for even positions, high half for odd
            gf[mt][h * 2 + 0] = (cd & 2u) ? 0u : sh;     // positions 0,1
            gf[mt][h * 2 + 1] = (cd & 2u) ? sh : 0u;     // positions 2,3
          }
        // next chunk's loads fly during this chunk's MFMAs
        if (next == 1) load_chunk(strip0 + s, pw0 + 32);
        else if (next == 2) load_chunk(strip0 + s + 1, wv * 8);
        u32x4 xf[2];
        const int pbase = 2 * s * ROW + 2 * pw0 * CIN;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const unsigned lo = patch16[pbase + xoff[nt][2 * d]];
            const unsigned hi = patch16[pbase + xoff[nt][2 * d + 1]];
            xf[nt][d] = ((lo | (hi << 16)) & xand[nt]) | xor_[nt];
          }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)&gf[mt], *(const bf16x8*)&xf[nt],
                                                                  acc[mt][nt], 0, 0, 0);
      }
    };
    // (`more` and, with WFIX, the chunk count are compile-time: the waits for the row loads can then be counted)
    auto do_strip = [&](int s, auto more_c) {
      constexpr bool more = decltype(more_c)::value;
      const int nrow0 = 2 * (ph0 + s) + 3;
      if (more) {
        stem_rows_load<CIN, NIT, A16>(pa, x, n, H, W, nrow0);
        __builtin_amdgcn_sched_barrier(0);  // requested before the strip's arithmetic, not in the middle of it
      }
      if (WFIX == 128) {
        do_chunk(s, wv * 8, 1);
        do_chunk(s, wv * 8 + 32, more ? 2 : 0);
      } else {
        for (int pw0 = wv * 8; pw0 < Wo; pw0 += 32) do_chunk(s, pw0, pw0 + 32 < Wo ? 1 : more ? 2 : 0);
      }
      if (more) stem_rows_store<CIN, NIT>(patch, pa, H, W, nrow0, 2 * s + 4);
      lds_barrier();  // after the last strip too: the next run's rows (or `red`) overwrite this one's
    };
    int s = 0;
    for (; s + 1 < ns; ++s) do_strip(s, std::true_type{});
    do_strip(s, std::false_type{});
  }
  // D rows = channels 4*(lg*4 + r) + mt, columns = k = l15 + 16*nt
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int k = l15 + 16 * nt;
      if (k <= KT)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wv][k][16 * lg + 4 * r + mt] = acc[mt][nt][r];
    }
  lds_barrier();
  for (int i = threadIdx.x; i < (KT + 1) * STEM_COUT; i += blockDim.x) {
    const int k = i / STEM_COUT, oc = i - k * STEM_COUT;
    partial[(long long)blockIdx.x * (KT + 1) * STEM_COUT + i] = red[0][k][oc] + red[1][k][oc] + red[2][k][oc] + red[3][k][oc];
  }
}

// dw[o][c][dr][ds] (strided) += sum_g partial[g][k][o];  dbias[o] += sum_g partial[g][9*CIN][o].
// grid (9*CIN + 1, 8): block (k, z) sums the partials g = z, z+8, ... with 8 thread groups, then one atomic per (k, o).
template <int CIN>
__global__ __launch_bounds__(512) void stem_bwd_reduce_kernel(const float* __restrict__ partial, int G,
                                                              float* __restrict__ dw, long long dsk, long long dsc,
                                                              long long dsr, long long dss,
                                                              float* __restrict__ dbias) {
  constexpr int KT = 9 * CIN;
  __shared__ float red[8][STEM_COUT];
  const int k = blockIdx.x, o = threadIdx.x & 63, part = threadIdx.x >> 6;  // 8 parts
  float s = 0.f;
  for (int g = blockIdx.y + 8 * part; g < G; g += 64) s += partial[((long long)g * (KT + 1) + k) * STEM_COUT + o];
  red[part][o] = s;
  __syncthreads();
  if (part == 0) {
#pragma unroll
    for (int p = 1; p < 8; ++p) s += red[p][o];
    if (k < KT) {
      const int c = k % CIN, t = k / CIN, ds = t % 3, dr = t / 3;
      if (dw) atomicAdd(&dw[o * dsk + c * dsc + dr * dsr + ds * dss], s);
    } else if (dbias) {
      atomicAdd(&dbias[o], s);
    }
  }
}

}  // namespace mr

using namespace mr;

#define DISPATCH_T(dtype, ...)                                   \
  if ((dtype) == MR_F32) { typedef float T; __VA_ARGS__; }       \
  else if ((dtype) == MR_BF16) { typedef bf16_t T; __VA_ARGS__; } \
  else { mr::set_error("bad dtype %d", (dtype)); return MR_ERR_DTYPE; }

static int stem_check(const char* who, int N, int Cin, int H, int W) {
  if (!(N > 0 && (Cin == 1 || Cin == 3) && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 &&
        4ll * (W + 2) * Cin * 4 <= 48 * 1024)) {
    mr::set_error("%s: unsupported shape N=%d Cin=%d H=%d W=%d (Cin in {1,3}, even H and W, W <= ~1000)", who, N,
                  Cin, H, W);
    return MR_ERR_ARG;
  }
  return MR_OK;
}

// MFMA kernels: pooled rows per workgroup run -- STEM_RUN, fewer when the image is lower or the run's 2*run + 2 LDS rows
// would not fit -- and the LDS bytes of those rows.
static int stem_run(int Cin, int H, int W) {
  int run = (STEM_LDS_ROWS_BYTES / ((W + 8) * Cin * 2) - 2) / 2;
  if (run > STEM_RUN) run = STEM_RUN;
  if (run > H / 2) run = H / 2;
  return run < 1 ? 1 : run;
}
// Instantiations of the MFMA kernels: NIT = 16-byte column groups of a row pair per thread (W <= 512: 1, <= 1024: 2, else
// 6: the widest admitted single-plane row); x that is not 16-byte aligned takes the widest one with dword loads; W = 128 (the
// recognition crop) has the width compiled in.
#define STEM_MFMA_DISPATCH(LAUNCH)                      \
  do {                                                  \
    if (Cin == 3) {                                     \
      if (!a16) LAUNCH(3, 2, false, 0);                 \
      else if (W == 128) LAUNCH(3, 1, true, 128);       \
      else if (W <= 512) LAUNCH(3, 1, true, 0);         \
      else LAUNCH(3, 2, true, 0);                       \
    } else {                                            \
      if (!a16) LAUNCH(1, 6, false, 0);                 \
      else if (W == 128) LAUNCH(1, 1, true, 128);       \
      else if (W <= 512) LAUNCH(1, 1, true, 0);         \
      else if (W <= 1024) LAUNCH(1, 2, true, 0);        \
      else LAUNCH(1, 6, true, 0);                       \
    }                                                   \
  } while (0)
static size_t stem_rows_lds(int Cin, int W, int run) { return (size_t)(2 * run + 2) * (W + 8) * Cin * 2; }

extern "C" {

long long mr_stem_bwd_workspace(int Cin) { return (long long)STEM_BWD_GROUPS * (9 * Cin + 1) * STEM_COUT; }

// bf16 filter bank for the MFMA forward path ([64][32], see stem_pack_kernel)
int mr_stem_pack(const float* w, long long wsk, long long wsc, long long wsr, long long wss, void* wpack, int Cin,
                 hipStream_t stream) {
  MR_CHECK_ARG(Cin == 1 || Cin == 3, "mr_stem_pack: Cin must be 1 or 3");
  if (Cin == 3)
    hipLaunchKernelGGL((stem_pack_kernel<3>), dim3(1), dim3(256), 0, stream, w, wsk, wsc, wsr, wss, (bf16_t*)wpack);
  else
    hipLaunchKernelGGL((stem_pack_kernel<1>), dim3(1), dim3(256), 0, stream, w, wsk, wsc, wsr, wss, (bf16_t*)wpack);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_stem_fwd(int dtype, const float* x, const float* w, long long wsk, long long wsc, long long wsr,
                long long wss, const void* wpack, const float* bias, void* y, unsigned char* code, int N, int Cin,
                int H, int W, hipStream_t stream) {
  if (int rc = stem_check("mr_stem_fwd", N, Cin, H, W)) return rc;
  const size_t lds = sizeof(float) * 4 * (W + 2) * Cin;
  const int strips = N * (H / 2);
  const int grid = strips < 8192 ? strips : 8192;
  if (dtype == MR_BF16 && (W / 2) % 16 == 0 && wpack != nullptr) {  // MFMA path
    const int run = stem_run(Cin, H, W);
    const dim3 g(N * cdiv(H / 2, run));
    const size_t l = stem_rows_lds(Cin, W, run);
    const bool a16 = ((uintptr_t)x & 15) == 0;
#define STEM_FWD(CIN, NIT, A16, WFIX)                                                                               \
  hipLaunchKernelGGL((stem_fwd_mfma_kernel<CIN, NIT, A16, WFIX>), g, dim3(256), l, stream, x, (const bf16_t*)wpack, bias, \
                     (bf16_t*)y, code, H, W, run)
    STEM_MFMA_DISPATCH(STEM_FWD);
#undef STEM_FWD
    MR_CHECK_LAUNCH();
    return MR_OK;
  }
  if (Cin == 3) {
    DISPATCH_T(dtype, hipLaunchKernelGGL((stem_fwd_kernel<T, 3>), dim3(grid), dim3(256), lds, stream, x, w, wsk, wsc,
                                         wsr, wss, bias, (T*)y, code, N, H, W));
  } else {
    DISPATCH_T(dtype, hipLaunchKernelGGL((stem_fwd_kernel<T, 1>), dim3(grid), dim3(256), lds, stream, x, w, wsk, wsc,
                                         wsr, wss, bias, (T*)y, code, N, H, W));
  }
  MR_CHECK_LAUNCH();
  return MR_OK;
}

// dw / dbias are ACCUMULATED into (either may be null); workspace: mr_stem_bwd_workspace(Cin) floats.
int mr_stem_bwd(int dtype, const void* dy, const unsigned char* code, const float* x, float* workspace, float* dw,
                long long dsk, long long dsc, long long dsr, long long dss, float* dbias, int N, int Cin, int H,
                int W, hipStream_t stream) {
  if (int rc = stem_check("mr_stem_bwd", N, Cin, H, W)) return rc;
  MR_CHECK_ARG(workspace != nullptr, "mr_stem_bwd: workspace is null");
  const size_t lds = sizeof(float) * 4 * (W + 2) * Cin;
  const int strips = N * (H / 2);
  const int G = strips < STEM_BWD_GROUPS ? strips : STEM_BWD_GROUPS;
  if (dtype == MR_BF16 && (W / 2) % 16 == 0 && ((uintptr_t)dy & 7) == 0 && ((uintptr_t)code & 3) == 0) {  // MFMA path
    const int run = stem_run(Cin, H, W);
    const long long units = (long long)N * cdiv(H / 2, run);
    const int Gm = units < STEM_BWD_GROUPS_MFMA ? (int)units : STEM_BWD_GROUPS_MFMA;
    const size_t red = sizeof(float) * 4 * (9 * Cin + 1) * STEM_COUT;   // the patch's LDS is reused for the wave sums
    const size_t rows = stem_rows_lds(Cin, W, run);
    const size_t l = rows > red ? rows : red;
    const bool a16 = ((uintptr_t)x & 15) == 0;
#define STEM_BWD(CIN, NIT, A16, WFIX)                                                                           \
  hipLaunchKernelGGL((stem_bwd_mfma_kernel<CIN, NIT, A16, WFIX>), dim3(Gm), dim3(256), l, stream, (const bf16_t*)dy, code, \
                     x, workspace, N, H, W, run)
    STEM_MFMA_DISPATCH(STEM_BWD);
#undef STEM_BWD
    if (Cin == 3) {
      hipLaunchKernelGGL((stem_bwd_reduce_kernel<3>), dim3(9 * 3 + 1, 8), dim3(512), 0, stream, workspace, Gm, dw, dsk,
                         dsc, dsr, dss, dbias);
    } else {
      hipLaunchKernelGGL((stem_bwd_reduce_kernel<1>), dim3(9 * 1 + 1, 8), dim3(512), 0, stream, workspace, Gm, dw, dsk,
                         dsc, dsr, dss, dbias);
    }
    MR_CHECK_LAUNCH();
    return MR_OK;
  }
  if (Cin == 3) {
    DISPATCH_T(dtype, hipLaunchKernelGGL((stem_bwd_kernel<T, 3>), dim3(G), dim3(256), lds, stream, (const T*)dy, code,
                                         x, workspace, N, H, W));
    hipLaunchKernelGGL((stem_bwd_reduce_kernel<3>), dim3(9 * 3 + 1, 8), dim3(512), 0, stream, workspace, G, dw, dsk, dsc,
                       dsr, dss, dbias);
  } else {
    DISPATCH_T(dtype, hipLaunchKernelGGL((stem_bwd_kernel<T, 1>), dim3(G), dim3(256), lds, stream, (const T*)dy, code,
                                         x, workspace, N, H, W));
    hipLaunchKernelGGL((stem_bwd_reduce_kernel<1>), dim3(9 * 1 + 1, 8), dim3(512), 0, stream, workspace, G, dw, dsk, dsc,
                       dsr, dss, dbias);
  }
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
