// Recognition augmentation (include/megreader_hip.h: mr_rec_augment): geometric jitter, a wavy baseline, a colour map, a 5 x 5
// blur, noise, pixelation and erased rectangles per sample, in ONE bilinear pass from the resident uint8 photos to the recogniser's
// normalised f32 planes.  The host plans each sample from shapes alone (data/recognition_augment.py); no decision reads a pixel.
//
// The launch shape is the renderer's (csrc/synth_text.hip).  One workgroup of 256 threads renders one 16 x 64 tile of one
// descriptor's canvas:
//   1. the knots dx, dy go to LDS (they are indexed per pixel); every other field of the descriptor is read at a
//      workgroup-uniform address;
//   2. comp -- displaced sampling point, jitter g, clamp, the crop map h, the four taps and the blend (bilinear3 of image_sample.h,
//      the crop kernels' core), the colour map -- is evaluated ONCE per cell of the tile and its halo of 2 (20 x 68 cells at the
//      coordinates the blur clamps its taps to) into LDS, 16 KB; without blur, of the tile alone;
//   3. the 25-tap sum runs out of LDS (the kernel is a general 5 x 5: a motion line is not separable), then the rectangles, the
//      noise and the normalising store, threads along u: 256 consecutive bytes per wave and plane.
// The stride of the LDS array is 3 dwords per cell along u: odd, so the 32 lanes of a half wave fall on 32 banks.
//
// Nothing the tables hold can make the kernel read outside the photos or the tables, write outside the N rows of dst, or loop
// without bound: `row` and `image` are tested against N and I, dst_w is cut to [0, W], n_erase to [0, MR_AUG_MAX_ERASE], quant
// to >= 1, the knot index to [0, 7], and a photo byte is addressed only for 0 <= row < h, 0 <= column < w.
#include "common.h"
#include "../../include/megreader_hip.h"
#include "image_sample.h"

#include <limits.h>

#include <vector>

// Bit-exactness against the numpy restatement (tests/_rec_augment_ref.py): every product and sum is rounded on its own.
#pragma clang fp contract(off)

namespace mr {

static_assert(sizeof(mr_aug_desc) == 560, "mr_aug_desc is mirrored by ctypes (data/recognition_augment.py)");
static_assert(MR_AUG_KNOTS == 9 && MR_AUG_MAX_ERASE == 4, "the array sizes of mr_aug_desc");

namespace aug {

constexpr int TH = MR_SYNTH_TILE_H, TW = MR_SYNTH_TILE_W, HALO = 2;
constexpr int CH = TH + 2 * HALO, CW = TW + 2 * HALO;

__device__ __forceinline__ unsigned lowbias32(unsigned r) {
  r ^= r >> 16;
  r *= 0x7FEB352Du;
  r ^= r >> 15;
  r *= 0x846CA68Bu;
  r ^= r >> 16;
  return r;
}

// comp(u, v) of include/megreader_hip.h.  wv: dst_w cut to [1, W]; q: quant cut to >= 1.
__device__ __forceinline__ void comp(const mr_aug_desc* __restrict__ d, const float* s_dx, const float* s_dy,
                                     const unsigned char* pix, int pitch, int pw, int ph, int wv, int q, int u, int v,
                                     float col[3]) {
  const int bu = (u / q) * q, bv = (v / q) * q;
  const double half = 0.5 * (double)q;
  const double U = (double)bu + half, V = (double)bv + half;
  const double t = U * 8.0 / (double)wv;
  const int j = (int)fmin(fmax(floor(t), 0.0), 7.0);
  const double f = t - (double)j;
  const double dxa = (double)s_dx[j], dxb = (double)s_dx[j + 1], dya = (double)s_dy[j], dyb = (double)s_dy[j + 1];
  const double U1 = U + (dxa + (dxb - dxa) * f);
  const double V1 = V + (dya + (dyb - dya) * f);
  const double cx = U1 * d->sx - 0.5, cy = V1 * d->sy - 0.5;
  const double X = d->g[0] * cx + d->g[1] * cy + d->g[2];
  const double Y = d->g[3] * cx + d->g[4] * cy + d->g[5];
  const double D = d->g[6] * cx + d->g[7] * cy + d->g[8];
  const double px = fmin(fmax(X / D, d->cu0), d->cu1);
  const double py = fmin(fmax(Y / D, d->cv0), d->cv1);
  const double X2 = d->h[0] * px + d->h[1] * py + d->h[2];
  const double Y2 = d->h[3] * px + d->h[4] * py + d->h[5];
  const double D2 = d->h[6] * px + d->h[7] * py + d->h[8];
  const double x = X2 / D2, y = Y2 / D2;
  float val[3] = {0.f, 0.f, 0.f};
  bilinear3(D > 0.0 && D2 > 0.0, x, y, pw, ph, [&](int xx, int yy, float p[3]) {   // D <= 0 or NaN: behind a map's horizon
    tap3(xx >= 0 && xx < pw && yy >= 0 && yy < ph, pix, pitch, yy, xx, p);
  }, val);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    col[c] = fminf(fmaxf(d->m[3 * c] * val[0] + d->m[3 * c + 1] * val[1] + d->m[3 * c + 2] * val[2] + d->b[c], 0.f), 255.f);
}

__global__ __launch_bounds__(256) void rec_augment_kernel(const unsigned char* __restrict__ src,
                                                          const mr_crop_image* __restrict__ images, int I,
                                                          const mr_aug_desc* __restrict__ descs, int N, int H, int W,
                                                          int tiles_x, int tiles_y, double m0, double m1, double m2,
                                                          float* __restrict__ dst) {
  __shared__ float s_comp[CH * CW * 3];
  __shared__ float s_dx[MR_AUG_KNOTS], s_dy[MR_AUG_KNOTS];

  const int tid = threadIdx.x;
  const unsigned per = (unsigned)tiles_x * (unsigned)tiles_y;
  const unsigned mi = blockIdx.x / per;
  const unsigned t = blockIdx.x - mi * per;
  const int ty0 = (int)(t / (unsigned)tiles_x) * TH, tx0 = (int)(t % (unsigned)tiles_x) * TW;
  const mr_aug_desc* __restrict__ d = descs + mi;
  const int row = d->row;
  if (row < 0 || row >= N) return;                                    // (uniform: the whole workgroup leaves)
  const int image = d->image;
  const int wv = min(max(d->dst_w, 0), W);
  const bool live = image >= 0 && image < I && tx0 < wv;              // otherwise the tile is all zero canvas
  const bool blur = d->blur != 0;

  if (live) {
    if (tid < MR_AUG_KNOTS) {
      s_dx[tid] = d->dx[tid];
      s_dy[tid] = d->dy[tid];
    }
    __syncthreads();
    const mr_crop_image im = images[image];
    const unsigned char* pix = src + im.offset;
    const int q = max(d->quant, 1);
    for (int cell = tid; cell < CH * CW; cell += 256) {
      const int cy = cell / CW, cx = cell - cy * CW;
      if (!blur && (cy < HALO || cy >= HALO + TH || cx < HALO || cx >= HALO + TW)) continue;
      const int u = min(max(tx0 - HALO + cx, 0), wv - 1), v = min(max(ty0 - HALO + cy, 0), H - 1);
      float col[3];
      comp(d, s_dx, s_dy, pix, im.pitch, im.w, im.h, wv, q, u, v, col);
#pragma unroll
      for (int c = 0; c < 3; ++c) s_comp[cell * 3 + c] = col[c];
    }
    __syncthreads();
  }

  const int ne = min(max(d->n_erase, 0), MR_AUG_MAX_ERASE);
  const float amp = d->noise_amp;
  const unsigned seed = (unsigned)d->seed;
  for (int p = tid; p < TH * TW; p += 256) {
    const int ty = p / TW, tx = p - ty * TW;
    const int u = tx0 + tx, v = ty0 + ty;
    if (u >= W || v >= H) continue;
    float col[3] = {0.f, 0.f, 0.f};
    if (live && u < wv) {
      if (blur) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
              const float term = d->k[j * 5 + i] * s_comp[((ty + j) * CW + tx + i) * 3 + c];
              acc = (i == 0 && j == 0) ? term : acc + term;
            }
          col[c] = acc;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c] = s_comp[((ty + HALO) * CW + tx + HALO) * 3 + c];
      }
      for (int e = 0; e < ne; ++e)
        if (u >= d->erase[4 * e] && u < d->erase[4 * e + 1] && v >= d->erase[4 * e + 2] && v < d->erase[4 * e + 3]) {
#pragma unroll
          for (int c = 0; c < 3; ++c) col[c] = d->erase_col[3 * e + c];
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned kk = ((unsigned)v * (unsigned)W + (unsigned)u) * 3u + (unsigned)c;
        const unsigned r = lowbias32(seed + kk * 0x9E3779B9u);
        col[c] = col[c] + amp * ((float)(r >> 8) * 0x1p-24f - 0.5f);
        col[c] = fminf(fmaxf(col[c], 0.f), 255.f);
      }
    }
    store_normalized(dst, row, v, u, H, W, col, m0, m1, m2);
  }
}

}  // namespace aug
}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_aug_desc(void) { return (int)sizeof(mr_aug_desc); }

int mr_rec_augment(const unsigned char* src, const void* images, int I, const void* descs, int M, int N, int H, int W,
                   double mean0, double mean1, double mean2, float* dst, hipStream_t stream) {
  MR_CHECK_ARG(I >= 0 && M >= 0 && N >= 0 && H >= 1 && W >= 1, "mr_rec_augment: bad shape I=%d M=%d N=%d H=%d W=%d", I, M, N, H,
               W);
  if (M == 0) return MR_OK;
  MR_CHECK_ARG(src != nullptr && images != nullptr && descs != nullptr && dst != nullptr, "mr_rec_augment: null pointer");
  const int tiles_x = cdiv(W, aug::TW), tiles_y = cdiv(H, aug::TH);
  const long long tiles = (long long)tiles_x * tiles_y * M;
  MR_CHECK_ARG(tiles <= (long long)INT_MAX, "mr_rec_augment: M=%d H=%d W=%d are %lld tiles, more than one launch", M, H, W,
               tiles);
  // A table in pinned host memory is readable on both sides: check it here.  Device memory is the kernel's to guard.
  // (Not while `stream` is being captured: a capture records the launch alone, and a replay would not repeat the check.)
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) (void)hipGetLastError();
  hipPointerAttribute_t attr;
  if (capturing == hipStreamCaptureStatusNone && hipPointerGetAttributes(&attr, descs) == hipSuccess &&
      attr.type == hipMemoryTypeHost) {
    const mr_aug_desc* hd = (const mr_aug_desc*)descs;
    std::vector<bool> named((size_t)N, false);
    for (int m = 0; m < M; ++m) {
      MR_CHECK_ARG(hd[m].row >= 0 && hd[m].row < N, "mr_rec_augment: descriptor %d names row %d of %d", m, hd[m].row, N);
      MR_CHECK_ARG(!named[hd[m].row], "mr_rec_augment: descriptor %d names row %d again", m, hd[m].row);
      named[hd[m].row] = true;
      MR_CHECK_ARG(hd[m].image >= 0 && hd[m].image < I, "mr_rec_augment: descriptor %d names photo %d of %d", m, hd[m].image,
                   I);
      MR_CHECK_ARG(hd[m].n_erase >= 0 && hd[m].n_erase <= MR_AUG_MAX_ERASE, "mr_rec_augment: descriptor %d has %d rectangles", m,
                   hd[m].n_erase);
      MR_CHECK_ARG(hd[m].dst_w >= 1 && hd[m].dst_w <= W, "mr_rec_augment: descriptor %d has dst_w %d of %d", m, hd[m].dst_w, W);
    }
  } else {
    (void)hipGetLastError();    // an address the runtime does not know is no error of this call
  }
  hipLaunchKernelGGL(aug::rec_augment_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, src, (const mr_crop_image*)images,
                     I, (const mr_aug_desc*)descs, N, H, W, tiles_x, tiles_y, mean0, mean1, mean2, dst);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
