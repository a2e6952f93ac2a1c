// DB detector augmentation, the image half (include/megreader_hip.h: mr_warp_normalize).  The reference resamples three
// times per sample on the host -- imgaug Affine (rotate), imgaug Resize, cv2.resize of the crop in
// data/processes/random_crop_data.py:31-34 -- and normalises afterwards (normalize_image.py:8-17).  None of the geometric
// decisions reads a pixel, so the host composes them into one affine map per image (data/detection_augment.py) and this
// kernel samples the decoded uint8 source ONCE along it, bilinear, writing the normalised NCHW canvas directly.
// Byte-gather work bound by HBM and the texture-address path: no LDS, no reuse staged by hand (at most 10 degrees of
// rotation, so neighbouring lanes hit the same cache lines).  One thread per canvas pixel, threads along u: a wavefront
// reads 64 neighbouring source pixels per tap and writes 256 consecutive bytes per plane.  Measured against 2 and 4 pixels
// per thread with 16-byte stores (CHANGELOG.md, "Fused DB detection augmentation"): this form is the fastest on every
// augmenting plan -- the wider forms spread one load instruction over 2 and 4 times as many cache lines.
#include "common.h"
#include "../../include/megreader_hip.h"

// Bit-exactness against the numpy restatement (tests/_db_augment_ref.py): every product and sum of this file is rounded
// on its own (hipcc contracts a*b + c*d into an fma by default).
#pragma clang fp contract(off)

namespace mr {

static_assert(sizeof(mr_warp_desc) == 128, "mr_warp_desc is mirrored by ctypes (data/detection_augment.py)");

// One source pixel (3 bytes) as floats; 0 outside the image or outside the uploaded window.  Only bytes of the window are
// ever addressed: row r < win_h at offset + r * pitch, column k < win_w.
__device__ __forceinline__ void warp_tap(const unsigned char* win, const mr_warp_desc& d, int xx, int yy, float p[3]) {
  const int k = xx - d.win_x, r = yy - d.win_y;
  const bool in = xx >= 0 && xx < d.src_w && yy >= 0 && yy < d.src_h && k >= 0 && k < d.win_w && r >= 0 && r < d.win_h;
  p[0] = p[1] = p[2] = 0.f;
  if (in) {
    const unsigned char* s = win + (long long)r * d.pitch + 3 * k;
    p[0] = (float)s[0];
    p[1] = (float)s[1];
    p[2] = (float)s[2];
  }
}

__global__ __launch_bounds__(256) void warp_normalize_kernel(const unsigned char* src, const mr_warp_desc* desc, int N,
                                                             int Hd, int Wd, double m0, double m1, double m2, float* dst) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;   // N * Hd * Wd < 2^31 (checked by the host)
  if (gid >= (unsigned)N * Hd * Wd) return;
  const unsigned row = gid / Wd;
  const int u = (int)(gid - row * Wd);
  const int n = (int)(row / Hd), v = (int)(row - (unsigned)n * Hd);
  const mr_warp_desc d = desc[n];
  const unsigned char* win = src + d.offset;
  float val[3] = {0.f, 0.f, 0.f};
  if (v < d.dst_h && u < d.dst_w) {
    const double uc = fmin(fmax((double)u, d.cu0), d.cu1);
    const double vc = fmin(fmax((double)v, d.cv0), d.cv1);
    const double x = d.a[0] * uc + d.a[1] * vc + d.a[2];
    const double y = d.a[3] * uc + d.a[4] * vc + d.a[5];
    // all four taps are outside the image otherwise (this also keeps a NaN or a huge coordinate away from the int cast)
    if (x > -1.0 && x < (double)d.src_w && y > -1.0 && y < (double)d.src_h) {
      const double xf = floor(x), yf = floor(y);
      const float fx = (float)(x - xf), fy = (float)(y - yf);
      const int ix = (int)xf, iy = (int)yf;
      float p00[3], p01[3], p10[3], p11[3];
      warp_tap(win, d, ix, iy, p00);
      warp_tap(win, d, ix + 1, iy, p01);
      warp_tap(win, d, ix, iy + 1, p10);
      warp_tap(win, d, ix + 1, iy + 1, p11);
      const float gx = 1.f - fx, gy = 1.f - fy;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = p00[c] * gx + p01[c] * fx;
        const float bot = p10[c] * gx + p11[c] * fx;
        val[c] = top * gy + bot * fy;
      }
    }
  }
  const double mean[3] = {m0, m1, m2};
  const long long per = (long long)Hd * Wd;
  float* o = dst + (long long)n * 3 * per + (long long)v * Wd + u;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * per] = (float)((double)val[c] - mean[c]) / 255.f;
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_warp_desc(void) { return (int)sizeof(mr_warp_desc); }

int mr_warp_normalize(const unsigned char* src, const void* desc, int N, int H, int W, double mean0, double mean1,
                      double mean2, float* dst, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && H > 0 && W > 0, "mr_warp_normalize: bad shape N=%d H=%d W=%d", N, H, W);
  if (N == 0) return MR_OK;
  MR_CHECK_ARG(src != nullptr && desc != nullptr && dst != nullptr, "mr_warp_normalize: null pointer");
  const long long total = (long long)N * H * W;
  MR_CHECK_ARG(total < 0x7fffff00LL, "mr_warp_normalize: N=%d H=%d W=%d exceed one launch", N, H, W);
  hipLaunchKernelGGL(warp_normalize_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, src,
                     (const mr_warp_desc*)desc, N, H, W, mean0, mean1, mean2, dst);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
