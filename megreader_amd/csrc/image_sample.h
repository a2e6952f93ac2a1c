// What the byte-gather kernels of csrc/image_sample.hip and the renderer of csrc/synth_text.hip share: the zero-border tap, the
// guarded bilinear blend and the normalising store.  They promise bit-equal results where their maps coincide
// (include/megreader_hip.h), so these are written once.
#pragma once
#include "common.h"

// Every product and sum below, and of the file that includes this one from here on, is rounded on its own (hipcc contracts
// a*b + c*d into an fma by default).
#pragma clang fp contract(off)

namespace mr {

// One source pixel (3 bytes) as floats: row r, column k of `base`, or 0 where the caller found it outside.  No byte is
// addressed unless `inside`.
__device__ __forceinline__ void tap3(bool inside, const unsigned char* base, int pitch, int r, int k, float p[3]) {
  p[0] = p[1] = p[2] = 0.f;
  if (inside) {
    const unsigned char* s = base + (long long)r * pitch + 3 * k;
    p[0] = (float)s[0];
    p[1] = (float)s[1];
    p[2] = (float)s[2];
  }
}

// val = the bilinear sample at (x, y) of a source of w columns and h rows whose pixels `tap(xx, yy, p)` reads (0 outside):
// floor, float32 fractions, four taps, horizontal pass then vertical pass.  Outside (-1, w) x (-1, h) all four taps are
// outside and val keeps its zeros; the test also keeps a NaN, an infinity or a huge coordinate away from the int cast.
// `ok`: a condition of the caller's map that joins the test (one branch for both: the form the crop kernel was measured in).
template <typename Tap>
__device__ __forceinline__ void bilinear3(bool ok, double x, double y, int w, int h, Tap tap, float val[3]) {
  if (ok && x > -1.0 && x < (double)w && y > -1.0 && y < (double)h) {
    const double xf = floor(x), yf = floor(y);
    const float fx = (float)(x - xf), fy = (float)(y - yf);
    const int ix = (int)xf, iy = (int)yf;
    float p00[3], p01[3], p10[3], p11[3];
    tap(ix, iy, p00);
    tap(ix + 1, iy, p01);
    tap(ix, iy + 1, p10);
    tap(ix + 1, iy + 1, p11);
    const float gx = 1.f - fx, gy = 1.f - fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = p00[c] * gx + p01[c] * fx;
      const float bot = p10[c] * gx + p11[c] * fx;
      val[c] = top * gy + bot * fy;
    }
  }
}

// dst[n][c][y][x] = (float)((double)val[c] - mean[c]) / 255.f: normalize_image.py:8-17 (-= RGB_MEAN in double, /= 255 in f32,
// HWC -> CHW).
__device__ __forceinline__ void store_normalized(float* dst, int n, int y, int x, int Hd, int Wd, const float val[3],
                                                 double m0, double m1, double m2) {
  const double mean[3] = {m0, m1, m2};
  const long long per = (long long)Hd * Wd;
  float* o = dst + (long long)n * 3 * per + (long long)y * Wd + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * per] = (float)((double)val[c] - mean[c]) / 255.f;
}

}  // namespace mr
