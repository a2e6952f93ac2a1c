// The three byte-gather kernels of the input side: mr_resize_normalize (the recogniser's and the detector's plain input),
// mr_warp_normalize (the DB detector's training augmentation) and mr_quad_crop (text-line crops for the recogniser).  Each reads
// packed uint8 HWC pixels along its own coordinate map and writes normalised f32 planes; they promise bit-equal results where
// their maps coincide (include/megreader_hip.h), so what they share -- the canvas index split, the zero-border tap, the guarded
// bilinear blend and the normalising store -- is written once, here and in image_sample.h (which csrc/synth_text.hip shares).
//
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
//
// Quad crops (include/megreader_hip.h: mr_quad_crop): the reference's `ImageCropper.crop` (data/crop_file_dataset.py:105-124)
// rectifies a quadrilateral with warpPerspective, turns a tall crop on its side (`ensure_horizontal`), resizes it with
// cv2.resize and normalises it -- two resamplings on the host per text line.  None of the geometry reads a pixel, so the
// host composes it into one projective map and one resize rule per crop (data/quad_crop.py) and this kernel samples the
// resident uint8 photo ONCE along them, bilinear, writing the normalised recognition batch directly.
// The same byte gather as mr_warp_normalize and the form measured fastest there: one thread per canvas pixel, threads
// along u, so a wavefront reads neighbouring source pixels per tap and writes 256 consecutive bytes per plane.  No LDS: the
// photo stays in L2 across the hundreds of crops that read it.
#include "common.h"
#include "../../include/megreader_hip.h"
#include "image_sample.h"

// Bit-exactness against the numpy restatements (oracle/pipeline.py, tests/_db_augment_ref.py, tests/_quad_crop_ref.py): every
// product and sum of this file is rounded on its own (hipcc contracts a*b + c*d into an fma by default, and HIP's __fmul_rn /
// __fadd_rn are plain operators that get contracted too); the two float64 divisions of the crop map are correctly rounded on
// both sides.
#pragma clang fp contract(off)

namespace mr {

static_assert(sizeof(mr_img_desc) == 40, "mr_img_desc is mirrored by ctypes (data/device_pipeline.py)");
static_assert(sizeof(mr_warp_desc) == 128, "mr_warp_desc is mirrored by ctypes (data/detection_augment.py)");
static_assert(sizeof(mr_crop_image) == 24, "mr_crop_image is mirrored by ctypes (data/quad_crop.py)");
static_assert(sizeof(mr_crop_desc) == 112, "mr_crop_desc is mirrored by ctypes (data/quad_crop.py)");
static_assert(sizeof(mr_strip_desc) == 776, "mr_strip_desc is mirrored by ctypes (data/strip_crop.py)");

// Canvas pixel number gid of [N][Hd][Wd], threads along u: image n, row v, column u.
__device__ __forceinline__ void canvas_split(unsigned gid, int Hd, int Wd, int& n, int& v, int& u) {
  const unsigned row = gid / Wd;
  u = (int)(gid - row * Wd);
  n = (int)(row / Hd);
  v = (int)(row - (unsigned)n * Hd);
}

// dst[n, c, y, x] = ((double)resize(src_n)[y, x, c] - mean[c]) -> f32, / 255.f ; canvas columns >= dst_w hold the
// normalised value of a zero pixel (mode "pad": resize_image.py:48-53 pastes into a zero canvas BEFORE normalising).
// cv2.resize float32 INTER_LINEAR: fx = (float)((x + 0.5) * scale - 0.5) with scale in double, taps clamped with the
// weight of the out-of-range tap forced to 0, horizontal pass then vertical pass, plain float mul/add (no fma).
__global__ __launch_bounds__(256) void resize_normalize_kernel(const unsigned char* src, const mr_img_desc* desc, int N,
                                                               int Hd, int Wd, double m0, double m1, double m2,
                                                               float* dst) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)Hd * Wd;
  if (gid >= per * N) return;
  const int n = (int)(gid / per);
  const int y = (int)((gid % per) / Wd), x = (int)(gid % Wd);
  const mr_img_desc d = desc[n];
  float v[3] = {0.f, 0.f, 0.f};
  if (x < d.dst_w) {
    const unsigned char* s = src + d.offset;
    if (d.h == Hd && d.w == d.dst_w) {   // cv2.resize returns a copy when the size already matches
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (float)s[(long long)y * d.pitch + 3 * x + c];
    } else {
      const double sx_scale = d.scale_x, sy_scale = d.scale_y;
      float fx = (float)((x + 0.5) * sx_scale - 0.5);   // rounded product, then rounded sum (contraction is off)
      int sx = (int)floorf(fx);
      fx -= sx;
      if (sx < 0) { sx = 0; fx = 0.f; }
      if (sx >= d.w - 1) { sx = d.w - 1; fx = 0.f; }
      float fy = (float)((y + 0.5) * sy_scale - 0.5);
      int sy = (int)floorf(fy);
      fy -= sy;
      if (sy < 0) { sy = 0; fy = 0.f; }
      if (sy >= d.h - 1) { sy = d.h - 1; fy = 0.f; }
      const int sx1 = min(sx + 1, d.w - 1), sy1 = min(sy + 1, d.h - 1);
      const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
      const unsigned char* r0 = s + (long long)sy * d.pitch;
      const unsigned char* r1 = s + (long long)sy1 * d.pitch;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = (float)r0[3 * sx + c] * a0 + (float)r0[3 * sx1 + c] * a1;
        const float bot = (float)r1[3 * sx + c] * a0 + (float)r1[3 * sx1 + c] * a1;
        v[c] = top * b0 + bot * b1;
      }
    }
  }
  store_normalized(dst, n, y, x, Hd, Wd, v, m0, m1, m2);
}

// mr_warp_normalize: the affine map of one augmentation plan.  A tap outside the image or outside the uploaded window is 0;
// only bytes of the window are ever addressed: row r < win_h at offset + r * pitch, column k < win_w.
__global__ __launch_bounds__(256) void warp_normalize_kernel(const unsigned char* src, const mr_warp_desc* desc, int N,
                                                             int Hd, int Wd, double m0, double m1, double m2, float* dst) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;   // N * Hd * Wd < 2^31 (checked by the host)
  if (gid >= (unsigned)N * Hd * Wd) return;
  int n, v, u;
  canvas_split(gid, Hd, Wd, n, v, u);
  const mr_warp_desc d = desc[n];
  const unsigned char* win = src + d.offset;
  float val[3] = {0.f, 0.f, 0.f};
  if (v < d.dst_h && u < d.dst_w) {
    const double uc = fmin(fmax((double)u, d.cu0), d.cu1);
    const double vc = fmin(fmax((double)v, d.cv0), d.cv1);
    const double x = d.a[0] * uc + d.a[1] * vc + d.a[2];
    const double y = d.a[3] * uc + d.a[4] * vc + d.a[5];
    bilinear3(true, x, y, d.src_w, d.src_h, [&](int xx, int yy, float p[3]) {
      const int k = xx - d.win_x, r = yy - d.win_y;
      tap3(xx >= 0 && xx < d.src_w && yy >= 0 && yy < d.src_h && k >= 0 && k < d.win_w && r >= 0 && r < d.win_h, win,
           d.pitch, r, k, p);
    }, val);
  }
  store_normalized(dst, n, v, u, Hd, Wd, val, m0, m1, m2);
}

// mr_quad_crop: cv2.resize's sampling point of the (rotated) crop frame, then the projective map into the photo.  A tap
// outside the photo is 0; only bytes of the photo are ever addressed.
__global__ __launch_bounds__(256) void quad_crop_kernel(const unsigned char* src, const mr_crop_image* images, int I,
                                                        const mr_crop_desc* crops, int M, int Hd, int Wd, double m0,
                                                        double m1, double m2, float* dst) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;   // M * Hd * Wd < 2^31 (checked by the host)
  if (gid >= (unsigned)M * Hd * Wd) return;
  int m, v, u;
  canvas_split(gid, Hd, Wd, m, v, u);
  const mr_crop_desc d = crops[m];
  float val[3] = {0.f, 0.f, 0.f};
  if (u < d.dst_w && d.image >= 0 && d.image < I) {
    const mr_crop_image im = images[d.image];
    const double cx = fmin(fmax(((double)u + 0.5) * d.sx - 0.5, 0.0), d.cu1);
    const double cy = fmin(fmax(((double)v + 0.5) * d.sy - 0.5, 0.0), d.cv1);
    const double X = d.h[0] * cx + d.h[1] * cy + d.h[2];
    const double Y = d.h[3] * cx + d.h[4] * cy + d.h[5];
    const double D = d.h[6] * cx + d.h[7] * cy + d.h[8];
    const double x = X / D, y = Y / D;
    const unsigned char* pix = src + im.offset;
    bilinear3(D > 0.0, x, y, im.w, im.h, [&](int xx, int yy, float p[3]) {      // D <= 0 or NaN: behind the map's horizon
      tap3(xx >= 0 && xx < im.w && yy >= 0 && yy < im.h, pix, im.pitch, yy, xx, p);
    }, val);
  }
  store_normalized(dst, m, v, u, Hd, Wd, val, m0, m1, m2);
}

// mr_strip_crop: mr_quad_crop's sampling point of the strip's frame, then the piecewise-bilinear mesh into the photo.  One
// workgroup per (crop, 64 canvas columns): the descriptor is uniform, the first wavefront finds every column's cell and blends
// its top and bottom point ONCE (the search over the knots, a division and four blends in float64), then each wavefront takes
// every fourth row and a pixel costs two blends -- the order the restatement (tests/_strip_crop_ref.py) rounds in.  Lanes run
// along u as in quad_crop_kernel: 256 consecutive bytes per plane and store.
constexpr int STRIP_COLS = 64;
__global__ __launch_bounds__(256) void strip_crop_kernel(const unsigned char* src, const mr_crop_image* images, int I,
                                                         const mr_strip_desc* strips, int tiles, int Hd, int Wd, double m0,
                                                         double m1, double m2, float* dst) {
  __shared__ double col[STRIP_COLS][4];                 // top.x, top.y, bot.x, bot.y of the column
  const int m = (int)(blockIdx.x / (unsigned)tiles);
  const int lane = threadIdx.x & 63, u = (int)(blockIdx.x - (unsigned)m * tiles) * STRIP_COLS + lane;
  const mr_strip_desc* d = strips + m;
  const int image = d->image, dst_w = d->dst_w, knots = d->knots;
  const bool sampled = image >= 0 && image < I && knots >= 2 && knots <= 18 && u < dst_w && u < Wd;
  if (threadIdx.x < STRIP_COLS && sampled) {
    const double cx = fmin(fmax(((double)u + 0.5) * d->sx - 0.5, 0.0), d->cu1);
    int i = 0;
    for (int j = 1; j <= knots - 2; ++j) i = d->s[j] <= cx ? j : i;
    const double a = (cx - d->s[i]) / (d->s[i + 1] - d->s[i]), g = 1.0 - a;
    col[lane][0] = d->top[i][0] * g + d->top[i + 1][0] * a;
    col[lane][1] = d->top[i][1] * g + d->top[i + 1][1] * a;
    col[lane][2] = d->bot[i][0] * g + d->bot[i + 1][0] * a;
    col[lane][3] = d->bot[i][1] * g + d->bot[i + 1][1] * a;
  }
  __syncthreads();
  if (u >= Wd) return;
  mr_crop_image im = {0, 0, 0, 0, 0};
  if (sampled) im = images[image];
  const unsigned char* pix = src + im.offset;
  const double sy = d->sy, cv1 = d->cv1, hgt = d->hgt;
  for (int v = threadIdx.x >> 6; v < Hd; v += 4) {
    float val[3] = {0.f, 0.f, 0.f};
    if (sampled) {
      const double cy = fmin(fmax(((double)v + 0.5) * sy - 0.5, 0.0), cv1);
      const double b = cy / hgt, g = 1.0 - b;
      const double x = col[lane][0] * g + col[lane][2] * b, y = col[lane][1] * g + col[lane][3] * b;
      bilinear3(true, x, y, im.w, im.h, [&](int xx, int yy, float p[3]) {       // a NaN or an infinity fails the range test
        tap3(xx >= 0 && xx < im.w && yy >= 0 && yy < im.h, pix, im.pitch, yy, xx, p);
      }, val);
    }
    store_normalized(dst, m, v, u, Hd, Wd, val, m0, m1, m2);
  }
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_img_desc(void) { return (int)sizeof(mr_img_desc); }
int mr_sizeof_warp_desc(void) { return (int)sizeof(mr_warp_desc); }
int mr_sizeof_crop_image(void) { return (int)sizeof(mr_crop_image); }
int mr_sizeof_crop_desc(void) { return (int)sizeof(mr_crop_desc); }

int mr_resize_normalize(const unsigned char* src, const void* desc, int N, int H, int W, double mean0, double mean1,
                        double mean2, float* dst, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && H > 0 && W > 0, "mr_resize_normalize: bad shape N=%d H=%d W=%d", N, H, W);
  if (N == 0) return MR_OK;
  const long long total = (long long)N * H * W;
  hipLaunchKernelGGL(resize_normalize_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, src,
                     (const mr_img_desc*)desc, N, H, W, mean0, mean1, mean2, dst);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

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

int mr_quad_crop(const unsigned char* src, const void* images, int I, const void* crops, int M, int H, int W, double mean0,
                 double mean1, double mean2, float* dst, hipStream_t stream) {
  MR_CHECK_ARG(I >= 0 && M >= 0 && H > 0 && W > 0, "mr_quad_crop: bad shape I=%d M=%d H=%d W=%d", I, M, H, W);
  if (M == 0) return MR_OK;
  MR_CHECK_ARG(src != nullptr && images != nullptr && crops != nullptr && dst != nullptr, "mr_quad_crop: null pointer");
  MR_CHECK_ARG(I > 0, "mr_quad_crop: %d crops and no photo", M);
  const long long total = (long long)M * H * W;
  MR_CHECK_ARG(total < 0x7fffff00LL, "mr_quad_crop: M=%d H=%d W=%d exceed one launch", M, H, W);
  // A table in pinned host memory is readable on both sides: check the indices here.  Device memory is the kernel's to check.
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, crops) == hipSuccess && attr.type == hipMemoryTypeHost) {
    const mr_crop_desc* c = (const mr_crop_desc*)crops;
    for (int m = 0; m < M; ++m)
      MR_CHECK_ARG(c[m].image >= 0 && c[m].image < I, "mr_quad_crop: crop %d names photo %d of %d", m, c[m].image, I);
  } else {
    (void)hipGetLastError();    // an address the runtime does not know is no error of this call
  }
  hipLaunchKernelGGL(quad_crop_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, src,
                     (const mr_crop_image*)images, I, (const mr_crop_desc*)crops, M, H, W, mean0, mean1, mean2, dst);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_sizeof_strip_desc(void) { return (int)sizeof(mr_strip_desc); }

int mr_strip_crop(const unsigned char* src, const void* images, int I, const void* strips, int M, int H, int W, double mean0,
                  double mean1, double mean2, float* dst, hipStream_t stream) {
  MR_CHECK_ARG(I >= 0 && M >= 0 && H > 0 && W > 0, "mr_strip_crop: bad shape I=%d M=%d H=%d W=%d", I, M, H, W);
  if (M == 0) return MR_OK;
  MR_CHECK_ARG(src != nullptr && images != nullptr && strips != nullptr && dst != nullptr, "mr_strip_crop: null pointer");
  MR_CHECK_ARG(I > 0, "mr_strip_crop: %d crops and no photo", M);
  const long long tiles = cdivll(W, STRIP_COLS);
  MR_CHECK_ARG((long long)M * H * W < 0x7fffff00LL && M * tiles < 0x7fffff00LL, "mr_strip_crop: M=%d H=%d W=%d exceed one launch",
               M, H, W);
  // A table in pinned host memory is readable on both sides: check it here.  Device memory is the kernel's to check.
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, strips) == hipSuccess && attr.type == hipMemoryTypeHost) {
    const mr_strip_desc* c = (const mr_strip_desc*)strips;
    for (int m = 0; m < M; ++m) {
      MR_CHECK_ARG(c[m].image >= 0 && c[m].image < I, "mr_strip_crop: crop %d names photo %d of %d", m, c[m].image, I);
      MR_CHECK_ARG(c[m].knots >= 2 && c[m].knots <= 18, "mr_strip_crop: crop %d has %d knots", m, c[m].knots);
    }
  } else {
    (void)hipGetLastError();    // an address the runtime does not know is no error of this call
  }
  hipLaunchKernelGGL(strip_crop_kernel, dim3((unsigned)(M * tiles)), dim3(256), 0, stream, src, (const mr_crop_image*)images, I,
                     (const mr_strip_desc*)strips, (int)tiles, H, W, mean0, mean1, mean2, dst);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
