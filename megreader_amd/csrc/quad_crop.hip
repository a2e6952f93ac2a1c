// Quad crops (include/megreader_hip.h: mr_quad_crop): the reference's `ImageCropper.crop` (data/crop_file_dataset.py:105-124)
// rectifies a quadrilateral with warpPerspective, turns a tall crop on its side (`ensure_horizontal`), resizes it with
// cv2.resize and normalises it -- two resamplings on the host per text line.  None of the geometry reads a pixel, so the
// host composes it into one projective map and one resize rule per crop (data/quad_crop.py) and this kernel samples the
// resident uint8 photo ONCE along them, bilinear, writing the normalised recognition batch directly.
// The same byte gather as csrc/db_augment.hip and the form measured fastest there: one thread per canvas pixel, threads
// along u, so a wavefront reads neighbouring source pixels per tap and writes 256 consecutive bytes per plane.  No LDS: the
// photo stays in L2 across the hundreds of crops that read it.
#include "common.h"
#include "../../include/megreader_hip.h"

// Bit-exactness against the numpy restatement (tests/_quad_crop_ref.py): every product and sum of this file is rounded
// on its own; the two float64 divisions are correctly rounded on both sides.
#pragma clang fp contract(off)

namespace mr {

static_assert(sizeof(mr_crop_image) == 24, "mr_crop_image is mirrored by ctypes (data/quad_crop.py)");
static_assert(sizeof(mr_crop_desc) == 112, "mr_crop_desc is mirrored by ctypes (data/quad_crop.py)");

// One photo pixel (3 bytes) as floats; 0 outside the photo.  Only bytes of the photo are ever addressed.
__device__ __forceinline__ void crop_tap(const unsigned char* pix, const mr_crop_image& im, int xx, int yy, float p[3]) {
  p[0] = p[1] = p[2] = 0.f;
  if (xx >= 0 && xx < im.w && yy >= 0 && yy < im.h) {
    const unsigned char* s = pix + (long long)yy * im.pitch + 3 * xx;
    p[0] = (float)s[0];
    p[1] = (float)s[1];
    p[2] = (float)s[2];
  }
}

__global__ __launch_bounds__(256) void quad_crop_kernel(const unsigned char* src, const mr_crop_image* images, int I,
                                                        const mr_crop_desc* crops, int M, int Hd, int Wd, double m0,
                                                        double m1, double m2, float* dst) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;   // M * Hd * Wd < 2^31 (checked by the host)
  if (gid >= (unsigned)M * Hd * Wd) return;
  const unsigned row = gid / Wd;
  const int u = (int)(gid - row * Wd);
  const int m = (int)(row / Hd), v = (int)(row - (unsigned)m * Hd);
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
    // D <= 0 or NaN: behind the map's horizon.  Outside (-1, w) x (-1, h) all four taps are outside the photo; the test
    // also keeps a NaN, an infinity or a huge coordinate away from the int cast.
    if (D > 0.0 && x > -1.0 && x < (double)im.w && y > -1.0 && y < (double)im.h) {
      const unsigned char* pix = src + im.offset;
      const double xf = floor(x), yf = floor(y);
      const float fx = (float)(x - xf), fy = (float)(y - yf);
      const int ix = (int)xf, iy = (int)yf;
      float p00[3], p01[3], p10[3], p11[3];
      crop_tap(pix, im, ix, iy, p00);
      crop_tap(pix, im, ix + 1, iy, p01);
      crop_tap(pix, im, ix, iy + 1, p10);
      crop_tap(pix, im, ix + 1, iy + 1, p11);
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
  float* o = dst + (long long)m * 3 * per + (long long)v * Wd + u;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * per] = (float)((double)val[c] - mean[c]) / 255.f;
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_crop_image(void) { return (int)sizeof(mr_crop_image); }
int mr_sizeof_crop_desc(void) { return (int)sizeof(mr_crop_desc); }

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

}  // extern "C"
