// Tiled multi-scale detection (include/megreader_hip.h: mr_tile_sample, mr_tile_stitch).  A photo larger than the detector's
// input is resized to a canvas at its own scale, the canvas is covered by overlapping detector-sized tiles, and the tiles'
// probability maps are fused into one map per photo before the boxes are read.  The host plans canvases and tiles from shapes
// only (megreader_amd/data/detection_tiles.py); the two passes here are the pixel work on both sides of the detector.
//
// mr_tile_sample is the byte gather of mr_resize_normalize with a window: one thread per tile pixel, threads along u, the form
// measured fastest for the byte gathers of image_sample.hip (CHANGELOG.md, "Fused DB detection augmentation": 2 and 4 pixels
// per thread spread one load instruction over 2 and 4 times as many cache lines).  A wavefront reads neighbouring source pixels
// per tap and writes 256 consecutive bytes per plane.  No LDS: the photos stay in L2 / the Infinity Cache across the tiles and
// levels that read them, and the overlap of neighbouring tiles (2 * halo of every tile side) is re-read from there.
//
// mr_tile_stitch is a gather as well: one thread per pixel of the fused map, threads along X, each pixel written once.  The base
// level is a 4-byte load and a 4-byte store per lane, 256 contiguous bytes per wavefront wherever it does not cross a core border;
// every other level adds four taps whose addresses follow the level's own scale, so there is no width that keeps a 16-byte
// access aligned across levels, and an owner change inside a 4-pixel run would need a scalar path beside the vector one.  The
// pass moves 4 bytes per map pixel and level against a detector that computes thousands of flops for the same pixel.
#include "common.h"
#include "../../include/megreader_hip.h"
#include "image_sample.h"

// Bit-exactness against the numpy restatements (tests/_det_tiles_ref.py) and against resize_normalize_kernel: every product and
// sum of this file is rounded on its own.
#pragma clang fp contract(off)

namespace mr {

static_assert(sizeof(mr_tile_desc) == 40, "mr_tile_desc is mirrored by ctypes (data/detection_tiles.py)");
static_assert(sizeof(mr_stitch_level) == 40, "mr_stitch_level is mirrored by ctypes (data/detection_tiles.py)");
static_assert(sizeof(mr_stitch_photo) == 32, "mr_stitch_photo is mirrored by ctypes (data/detection_tiles.py)");

// Tile pixel (u, v) of tile t is canvas pixel (x0 + u, y0 + v); inside the canvas the arithmetic is resize_normalize_kernel's
// (image_sample.hip) statement for statement, outside it the three planes get 0.0f.
__global__ __launch_bounds__(256) void tile_sample_kernel(const unsigned char* src, const mr_crop_image* images, int I,
                                                          const mr_tile_desc* tiles, int T, int th, int tw, double m0,
                                                          double m1, double m2, float* dst) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;   // T * th * tw * 3 < 2^31 (checked by the host)
  if (gid >= (unsigned)T * th * tw) return;
  const unsigned row = gid / tw;
  const int u = (int)(gid - row * tw);
  const int t = (int)(row / th);
  const int v = (int)(row - (unsigned)t * th);
  const mr_tile_desc d = tiles[t];
  const int x = d.x0 + u, y = d.y0 + v;
  if (d.image >= 0 && d.image < I && x >= 0 && x < d.wc && y >= 0 && y < d.hc) {
    const mr_crop_image im = images[d.image];
    const unsigned char* s = src + im.offset;
    float val[3] = {0.f, 0.f, 0.f};
    if (im.h == d.hc && im.w == d.wc) {   // cv2.resize returns a copy when the size already matches
#pragma unroll
      for (int c = 0; c < 3; ++c) val[c] = (float)s[(long long)y * im.pitch + 3 * x + c];
    } else if (im.h > 0 && im.w > 0) {
      float fx = (float)((x + 0.5) * d.scale_x - 0.5);   // rounded product, then rounded sum (contraction is off)
      int sx = (int)floorf(fx);
      fx -= sx;
      if (sx < 0) { sx = 0; fx = 0.f; }
      if (sx >= im.w - 1) { sx = im.w - 1; fx = 0.f; }
      float fy = (float)((y + 0.5) * d.scale_y - 0.5);
      int sy = (int)floorf(fy);
      fy -= sy;
      if (sy < 0) { sy = 0; fy = 0.f; }
      if (sy >= im.h - 1) { sy = im.h - 1; fy = 0.f; }
      const int sx1 = min(sx + 1, im.w - 1), sy1 = min(sy + 1, im.h - 1);
      const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
      const unsigned char* r0 = s + (long long)sy * im.pitch;
      const unsigned char* r1 = s + (long long)sy1 * im.pitch;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = (float)r0[3 * sx + c] * a0 + (float)r0[3 * sx1 + c] * a1;
        const float bot = (float)r1[3 * sx + c] * a0 + (float)r1[3 * sx1 + c] * a1;
        val[c] = top * b0 + bot * b1;
      }
    }
    store_normalized(dst, t, v, u, th, tw, val, m0, m1, m2);
  } else {
    const long long per = (long long)th * tw;
    float* o = dst + (long long)t * 3 * per + (long long)v * tw + u;
    o[0] = 0.f;
    o[per] = 0.f;
    o[2 * per] = 0.f;
  }
}

// The 1-D cover's owner of canvas coordinate p: tiles of side t, halo h, stride s = t - 2h, K of them.
__device__ __forceinline__ int cover_owner(int p, int t, int h, int s, int K) {
  return p < t - h ? 0 : min(K - 1, (p - h) / s);
}

struct StitchGeom {
  int T, th, tw, hy, hx, sy, sx;
};

// maps[tile that owns (x, y) of level lv][y - its origin][x - its origin], or 0 where the table does not lead inside maps.
template <typename M>
__device__ __forceinline__ float tile_value(const M* maps, const StitchGeom& g, const mr_stitch_level& lv, int x, int y) {
  const int ky = cover_owner(y, g.th, g.hy, g.sy, lv.ky), kx = cover_owner(x, g.tw, g.hx, g.sx, lv.kx);
  const int ly = y - ky * g.sy, lx = x - kx * g.sx;
  const long long t = (long long)lv.first + (long long)ky * lv.kx + kx;
  if (t < 0 || t >= g.T || (unsigned)ly >= (unsigned)g.th || (unsigned)lx >= (unsigned)g.tw) return 0.f;
  return to_f32(maps[((int)t * g.th + ly) * g.tw + lx]);   // T * th * tw < 2^31 (checked by the host)
}

// The sampling point of one axis of a level that is not the base: i0, i1 and the f32 fraction.
__device__ __forceinline__ void level_axis(int P, int side, double ratio, int& i0, int& i1, float& f) {
  double x = ((double)P + 0.5) * ratio - 0.5;
  x = fmin(fmax(x, 0.0), (double)(side - 1));
  const double xf = floor(x);
  f = (float)(x - xf);
  i0 = (int)xf;
  i1 = min(i0 + 1, side - 1);
}

template <typename M>
__global__ __launch_bounds__(256) void tile_stitch_kernel(const M* maps, StitchGeom g, const mr_stitch_level* levels, int L,
                                                          const mr_stitch_photo* photos, int fuse, float* out,
                                                          long long out_elems) {
  const mr_stitch_photo ph = photos[blockIdx.y];
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;   // max_pixels < 2^31 (checked by the host)
  if (ph.hb < 1 || ph.wb < 1 || ph.levels < 1 || ph.base < 0 || ph.base >= ph.levels || ph.first_level < 0 ||
      (long long)ph.first_level + ph.levels > L)
    return;
  const long long per = (long long)ph.hb * ph.wb;
  if (gid >= per || ph.offset < 0 || ph.offset > out_elems - per) return;
  const int Y = (int)(gid / (unsigned)ph.wb), X = (int)(gid - (unsigned)Y * (unsigned)ph.wb);
  float acc = 0.f;
  for (int l = 0; l < ph.levels; ++l) {
    const mr_stitch_level lv = levels[ph.first_level + l];
    float val = 0.f;
    if (l == ph.base) {
      val = tile_value(maps, g, lv, X, Y);
    } else if (lv.hc > 0 && lv.wc > 0) {
      int ix, ix1, iy, iy1;
      float fx, fy;
      level_axis(X, lv.wc, lv.ratio_x, ix, ix1, fx);
      level_axis(Y, lv.hc, lv.ratio_y, iy, iy1, fy);
      const float p00 = tile_value(maps, g, lv, ix, iy), p01 = tile_value(maps, g, lv, ix1, iy);
      const float p10 = tile_value(maps, g, lv, ix, iy1), p11 = tile_value(maps, g, lv, ix1, iy1);
      const float gx = 1.f - fx, gy = 1.f - fy;
      const float top = p00 * gx + p01 * fx;
      const float bot = p10 * gx + p11 * fx;
      val = top * gy + bot * fy;
    }
    acc = l == 0 ? val : (fuse == MR_TILE_FUSE_MAX ? fmaxf(acc, val) : acc + val);
  }
  if (fuse == MR_TILE_FUSE_MEAN) acc = acc / (float)ph.levels;
  out[ph.offset + gid] = acc;
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_tile_desc(void) { return (int)sizeof(mr_tile_desc); }
int mr_sizeof_stitch_level(void) { return (int)sizeof(mr_stitch_level); }
int mr_sizeof_stitch_photo(void) { return (int)sizeof(mr_stitch_photo); }

int mr_tile_sample(const unsigned char* src, const void* images, int I, const void* tiles, int T, int th, int tw,
                   double mean0, double mean1, double mean2, float* dst, hipStream_t stream) {
  MR_CHECK_ARG(I >= 0 && T >= 0 && th > 0 && tw > 0, "mr_tile_sample: bad shape I=%d T=%d th=%d tw=%d", I, T, th, tw);
  if (T == 0) return MR_OK;
  MR_CHECK_ARG(src != nullptr && images != nullptr && tiles != nullptr && dst != nullptr, "mr_tile_sample: null pointer");
  const long long total = (long long)T * th * tw;
  MR_CHECK_ARG(total * 3 < 0x7fffff00LL, "mr_tile_sample: T=%d th=%d tw=%d exceed one launch", T, th, tw);
  hipLaunchKernelGGL(tile_sample_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, stream, src,
                     (const mr_crop_image*)images, I, (const mr_tile_desc*)tiles, T, th, tw, mean0, mean1, mean2, dst);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_tile_stitch(int dtype, const void* maps, int T, int th, int tw, int halo_y, int halo_x, const void* levels, int L,
                   const void* photos, int P, long long max_pixels, int fuse, float* out, long long out_elems,
                   hipStream_t stream) {
  MR_CHECK_ARG(T >= 0 && L >= 0 && P >= 0 && th > 0 && tw > 0, "mr_tile_stitch: bad shape T=%d L=%d P=%d th=%d tw=%d", T, L, P,
               th, tw);
  MR_CHECK_ARG(halo_y >= 0 && halo_x >= 0 && th > 2 * halo_y && tw > 2 * halo_x,
               "mr_tile_stitch: tiles %d x %d do not exceed twice the halo (%d, %d)", th, tw, halo_y, halo_x);
  MR_CHECK_ARG(fuse == MR_TILE_FUSE_MAX || fuse == MR_TILE_FUSE_MEAN, "mr_tile_stitch: fuse %d is neither 0 (max) nor 1 (mean)",
               fuse);
  if (dtype != MR_F32 && dtype != MR_BF16) {
    set_error("mr_tile_stitch: dtype %d is neither f32 nor bf16", dtype);
    return MR_ERR_DTYPE;
  }
  if (P == 0) return MR_OK;
  MR_CHECK_ARG((maps != nullptr || T == 0) && levels != nullptr && photos != nullptr && out != nullptr,
               "mr_tile_stitch: null pointer");
  MR_CHECK_ARG((long long)T * th * tw < 0x7fffff00LL, "mr_tile_stitch: T=%d th=%d tw=%d exceed 2^31 elements", T, th, tw);
  MR_CHECK_ARG(max_pixels >= 1 && max_pixels < 0x7fffff00LL && out_elems >= 0 && P <= 65535,
               "mr_tile_stitch: max_pixels=%lld out_elems=%lld P=%d out of range", max_pixels, out_elems, P);
  const StitchGeom g = {T, th, tw, halo_y, halo_x, th - 2 * halo_y, tw - 2 * halo_x};
  const dim3 grid((unsigned)cdivll(max_pixels, 256), (unsigned)P);
  if (dtype == MR_F32)
    hipLaunchKernelGGL(tile_stitch_kernel<float>, grid, dim3(256), 0, stream, (const float*)maps, g,
                       (const mr_stitch_level*)levels, L, (const mr_stitch_photo*)photos, fuse, out, out_elems);
  else
    hipLaunchKernelGGL(tile_stitch_kernel<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)maps, g,
                       (const mr_stitch_level*)levels, L, (const mr_stitch_photo*)photos, fuse, out, out_elems);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
