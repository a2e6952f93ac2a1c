// The inverse-DCT half of the JPEG decoder, shared by the single-wave path (csrc/jpeg.hip) and the split path
// (csrc/jpeg_split.hip): zigzag order, the slow-integer 8-point pass, the range limit and the 8-blocks-per-wave flush.  The
// arithmetic is restated in tests/_jpeg_ref.py; both paths must produce the same bytes, so there is one copy of it.
#pragma once
#include "common.h"

namespace mr {
namespace jpeg_dev {

constexpr int BLK_STRIDE = 72;    // dwords between the 8 waiting blocks

static __device__ const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One pass of the slow-integer inverse DCT over 8 values.
__device__ __forceinline__ void idct8(const int v[8], int out[8], int shift) {
  int z2 = v[2], z3 = v[6];
  int z1 = (z2 + z3) * 4433;
  const int t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
  const int t0 = (v[0] + v[4]) << 13, t1 = (v[0] - v[4]) << 13;
  const int e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
  int o0 = v[7], o1 = v[5], o2 = v[3], o3 = v[1];
  z1 = o0 + o3, z2 = o1 + o2, z3 = o0 + o2;
  int z4 = o1 + o3;
  const int z5 = (z3 + z4) * 9633;
  o0 *= 2446, o1 *= 16819, o2 *= 25172, o3 *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
  const int r = 1 << (shift - 1);
  out[0] = (e0 + o3 + r) >> shift, out[7] = (e0 - o3 + r) >> shift;
  out[1] = (e1 + o2 + r) >> shift, out[6] = (e1 - o2 + r) >> shift;
  out[2] = (e2 + o1 + r) >> shift, out[5] = (e2 - o1 + r) >> shift;
  out[3] = (e3 + o0 + r) >> shift, out[4] = (e3 - o0 + r) >> shift;
}

// The range-limit table of the IDCT output, indexed by the low 10 bits: as a signed 10-bit number x it holds clamp(x + 128).
__device__ __forceinline__ unsigned range_limit(int v) {
  const int x = ((v & 1023) ^ 512) - 512;
  return (unsigned)min(max(x + 128, 0), 255);
}

// Inverse DCT of the `ns` waiting blocks: lane = (block, column), then (block, row); 8 bytes per lane to dst[block] + row * pitch.
__device__ __forceinline__ void flush_blocks(int* blk, const long long* dst, const int* pitch, int ns, unsigned char* ws,
                                             int lane) {
  const int b = lane >> 3, c = lane & 7;
  __syncthreads();
  if (b < ns) {
    int v[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = blk[b * BLK_STRIDE + r * 8 + c];
    idct8(v, o, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) blk[b * BLK_STRIDE + r * 8 + c] = o[r];
  }
  __syncthreads();
  if (b < ns) {
    int v[8], o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = blk[b * BLK_STRIDE + c * 8 + j];
    idct8(v, o, 18);
    uint2 px;
    px.x = range_limit(o[0]) | range_limit(o[1]) << 8 | range_limit(o[2]) << 16 | range_limit(o[3]) << 24;
    px.y = range_limit(o[4]) | range_limit(o[5]) << 8 | range_limit(o[6]) << 16 | range_limit(o[7]) << 24;
    *(uint2*)(ws + dst[b] + (long long)c * pitch[b]) = px;   // planes are 16-byte aligned with pitches that are multiples of 8
  }
  __syncthreads();
}

}  // namespace jpeg_dev
}  // namespace mr
