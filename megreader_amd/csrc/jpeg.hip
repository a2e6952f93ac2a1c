// Baseline JPEG decode on the device (include/megreader_hip.h: mr_jpeg_plan, mr_jpeg_decode): the "decode" in front of
// mr_resize_normalize.  The reference decodes every sample on the host (data/unpack_msgpack_data.py:28-35 with PIL,
// data/lmdb_dataset.py:80-88 with cv2.imdecode); a batch of recognition crops is hundreds of independent, tiny bitstreams, so here
// the host reads only the marker segments (csrc/jpeg_plan.h) and the encoded bytes cross PCIe.
//
// Stage A, jpeg_entropy_idct_kernel: ONE WAVEFRONT PER WORK ITEM (an image, or one restart interval of it).  Huffman decoding is
// serial, so the wave acts as one scalar decoder with 64-lane helpers; everything that steers it is wave-uniform (no divergence):
//   * bytes: the wave loads 256 source bytes at a time (one aligned dword per lane), drops the byte after every FF -- inside an
//     item that is a stuffed 00 or a fill FF, the plan guarantees it -- with four ballots and prefix popcounts, and appends the
//     rest to a 1 KiB LDS window; the bit reader takes big-endian words from it into a 64-bit buffer.  Past the item's last byte
//     it reads zeros;
//   * code length in one step: lane l holds the largest code of length l + 1; lanes 0..15 compare the 16-bit peek, one ballot,
//     lowest set bit (T.81 F.2.2.3's loop, all lengths at once).  The symbol offset of that length comes by readlane;
//   * coefficients are dequantised as they are placed, de-zigzagged, into an LDS buffer of 8 blocks (quantiser and zigzag
//     position by readlane from the lane that owns coefficient k);
//   * the inverse DCT runs when 8 blocks are waiting: 64 lanes each own a column (row stride 8, block stride 72 dwords: the 32
//     lanes of a half hit 32 banks), then a row, and store 8 range-limited bytes each into the component plane in the workspace.
//   The coefficient index stops at 63, every loop is bounded by the item's MCU count, block positions come from the MCU number
//   alone: a malformed stream ends as MR_JPEG_CORRUPT in the image's status word (invalid code, DC size > 11, a run past 63, more
//   bits used than the item has), never as an access outside the planes.
//   Items that the split plan took (mr_jpeg_plan_split marks them through `reserved`) are skipped here: csrc/jpeg_split.hip decodes
//   each of them with many lanes into the same planes, between this kernel and Stage B.
// Stage B, jpeg_color_kernel: elementwise over output pixels, chroma upsampling + YCbCr -> RGB, 4 pixels = three aligned dword
// stores per thread over the image's flat h*w*3 bytes (rows have no padding, so alignment follows the flat index, not the row).
//
// Arithmetic (restated in tests/_jpeg_ref.py, which the CPU tests hold against PIL bit for bit): slow-integer IDCT with 13-bit
// constants, descale 11 then 18; the DC-only shortcut of the usual implementations gives the same values as the full
// butterfly (all products of zero), so there is no per-lane branch for it; range limit as the 10-bit masked table; triangle
// upsampling for chroma planes wider than 2 samples, replication otherwise; 16-bit fixed-point colour conversion.
#include <stddef.h>

#include "common.h"
#include "jpeg_idct.h"
#include "jpeg_plan.h"
#include "../../include/megreader_hip.h"

namespace mr {

using jpeg::Image;
using jpeg::Item;
using namespace jpeg_dev;

static_assert(sizeof(Image) == sizeof(mr_jpeg_image) && sizeof(Image) % 8 == 0, "csrc/jpeg_plan.h restates mr_jpeg_image");
static_assert(offsetof(Image, blob_off) == offsetof(mr_jpeg_image, blob_off) &&
              offsetof(Image, plane_off) == offsetof(mr_jpeg_image, plane_off) &&
              offsetof(Image, out_off) == offsetof(mr_jpeg_image, out_off) &&
              offsetof(Image, comp_tq) == offsetof(mr_jpeg_image, comp_tq) &&
              offsetof(Image, quant) == offsetof(mr_jpeg_image, quant) &&
              offsetof(Image, huff_sym) == offsetof(mr_jpeg_image, huff_sym), "csrc/jpeg_plan.h restates mr_jpeg_image");
static_assert(sizeof(Item) == sizeof(mr_jpeg_item) && offsetof(Item, off) == offsetof(mr_jpeg_item, off),
              "csrc/jpeg_plan.h restates mr_jpeg_item");

namespace {

constexpr int WIN_BYTES = 1024;   // unstuffed bytes the LDS window holds

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The byte side and the bit side of one item's stream.  Every member is the same in all lanes.
struct Stream {
  const unsigned char* base;   // the blob buffer
  long long begin, end;        // the item's stuffed bytes [begin, end) inside it
  long long src;               // next source byte, a multiple of 4 (bytes outside [begin, end) are masked)
  int last;                    // the source byte in front of src (0 at the start)
  unsigned char* win;          // LDS window, WIN_BYTES + 4
  int wbytes;                  // unstuffed bytes in the window
  int wpos;                    // next window WORD the bit buffer takes
  long long shifted;           // unstuffed bytes that have left the window
  long long total;             // unstuffed bytes seen so far
  unsigned long long buf;      // bits, first one at the top
  int cnt;                     // valid bits in buf
};

// Move the (at most 3) unread bytes to the front of the window and append source chunks while 256 more bytes fit.
__device__ __forceinline__ void refill(Stream& s, int lane) {
  const int from = s.wpos * 4, tail = s.wbytes - from;
  unsigned char keep = 0;
  if (lane < tail) keep = s.win[from + lane];
  __syncthreads();
  if (lane < tail) s.win[lane] = keep;
  s.shifted += from;
  s.wbytes = tail;
  s.wpos = 0;
  while (s.src < s.end && s.wbytes + 256 <= WIN_BYTES) {
    const long long p = s.src + 4 * lane;
    unsigned w = 0;
    if (p < s.end) w = *(const unsigned*)(s.base + p);   // an aligned dword that overlaps the blob: inside its 16-byte padding
    unsigned prev = __shfl_up(w >> 24, 1, 64);
    if (lane == 0) prev = (unsigned)s.last;
    unsigned b[4];
    bool k[4];
    unsigned long long m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[j] = (w >> (8 * j)) & 255u;
      const bool prev_in = p + j - 1 >= s.begin;   // the byte in front of the item is not part of it
      k[j] = p + j >= s.begin && p + j < s.end && !(prev_in && prev == 255u);
      prev = b[j];
      m[j] = __ballot(k[j]);
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int at = s.wbytes;
#pragma unroll
    for (int j = 0; j < 4; ++j) at += __popcll(m[j] & below);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k[j]) s.win[at] = (unsigned char)b[j];
      at += k[j] ? 1 : 0;
    }
    const int added = __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
    s.last = uni((int)__shfl(w >> 24, 63, 64));
    s.wbytes += added;
    s.total += added;
    s.src += 256;
  }
  if (lane < 4) s.win[s.wbytes + lane] = 0;   // the last word reads as zero bits past the data
  __syncthreads();
}

// At least 32 valid bits (zeros past the end of the item).
__device__ __forceinline__ void fill(Stream& s, int lane) {
  if (s.cnt <= 32) {
    if (s.wpos * 4 + 4 > s.wbytes && s.src < s.end) refill(s, lane);
    unsigned w = 0;
    if (s.wpos * 4 < s.wbytes) w = (unsigned)uni((int)((const unsigned*)s.win)[s.wpos]);
    s.buf |= (unsigned long long)__builtin_bswap32(w) << (32 - s.cnt);
    s.cnt += 32;
    s.wpos += 1;
  }
}

__device__ __forceinline__ int take(Stream& s, int nbits) {   // nbits <= 16, within what fill() left
  const int v = nbits ? (int)(s.buf >> (64 - nbits)) : 0;
  s.buf = nbits ? s.buf << nbits : s.buf;
  s.cnt -= nbits;
  return v;
}

// One Huffman symbol: maxcode / valoff are this lane's entries (lane l: code length l + 1), syms the table's 256 bytes in LDS.
__device__ __forceinline__ int symbol(Stream& s, int lane, int maxcode, int valoff, const unsigned char* syms, bool& bad) {
  fill(s, lane);
  const int peek = (int)(s.buf >> 48);
  const unsigned long long hit = __ballot(lane < 16 && (peek >> (15 - (lane & 15))) <= maxcode);
  if (hit == 0) {   // no length accepts these 16 bits
    bad = true;
    take(s, 16);
    return 0;
  }
  const int l = uni(__ffsll((long long)hit) - 1);
  const int code = take(s, l + 1);
  return uni((int)syms[(code + __builtin_amdgcn_readlane(valoff, l)) & 255]);
}

__device__ __forceinline__ int extend(int v, int nbits) {   // T.81 F.2.2.1
  return nbits && v < (1 << (nbits - 1)) ? v - (1 << nbits) + 1 : v;
}

__global__ __launch_bounds__(64) void jpeg_entropy_idct_kernel(const unsigned char* blobs, const Image* images,
                                                               const Item* items, unsigned char* ws, int* status) {
  __shared__ __attribute__((aligned(16))) unsigned char win[WIN_BYTES + 16];
  __shared__ __attribute__((aligned(16))) int blk[8 * BLK_STRIDE];
  __shared__ __attribute__((aligned(16))) unsigned char syms[4 * 256];
  __shared__ long long slot_dst[8];
  __shared__ int slot_pitch[8];
  const int lane = threadIdx.x;
  const Item it = items[blockIdx.x];
  const Image* im = images + it.image;
  if (it.reserved != 0) return;         // an item of the split plan: csrc/jpeg_split.hip decodes it
  if (im->status != jpeg::OK) return;   // an image the caller re-marked for the host decoder after planning
  const int ncomp = im->ncomp, mcu_w = im->mcu_w;
  // this lane's share of the tables: code-length entries (lanes 0..15), the quantiser and the zigzag position of coefficient `lane`
  int maxcode[4], valoff[4], quant[3];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    maxcode[t] = lane < 16 ? im->huff_maxcode[t * 16 + lane] : -1;
    valoff[t] = lane < 16 ? im->huff_valoff[t * 16 + lane] : 0;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) quant[c] = c < ncomp ? ((const unsigned char*)im->quant)[64 * (im->comp_tq[c] & 3) + lane] : 0;
  const int zigzag = ZIGZAG[lane];
#pragma unroll
  for (int j = 0; j < 4; ++j) ((int*)syms)[lane * 4 + j] = im->huff_sym[lane * 4 + j];

  Stream s;
  s.base = blobs + im->blob_off;
  s.begin = it.off;
  s.end = it.off + it.len;
  s.src = it.off & ~3LL;
  s.last = 0;
  s.win = win;
  s.wbytes = 0, s.wpos = 0, s.shifted = 0, s.total = 0, s.buf = 0, s.cnt = 0;
  if (lane < 4) win[lane] = 0;
  __syncthreads();

  bool bad = false;
  int pred[3] = {0, 0, 0};
  int ns = 0;
  for (int m = it.mcu0; m < it.mcu0 + it.nmcu; ++m) {
    const int my = m / mcu_w, mx = m - my * mcu_w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= ncomp) break;
      const int hs = c == 0 ? im->hs : 1, vs = c == 0 ? im->vs : 1;
      const int td = im->comp_td[c] & 1, ta = 2 + (im->comp_ta[c] & 1);
      const int pitch = im->plane_pitch[c];
      for (int sub = 0; sub < hs * vs; ++sub) {
        const int by = sub / hs, bx = sub - by * hs;
        int* out = blk + ns * BLK_STRIDE;
        out[lane] = 0;
        if (lane == 0) {
          slot_dst[ns] = im->plane_off[c] + (long long)(my * vs + by) * 8 * pitch + (mx * hs + bx) * 8;
          slot_pitch[ns] = pitch;
        }
        int size = symbol(s, lane, td ? maxcode[1] : maxcode[0], td ? valoff[1] : valoff[0], syms + 256 * td, bad);
        if (size > 11) bad = true;   // (a symbol is a byte: size <= 255; the mask keeps take() within 16 bits)
        size &= 15;
        pred[c] += extend(take(s, size), size);
        if (lane == 0) out[0] = pred[c] * __builtin_amdgcn_readlane(quant[c], 0);
        for (int k = 1; k < 64;) {
          const int rs = symbol(s, lane, ta == 3 ? maxcode[3] : maxcode[2], ta == 3 ? valoff[3] : valoff[2], syms + 256 * ta, bad);
          const int run = rs >> 4, nbits = rs & 15;
          if (nbits == 0) {
            if (run != 15) break;   // end of block
            k += 16;
            continue;
          }
          k += run;
          if (k > 63) {
            bad = true;
            break;
          }
          const int coef = extend(take(s, nbits), nbits) * __builtin_amdgcn_readlane(quant[c], k);
          const int at = __builtin_amdgcn_readlane(zigzag, k);
          if (lane == 0) out[at] = coef;
          ++k;
        }
        if (++ns == 8) {
          flush_blocks(blk, slot_dst, slot_pitch, ns, ws, lane);
          ns = 0;
        }
      }
    }
  }
  if (ns) flush_blocks(blk, slot_dst, slot_pitch, ns, ws, lane);
  // more bits used than the item has: it ended before its last MCU
  const long long used = (s.shifted + 4LL * s.wpos) * 8 - s.cnt;
  if (s.src >= s.end && used > s.total * 8) bad = true;   // (while source bytes remain, fill() refills before it runs dry)
  if (bad && lane == 0) atomicMax(status + it.image, (int)jpeg::CORRUPT);
}

__global__ __launch_bounds__(256) void jpeg_status_kernel(const Image* images, int n, int* status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) status[i] = images[i].status;
}

// One chroma sample at full-size position (x, y): plane P of real size cw x ch (pitch: its padded width).
__device__ __forceinline__ int chroma_at(const unsigned char* P, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return P[(long long)y * pitch + x];
  const int cx = x >> 1;
  if (vs == 1) {
    const unsigned char* row = P + (long long)y * pitch;
    const int t = row[cx];
    if (cw <= 2) return t;
    if (x & 1) return cx == cw - 1 ? t : (3 * t + row[cx + 1] + 2) >> 2;
    return cx == 0 ? t : (3 * t + row[cx - 1] + 1) >> 2;
  }
  const int cy = y >> 1;
  if (cw <= 2) return P[(long long)cy * pitch + cx];
  const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);   // the real plane's edge row, replicated
  const unsigned char* near = P + (long long)cy * pitch;
  const unsigned char* far = P + (long long)fy * pitch;
  const int t = 3 * near[cx] + far[cx];
  if (x & 1) return cx == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

// The three output bytes of pixel p (row-major) in the low 24 bits, first byte lowest.
__device__ __forceinline__ unsigned pixel(const Image& im, const unsigned char* ws, unsigned p, int rgb) {
  const int y = (int)(p / (unsigned)im.w), x = (int)(p - (unsigned)y * im.w);
  const int Y = ws[im.plane_off[0] + (long long)y * im.plane_pitch[0] + x];
  if (im.ncomp == 1) return (unsigned)Y * 0x010101u;
  const int cw = (im.w + im.hs - 1) / im.hs, ch = (im.h + im.vs - 1) / im.vs;
  const int cb = chroma_at(ws + im.plane_off[1], im.plane_pitch[1], cw, ch, im.hs, im.vs, x, y) - 128;
  const int cr = chroma_at(ws + im.plane_off[2], im.plane_pitch[2], cw, ch, im.hs, im.vs, x, y) - 128;
  const unsigned r = (unsigned)min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
  const unsigned g = (unsigned)min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
  const unsigned b = (unsigned)min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
  return rgb ? r | g << 8 | b << 16 : b | g << 8 | r << 16;
}

// grid (image, 8): the blocks of an image stride over its groups of 4 pixels (12 bytes: three dword stores at a flat offset that is
// a multiple of 4 from the 16-byte aligned region); the last h*w % 4 pixels are written byte by byte, so no store leaves the region.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const Image* images, const unsigned char* ws, unsigned char* out,
                                                         int rgb) {
  const Image& im = images[blockIdx.x];
  if (im.status != jpeg::OK) return;
  const unsigned npix = (unsigned)im.h * (unsigned)im.w, groups = npix / 4;
  unsigned char* dst = out + im.out_off;
  for (unsigned g = blockIdx.y * 256u + threadIdx.x; g < groups; g += gridDim.y * 256u) {
    const unsigned p0 = pixel(im, ws, 4 * g, rgb), p1 = pixel(im, ws, 4 * g + 1, rgb);
    const unsigned p2 = pixel(im, ws, 4 * g + 2, rgb), p3 = pixel(im, ws, 4 * g + 3, rgb);
    unsigned* o = (unsigned*)(dst + 12ull * g);
    o[0] = p0 | p1 << 24;
    o[1] = p1 >> 8 | p2 << 16;
    o[2] = p2 >> 16 | p3 << 8;
  }
  if (blockIdx.y == 0 && threadIdx.x < npix - 4 * groups) {
    const unsigned p = 4 * groups + threadIdx.x, v = pixel(im, ws, p, rgb);
    dst[3ull * p] = (unsigned char)v;
    dst[3ull * p + 1] = (unsigned char)(v >> 8);
    dst[3ull * p + 2] = (unsigned char)(v >> 16);
  }
}

}  // namespace

// csrc/jpeg_split.hip: the stages that decode the items of the split plan
int jpeg_split_stages(const unsigned char* blobs, const Image* images, const Item* items, const jpeg::Split* host,
                      const jpeg::Split* dev, int n_splits, unsigned char* ws, int* status, hipStream_t stream);

}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_jpeg_image(void) { return (int)sizeof(mr_jpeg_image); }
int mr_sizeof_jpeg_item(void) { return (int)sizeof(mr_jpeg_item); }

int mr_jpeg_plan(int n, const void* const* blobs, const long long* lens, mr_jpeg_image* images, mr_jpeg_item* items,
                 long long max_items, long long* totals) {
  MR_CHECK_ARG(n >= 0 && max_items >= 0 && totals != nullptr, "mr_jpeg_plan: bad arguments n=%d max_items=%lld", n, max_items);
  MR_CHECK_ARG(n == 0 || (blobs != nullptr && lens != nullptr && images != nullptr), "mr_jpeg_plan: null pointer");
  MR_CHECK_ARG(max_items == 0 || items != nullptr, "mr_jpeg_plan: null item list");
  jpeg::Totals t;
  jpeg::plan(n, blobs, lens, (Image*)images, (Item*)items, max_items, &t);
  totals[0] = t.n_items, totals[1] = t.blob_bytes, totals[2] = t.workspace_bytes, totals[3] = t.out_bytes;
  return MR_OK;
}

int mr_jpeg_decode_split(const void* blobs_dev, const void* plan_dev, int n_images, int n_items, const mr_jpeg_split* splits_host,
                         const void* splits_dev, int n_splits, void* workspace, void* out, int* status, int rgb,
                         hipStream_t stream) {
  MR_CHECK_ARG(n_images >= 0 && n_items >= 0 && n_splits >= 0 && n_splits <= 65535 && n_splits <= n_items,
               "mr_jpeg_decode: bad counts n_images=%d n_items=%d n_splits=%d", n_images, n_items, n_splits);
  if (n_images == 0) return MR_OK;
  MR_CHECK_ARG(plan_dev != nullptr && status != nullptr, "mr_jpeg_decode: null pointer");
  MR_CHECK_ARG(((uintptr_t)blobs_dev & 15) == 0 && ((uintptr_t)plan_dev & 15) == 0 && ((uintptr_t)workspace & 15) == 0 &&
                   ((uintptr_t)out & 15) == 0 && ((uintptr_t)splits_dev & 15) == 0,
               "mr_jpeg_decode: the blob buffer, the plan, the split table, the workspace and the output must be 16-byte aligned");
  MR_CHECK_ARG(n_splits == 0 || (splits_host != nullptr && splits_dev != nullptr), "mr_jpeg_decode_split: null split table");
  const Image* images = (const Image*)plan_dev;
  const Item* items = (const Item*)(images + n_images);
  hipLaunchKernelGGL(jpeg_status_kernel, dim3(cdiv(n_images, 256)), dim3(256), 0, stream, images, n_images, status);
  MR_CHECK_LAUNCH();
  if (n_items == 0) return MR_OK;   // nothing the device can decode
  MR_CHECK_ARG(blobs_dev != nullptr && workspace != nullptr && out != nullptr, "mr_jpeg_decode: null pointer");
  hipLaunchKernelGGL(jpeg_entropy_idct_kernel, dim3(n_items), dim3(64), 0, stream, (const unsigned char*)blobs_dev, images, items,
                     (unsigned char*)workspace, status);
  MR_CHECK_LAUNCH();
  if (n_splits > 0) {
    const int rc = jpeg_split_stages((const unsigned char*)blobs_dev, images, items, (const jpeg::Split*)splits_host,
                                     (const jpeg::Split*)splits_dev, n_splits, (unsigned char*)workspace, status, stream);
    if (rc != MR_OK) return rc;
  }
  hipLaunchKernelGGL(jpeg_color_kernel, dim3(n_images, 8), dim3(256), 0, stream, images, (const unsigned char*)workspace,
                     (unsigned char*)out, rgb);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_jpeg_decode(const void* blobs_dev, const void* plan_dev, int n_images, int n_items, void* workspace, void* out,
                   int* status, int rgb, hipStream_t stream) {
  return mr_jpeg_decode_split(blobs_dev, plan_dev, n_images, n_items, nullptr, nullptr, 0, workspace, out, status, rgb, stream);
}

}  // extern "C"
