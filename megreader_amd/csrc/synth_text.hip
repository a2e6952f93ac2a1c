// Synthetic text (include/megreader_hip.h: mr_synth_render): labelled word crops and scenes rendered where they are consumed.
// The recognition configurations train on Synth90k and SynthText, which are rendered text themselves; this kernel renders words
// from glyph atlases along projective maps the host plans (data/synth_text.py), so a training run, a test or a benchmark needs no
// dataset on disk.
//
// One workgroup of 256 threads renders one MR_SYNTH_TILE_H x MR_SYNTH_TILE_W (16 x 64) tile of one canvas:
//   1. wave 0 culls the canvas's items (at most 32) by their boxes against the tile and its blur halo: one ballot, the kept items
//      keep their table order;
//   2. the kept items' maps and colours, and the prefix sums of their glyphs' advance boxes, go to LDS (32 threads per item load
//      the (x0, w) pairs, one thread per item adds them up);
//   3. the composite -- background, then shadow and foreground of every kept item whose box holds the pixel -- is evaluated ONCE
//      per pixel of the tile and its halo of 2 (20 x 68 cells, clamped to the canvas as the blur clamps its taps) into LDS.  A tap
//      of the virtual line image finds its glyph with a 5-step binary search over the 33 prefix sums in LDS and reads one atlas
//      byte; the four taps and the blend are bilinear3 of image_sample.h, the crop kernels' core;
//   4. the blur runs from LDS: a horizontal pass over the 20 rows into a second LDS array, then the vertical pass per pixel;
//   5. noise, quantisation, the normalising store of the f32 planes (threads along x: 256 consecutive bytes per wave and plane),
//      and the three bytes per pixel into an LDS row buffer;
//   6. the uint8 rows leave as whole aligned dwords along the canvas row (pitch W*3; alignment follows the address, the bytes in
//      front of the first and behind the last whole dword of the tile's row segment are stored singly), as jpeg.hip's colour pass.
// LDS: 16 KB composite + 15 KB row pass + 3 KB bytes + 13 KB item tables = 47 KB, three workgroups per CU.  The strides of the
// float arrays are 3 dwords per pixel along x: odd, so the 32 lanes of a half wave fall on 32 banks.
//
// Nothing the tables hold can make the kernel read outside the atlases, the photos or the tables themselves, or loop without
// bound: item counts and glyph counts are clamped to their limits, table indices are tested against F, G and I, a glyph pair
// that does not lie inside its atlas counts as "no glyph", and an atlas byte is addressed only for 0 <= row < gh, 0 <= column < aw.
#include "common.h"
#include "../../include/megreader_hip.h"
#include "image_sample.h"

#include <limits.h>

// Bit-exactness against the numpy restatement (tests/_synth_text_ref.py): every product and sum is rounded on its own.
#pragma clang fp contract(off)

namespace mr {

static_assert(sizeof(mr_synth_font) == 32, "mr_synth_font is mirrored by ctypes (data/synth_text.py)");
static_assert(sizeof(mr_synth_item) == 280, "mr_synth_item is mirrored by ctypes (data/synth_text.py)");
static_assert(sizeof(mr_synth_canvas) == 88, "mr_synth_canvas is mirrored by ctypes (data/synth_text.py)");
static_assert(MR_SYNTH_MAX_ITEMS == 32 && MR_SYNTH_MAX_GLYPHS == 32, "one lane per item, one per glyph; 5-step search");

namespace synth {

constexpr int TH = MR_SYNTH_TILE_H, TW = MR_SYNTH_TILE_W, HALO = 2;
constexpr int CH = TH + 2 * HALO, CW = TW + 2 * HALO;
constexpr int MAXI = MR_SYNTH_MAX_ITEMS, MAXG = MR_SYNTH_MAX_GLYPHS;

// A kept item as the pixel loop reads it.
struct ItemL {
  double h[9];
  double sdx, sdy;
  float fg[3], sh[3];
  float sa;
  int x0, x1, y0, y1;
  int lw, gh, aw, pitch;        // lw: the line's width, 0 for an item that contributes nothing
  long long atlas_off;
};

// cov(u, v) of include/megreader_hip.h: the bilinear sample of the item's virtual line image over 255.
__device__ __forceinline__ float coverage(const ItemL& it, const int* start, const int* delta, const unsigned char* base,
                                          bool ok, double u, double v) {
  float val[3] = {0.f, 0.f, 0.f};
  bilinear3(ok, u, v, it.lw, it.gh, [&](int xx, int yy, float p[3]) {
    p[0] = p[1] = p[2] = 0.f;
    if (xx >= 0 && xx < it.lw && yy >= 0 && yy < it.gh) {
      int g = 0;                                        // the last g in [0, 32) with start[g] <= xx: start[g + 1] > xx
#pragma unroll
      for (int step = MAXG / 2; step > 0; step >>= 1)
        if (start[g + step] <= xx) g += step;
      const int col = delta[g] + xx;                    // x0[g] + xx - start[g], inside the glyph's box, which is inside the atlas
      if (col >= 0 && col < it.aw) p[0] = (float)base[it.atlas_off + (long long)yy * it.pitch + col];
    }
  }, val);
  return val[0] / 255.f;
}

__device__ __forceinline__ unsigned lowbias32(unsigned r) {
  r ^= r >> 16;
  r *= 0x7FEB352Du;
  r ^= r >> 15;
  r *= 0x846CA68Bu;
  r ^= r >> 16;
  return r;
}

__global__ __launch_bounds__(256) void synth_render_kernel(const unsigned char* base, const mr_synth_font* fonts, int F,
                                                           const int* glyphs, int G, const mr_synth_item* items, int I,
                                                           const mr_synth_canvas* canvases, int H, int W, int tiles_x,
                                                           int tiles_y, double m0, double m1, double m2,
                                                           unsigned char* out_u8, float* out_f32) {
  __shared__ ItemL s_item[MAXI];
  __shared__ int s_start[MAXI][MAXG + 1];
  __shared__ int s_delta[MAXI][MAXG];
  __shared__ int s_list[MAXI];
  __shared__ int s_nkept;
  __shared__ float s_comp[CH * CW * 3];
  __shared__ float s_row[CH * TW * 3];
  __shared__ __attribute__((aligned(4))) unsigned char s_q[TH * TW * 3];

  const int tid = threadIdx.x;
  const unsigned per = (unsigned)tiles_x * (unsigned)tiles_y;
  const int n = (int)(blockIdx.x / per);
  const unsigned t = blockIdx.x - (unsigned)n * per;
  const int ty0 = (int)(t / (unsigned)tiles_x) * TH, tx0 = (int)(t % (unsigned)tiles_x) * TW;
  const mr_synth_canvas cv = canvases[n];
  const bool blur = cv.blur != 0;

  // 1. cull
  if (tid < 64) {
    const int cnt = min(max(cv.n_items, 0), MAXI);
    const long long idx = (long long)cv.first_item + tid;
    bool hit = false;
    if (tid < cnt && idx >= 0 && idx < I) {
      const mr_synth_item* it = items + idx;
      const int halo = blur ? HALO : 0;
      const int rx0 = max(tx0 - halo, 0), rx1 = min(tx0 + TW + halo, W);
      const int ry0 = max(ty0 - halo, 0), ry1 = min(ty0 + TH + halo, H);
      hit = it->canvas == n && it->x0 < rx1 && it->x1 > rx0 && it->y0 < ry1 && it->y1 > ry0;
    }
    const unsigned long long mask = __ballot(hit);
    if (hit) s_list[__popcll(mask & ((1ull << tid) - 1ull))] = (int)idx;
    if (tid == 0) s_nkept = __popcll(mask);
  }
  __syncthreads();
  const int nkept = s_nkept;

  // 2. the kept items' tables
  for (int s = tid / MAXG; s < nkept; s += 256 / MAXG) {
    const int g = tid % MAXG;
    const mr_synth_item* it = items + s_list[s];
    const bool fok = it->font >= 0 && it->font < F && it->n_glyphs >= 0 && it->n_glyphs <= MAXG;
    mr_synth_font f = {};
    if (fok) f = fonts[it->font];
    const bool ok = fok && f.gh >= 1 && f.aw >= 1;
    int x0 = 0, w = 0;
    if (ok && g < it->n_glyphs) {
      const int id = it->glyph[g];
      const long long pi = (long long)f.glyph_first + id;
      if (id >= 0 && id < f.n_classes && pi >= 0 && pi < G) {
        const int gx0 = glyphs[2 * pi], gw = glyphs[2 * pi + 1];
        if (gx0 >= 0 && gw > 0 && gw <= MR_SYNTH_MAX_GLYPH_W && (long long)gx0 + gw <= f.aw) {
          x0 = gx0;
          w = gw;
        }
      }
    }
    s_start[s][g + 1] = w;
    s_delta[s][g] = x0;
    if (g == 0) {
      ItemL& L = s_item[s];
#pragma unroll
      for (int k = 0; k < 9; ++k) L.h[k] = it->h[k];
      L.sdx = it->shadow_dx;
      L.sdy = it->shadow_dy;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        L.fg[c] = it->fg[c];
        L.sh[c] = it->shadow[c];
      }
      L.sa = it->shadow_alpha;
      L.x0 = it->x0; L.x1 = it->x1; L.y0 = it->y0; L.y1 = it->y1;
      L.gh = ok ? f.gh : 0;
      L.aw = f.aw;
      L.pitch = f.pitch;
      L.atlas_off = f.atlas_off;
    }
  }
  __syncthreads();
  if (tid < nkept) {
    int acc = 0;
    s_start[tid][0] = 0;
    for (int g = 0; g < MAXG; ++g) {
      const int w = s_start[tid][g + 1];
      s_delta[tid][g] -= acc;
      acc += w;
      s_start[tid][g + 1] = acc;
    }
    s_item[tid].lw = s_item[tid].gh >= 1 ? acc : 0;
  }
  __syncthreads();

  // 3. the composite, once per cell of the tile and its halo (without blur: of the tile)
  for (int cell = tid; cell < CH * CW; cell += 256) {
    const int cy = cell / CW, cx = cell - cy * CW;
    if (!blur && (cy < HALO || cy >= HALO + TH || cx < HALO || cx >= HALO + TW)) continue;
    const int x = min(max(tx0 - HALO + cx, 0), W - 1), y = min(max(ty0 - HALO + cy, 0), H - 1);
    float col[3];
    if (cv.photo != 0) {
      const unsigned char* p = base + cv.photo_off + (long long)y * cv.photo_pitch + 3 * x;
      col[0] = (float)p[0];
      col[1] = (float)p[1];
      col[2] = (float)p[2];
    } else {
      const float tt = fminf(fmaxf(cv.gx * ((float)x + 0.5f) + cv.gy * ((float)y + 0.5f) + cv.g0, 0.f), 1.f);
#pragma unroll
      for (int c = 0; c < 3; ++c) col[c] = cv.bg0[c] + (cv.bg1[c] - cv.bg0[c]) * tt;
    }
    for (int s = 0; s < nkept; ++s) {
      const ItemL& it = s_item[s];
      if (x < it.x0 || x >= it.x1 || y < it.y0 || y >= it.y1) continue;
      const double px = (double)x + 0.5, py = (double)y + 0.5;
      const double X = it.h[0] * px + it.h[1] * py + it.h[2];
      const double Y = it.h[3] * px + it.h[4] * py + it.h[5];
      const double D = it.h[6] * px + it.h[7] * py + it.h[8];
      const double u = X / D - 0.5, v = Y / D - 0.5;
      const bool ok = D > 0.0;                              // D <= 0 or NaN: behind the map's horizon
      const float a = coverage(it, s_start[s], s_delta[s], base, ok, u, v);
      if (it.sa != 0.f) {
        const float sc = coverage(it, s_start[s], s_delta[s], base, ok, u - it.sdx, v - it.sdy);
        const float ts = sc * it.sa;
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c] = col[c] * (1.f - ts) + it.sh[c] * ts;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) col[c] = col[c] * (1.f - a) + it.fg[c] * a;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s_comp[cell * 3 + c] = col[c];
  }
  __syncthreads();

  // 4. the blur's horizontal pass over the tile's columns and all CH rows
  const float k0 = cv.w0, k1 = cv.w1, k2 = cv.w2;
  if (blur) {
    for (int cell = tid; cell < CH * TW; cell += 256) {
      const int ry = cell / TW, rx = cell - ry * TW;
      const float* p = s_comp + (ry * CW + rx) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        s_row[cell * 3 + c] = k2 * p[c] + k1 * p[3 + c] + k0 * p[6 + c] + k1 * p[9 + c] + k2 * p[12 + c];
    }
    __syncthreads();
  }

  // 5. vertical pass, noise, quantisation, the f32 planes; the bytes go to s_q
  for (int p = tid; p < TH * TW; p += 256) {
    const int ty = p / TW, tx = p - ty * TW;
    const int x = tx0 + tx, y = ty0 + ty;
    if (x >= W || y >= H) continue;
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float col;
      if (blur) {
        const float* r = s_row + (ty * TW + tx) * 3 + c;
        col = k2 * r[0] + k1 * r[TW * 3] + k0 * r[2 * TW * 3] + k1 * r[3 * TW * 3] + k2 * r[4 * TW * 3];
      } else {
        col = s_comp[((ty + HALO) * CW + tx + HALO) * 3 + c];
      }
      const unsigned k = ((unsigned)y * (unsigned)W + (unsigned)x) * 3u + (unsigned)c;
      const unsigned r = lowbias32((unsigned)cv.seed + k * 0x9E3779B9u);
      col = col + cv.noise_amp * ((float)(r >> 8) * 0x1p-24f - 0.5f);
      q[c] = fminf(fmaxf(floorf(col + 0.5f), 0.f), 255.f);
      s_q[p * 3 + c] = (unsigned char)q[c];
    }
    if (out_f32 != nullptr) store_normalized(out_f32, n, y, x, H, W, q, m0, m1, m2);
  }
  if (out_u8 == nullptr) return;
  __syncthreads();

  // 6. the uint8 rows: whole aligned dwords, single bytes at the two ends of the tile's row segment
  const int ncols = min(TW, W - tx0), nbytes = ncols * 3;
  for (int e = tid; e < TH * 64; e += 256) {
    const int r = e >> 6, slot = e & 63;
    const int y = ty0 + r;
    if (y >= H) continue;
    unsigned char* g0 = out_u8 + (((long long)n * H + y) * W + tx0) * 3;
    const int lead = (int)((uintptr_t)g0 & 3u);
    const int off = 4 * slot - lead;                        // this slot's first byte in the row segment
    if (off >= nbytes) continue;
    const unsigned char* q = s_q + r * TW * 3;
    if (off >= 0 && off + 4 <= nbytes) {
      *(unsigned*)(g0 + off) = (unsigned)q[off] | (unsigned)q[off + 1] << 8 | (unsigned)q[off + 2] << 16 |
                               (unsigned)q[off + 3] << 24;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (off + b >= 0 && off + b < nbytes) g0[off + b] = q[off + b];
    }
  }
}

// A table the host can read (pinned host memory), or nullptr.
template <typename T>
static const T* host_view(const void* p) {
  hipPointerAttribute_t attr;
  if (p != nullptr && hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost) return (const T*)p;
  (void)hipGetLastError();    // an address the runtime does not know is no error of this call
  return nullptr;
}

}  // namespace synth
}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_synth_font(void) { return (int)sizeof(mr_synth_font); }
int mr_sizeof_synth_item(void) { return (int)sizeof(mr_synth_item); }
int mr_sizeof_synth_canvas(void) { return (int)sizeof(mr_synth_canvas); }

int mr_synth_render(const unsigned char* base, const void* fonts, int F, const int* glyphs, int G, const void* items, int I,
                    const void* canvases, int N, int H, int W, double mean0, double mean1, double mean2,
                    unsigned char* out_u8, float* out_f32, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && F >= 0 && G >= 0 && I >= 0 && H >= 1 && W >= 1,
               "mr_synth_render: bad shape N=%d F=%d G=%d I=%d H=%d W=%d", N, F, G, I, H, W);
  if (N == 0) return MR_OK;
  MR_CHECK_ARG(out_u8 != nullptr || out_f32 != nullptr, "mr_synth_render: both outputs are null");
  MR_CHECK_ARG(canvases != nullptr && (I == 0 || items != nullptr) && (F == 0 || fonts != nullptr) &&
               (G == 0 || glyphs != nullptr), "mr_synth_render: null table");
  const int tiles_x = cdiv(W, synth::TW), tiles_y = cdiv(H, synth::TH);
  const long long tiles = (long long)tiles_x * tiles_y * N;
  MR_CHECK_ARG(tiles <= (long long)INT_MAX, "mr_synth_render: N=%d H=%d W=%d are %lld tiles, more than one launch", N, H, W,
               tiles);
  // Tables in pinned host memory are readable on both sides: check their indices here.  Device memory is the kernel's to guard.
  // (Not while `stream` is being captured: a capture records the launch alone, and a replay would not repeat the check.)
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) (void)hipGetLastError();
  const bool look = capturing == hipStreamCaptureStatusNone;
  const mr_synth_canvas* hc = look ? synth::host_view<mr_synth_canvas>(canvases) : nullptr;
  const mr_synth_item* hi = look ? synth::host_view<mr_synth_item>(items) : nullptr;
  const mr_synth_font* hf = look ? synth::host_view<mr_synth_font>(fonts) : nullptr;
  if (hc != nullptr)
    for (int n = 0; n < N; ++n) {
      MR_CHECK_ARG(hc[n].n_items >= 0 && hc[n].n_items <= MR_SYNTH_MAX_ITEMS && hc[n].first_item >= 0 &&
                   (long long)hc[n].first_item + hc[n].n_items <= I,
                   "mr_synth_render: canvas %d lists items %d + %d of %d (at most %d a canvas)", n, hc[n].first_item,
                   hc[n].n_items, I, MR_SYNTH_MAX_ITEMS);
      if (hi != nullptr)
        for (int k = hc[n].first_item; k < hc[n].first_item + hc[n].n_items; ++k)
          MR_CHECK_ARG(hi[k].canvas == n, "mr_synth_render: item %d of canvas %d names canvas %d", k, n, hi[k].canvas);
    }
  if (hi != nullptr)
    for (int k = 0; k < I; ++k) {
      MR_CHECK_ARG(hi[k].n_glyphs >= 0 && hi[k].n_glyphs <= MR_SYNTH_MAX_GLYPHS, "mr_synth_render: item %d has %d glyphs", k,
                   hi[k].n_glyphs);
      MR_CHECK_ARG(hi[k].font >= 0 && hi[k].font < F, "mr_synth_render: item %d names font %d of %d", k, hi[k].font, F);
      MR_CHECK_ARG(hi[k].canvas >= 0 && hi[k].canvas < N, "mr_synth_render: item %d names canvas %d of %d", k, hi[k].canvas, N);
    }
  if (hf != nullptr)
    for (int f = 0; f < F; ++f)
      MR_CHECK_ARG(hf[f].glyph_first >= 0 && hf[f].n_classes >= 0 && (long long)hf[f].glyph_first + hf[f].n_classes <= G,
                   "mr_synth_render: font %d lists glyph pairs %d + %d of %d", f, hf[f].glyph_first, hf[f].n_classes, G);
  hipLaunchKernelGGL(synth::synth_render_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, base,
                     (const mr_synth_font*)fonts, F, glyphs, G, (const mr_synth_item*)items, I,
                     (const mr_synth_canvas*)canvases, H, W, tiles_x, tiles_y, mean0, mean1, mean2, out_u8, out_f32);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
