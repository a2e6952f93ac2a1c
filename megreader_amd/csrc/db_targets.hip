// Training targets of the DB detector on the GPU: the four maps L1BalanceCELoss consumes (gt, mask, thresh_map, thresh_mask),
// which the reference draws on the host per sample with pyclipper, shapely and cv2 -- data/processes/
// make_seg_detection_data.py (`MakeSegDetectionData.process`, `validate_polygons`, `polygon_area`) and
// data/processes/make_border_map.py (`MakeBorderMap.process`, `draw_border_map`, `distance`) -- for QUADRILATERALS.
//   db_prep_kernel : one wavefront per polygon slot.  Clip to the image, signed area (`polygon_area`, same summation order),
//                    reorder, size filter, D = |a| (1 - r^2) / perimeter, and `shrinked == []` restated as "no pixel of the
//                    polygon's own box is inside it at squared distance >= D^2 from its boundary" (a scan with a
//                    wavefront-wide OR and an early exit).  Writes one DbRecord per slot.
//   db_map_kernel  : one workgroup per 64 x 16 pixel tile.  The image's records go through LDS in chunks of 256; each chunk
//                    is culled against the tile by box and compacted; every thread then walks the survivors for its four
//                    pixels and writes all four maps once (a wavefront stores 64 consecutive floats of a row).
// The combination rules are OR (gt, thresh_mask), AND (mask) and max (thresh_map): order-independent, so no atomics and
// the results are deterministic.  Pixel (x, y) is the integer point (x, y).  All geometry is float64 and is NOT contracted
// into FMAs, so that the float64 restatement the tests compare with (tests/_db_targets_ref.py) rounds the same way; what
// remains open against pyclipper / cv2 / shapely is stated in megreader_amd/data/detection_pipeline.py ("parity unpinned").
#include "common.h"
#include "../../include/megreader_hip.h"

#pragma clang fp contract(off)

namespace mr {

constexpr int DBT_MAX = 1024;      // polygon slots per image
constexpr int DBT_TX = 64;         // tile width: one wavefront per row
constexpr int DBT_TY = 16;         // tile height
constexpr int DBT_THREADS = 256;   // 4 wavefronts; thread (tx, ty) owns the pixels (tx, ty + 4 j), j = 0..3
constexpr int DBT_PPT = DBT_TY / (DBT_THREADS / DBT_TX);
constexpr int DBT_CHUNK = DBT_THREADS;   // records staged per pass: one per thread

constexpr int DB_UNUSED = 0, DB_KEPT = 1, DB_IGNORED = 2;

struct DbRecord {
  double p[8];       // clipped, reordered points (x0, y0, ..., x3, y3)
  double D, D2;      // shrink / border distance and its square (0 unless kept)
  int state;         // DB_UNUSED (slot >= count), DB_KEPT, DB_IGNORED
  int x0, x1, y0, y1;   // inclusive box.  kept: the border map's box [rnd(min - D), rnd(max + D)]; ignored: box of the
                        // truncated vertices.  Both are grown by one pixel where the map kernel culls.
  int pad[3];
};
static_assert(sizeof(DbRecord) == 112, "DbRecord layout");

__device__ __forceinline__ double sq(double v) { return v * v; }

// pyclipper's Round(): half away from zero
__device__ __forceinline__ double rnd_away(double v) { return copysign(floor(fabs(v) + 0.5), v); }

__device__ __forceinline__ int clamp_to_int(double v, int lo, int hi) {
  return v < (double)lo ? lo : (v > (double)hi ? hi : (int)v);
}

// does the edge a -> b cross the ray from (x, y) towards +x (even-odd rule)?
__device__ __forceinline__ bool crosses(double ax, double ay, double bx, double by, double x, double y) {
  if ((ay > y) == (by > y)) return false;
  const double xc = ax + (y - ay) * (bx - ax) / (by - ay);
  return x < xc;
}

// squared distance from (x, y) to the closed segment a-b of squared length s > 0
__device__ __forceinline__ double seg_dist2(double ax, double ay, double bx, double by, double s, double x, double y) {
  double t = ((x - ax) * (bx - ax) + (y - ay) * (by - ay)) / s;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double qx = ax + t * (bx - ax), qy = ay + t * (by - ay);
  return sq(x - qx) + sq(y - qy);
}

// MakeBorderMap.distance (make_border_map.py:95-120) for one pixel and one edge; s1, s2 = squared distances to the end
// points, s > 0 the squared edge length.  0 where s1 or s2 is 0 (the reference's nan_to_num path); 1 - cosin^2 is clamped
// at 0, where the reference would take the root of a negative rounding residue.
__device__ __forceinline__ double border_dist(double s1, double s2, double s) {
  if (s1 == 0.0 || s2 == 0.0) return 0.0;
  const double cosin = (s - s1 - s2) / (2.0 * sqrt(s1 * s2));
  if (cosin < 0.0) return sqrt(fmin(s1, s2));
  const double sin2 = fmax(1.0 - cosin * cosin, 0.0);
  return sqrt(s1 * s2 * sin2 / s);
}

// inside (even-odd) and minimum squared segment distance of (x, y) for the quad p; zero-length edges are skipped
__device__ __forceinline__ void quad_inside_dist2(const double* p, double x, double y, bool& inside, double& d2) {
  inside = false;
  d2 = INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int k1 = (k + 1) & 3;
    const double ax = p[2 * k], ay = p[2 * k + 1], bx = p[2 * k1], by = p[2 * k1 + 1];
    if (crosses(ax, ay, bx, by, x, y)) inside = !inside;
    const double s = sq(bx - ax) + sq(by - ay);
    if (s > 0.0) d2 = fmin(d2, seg_dist2(ax, ay, bx, by, s, x, y));
  }
}

__global__ __launch_bounds__(64) void db_prep_kernel(const double* __restrict__ polys, const int* __restrict__ count,
                                                     const int* __restrict__ ignore_in, int G, int H, int W,
                                                     double min_text_size, double shrink_ratio,
                                                     DbRecord* __restrict__ records, int* __restrict__ ignore_out,
                                                     double* __restrict__ dist) {
  const long long slot = blockIdx.x;                   // n * G + g
  const int n = (int)(slot / G), g = (int)(slot - (long long)n * G);
  const int lane = threadIdx.x;
  DbRecord r;
#pragma unroll
  for (int c = 0; c < 8; ++c) r.p[c] = 0.0;
  r.D = r.D2 = 0.0;
  r.state = DB_UNUSED;
  r.x0 = r.y0 = 0;
  r.x1 = r.y1 = -1;
  r.pad[0] = r.pad[1] = r.pad[2] = 0;
  if (g < count[n]) {                                  // wavefront-uniform
    double q[8];
    // 1. clip (every polygon, ignored ones included)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q[2 * k] = fmin(fmax(polys[slot * 8 + 2 * k], 0.0), (double)(W - 1));
      q[2 * k + 1] = fmin(fmax(polys[slot * 8 + 2 * k + 1], 0.0), (double)(H - 1));
    }
    // 2. polygon_area, summed in the reference's order
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int k1 = (k + 1) & 3;
      a += (q[2 * k1] - q[2 * k]) * (q[2 * k1 + 1] + q[2 * k + 1]);
    }
    a = a / 2.0;
    bool ignored = ignore_in[slot] != 0 || fabs(a) < 1.0;
    if (a > 0.0) {                                     // (0, 3, 2, 1)
      double t = q[2]; q[2] = q[6]; q[6] = t;
      t = q[3]; q[3] = q[7]; q[7] = t;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) r.p[c] = q[c];
    // 3. size filter
    const double e01 = sqrt(sq(q[0] - q[2]) + sq(q[1] - q[3])), e12 = sqrt(sq(q[2] - q[4]) + sq(q[3] - q[5]));
    const double e23 = sqrt(sq(q[4] - q[6]) + sq(q[5] - q[7])), e30 = sqrt(sq(q[6] - q[0]) + sq(q[7] - q[1]));
    const double height = fmin(e30, e12), width = fmin(e01, e23);
    if (fmin(height, width) < min_text_size) ignored = true;
    const double xl = fmin(fmin(q[0], q[2]), fmin(q[4], q[6])), xh = fmax(fmax(q[0], q[2]), fmax(q[4], q[6]));
    const double yl = fmin(fmin(q[1], q[3]), fmin(q[5], q[7])), yh = fmax(fmax(q[1], q[3]), fmax(q[5], q[7]));
    double D = 0.0, D2 = 0.0;
    if (!ignored) {
      // 4. D
      const double perimeter = e01 + e12 + e23 + e30;
      D = fabs(a) * (1.0 - shrink_ratio * shrink_ratio) / perimeter;
      D2 = D * D;
      // 5. does the shrunk region cover a pixel?  scan of the vertex box (inside [0, W-1] x [0, H-1] after the clip)
      const int bx0 = (int)ceil(xl), bx1 = (int)floor(xh), by0 = (int)ceil(yl), by1 = (int)floor(yh);
      const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
      bool found = false;
      if (bw > 0 && bh > 0) {
        const int total = bw * bh;                     // <= H * W, which the launcher keeps below 2^31
        for (int base = 0; base < total && !found; base += 64) {
          const int i = base + lane;
          bool hit = false;
          if (i < total) {
            const int yy = i / bw, xx = i - yy * bw;
            bool inside;
            double d2;
            quad_inside_dist2(q, (double)(bx0 + xx), (double)(by0 + yy), inside, d2);
            hit = inside && d2 >= D2;
          }
          found = __ballot(hit) != 0ull;
        }
      }
      if (!found) {
        ignored = true;
        D = D2 = 0.0;
      }
    }
    r.D = D;
    r.D2 = D2;
    if (ignored) {
      r.state = DB_IGNORED;
      r.x0 = (int)xl; r.x1 = (int)xh; r.y0 = (int)yl; r.y1 = (int)yh;   // truncation is monotone: the box of the truncated points
    } else {
      r.state = DB_KEPT;
      r.x0 = clamp_to_int(rnd_away(xl - D), -1, W);
      r.x1 = clamp_to_int(rnd_away(xh + D), -1, W);
      r.y0 = clamp_to_int(rnd_away(yl - D), -1, H);
      r.y1 = clamp_to_int(rnd_away(yh + D), -1, H);
    }
  }
  if (lane == 0) {
    records[slot] = r;
    ignore_out[slot] = r.state == DB_IGNORED ? 1 : 0;
    dist[slot] = r.D;
  }
}

__global__ __launch_bounds__(DBT_THREADS) void db_map_kernel(const DbRecord* __restrict__ records, const int* __restrict__ count,
                                                             int G, int H, int W, float thresh_scale, float thresh_base,
                                                             float* __restrict__ gt, float* __restrict__ mask,
                                                             float* __restrict__ thresh_map, float* __restrict__ thresh_mask) {
  __shared__ DbRecord list[DBT_CHUNK];                 // 28 KiB: the chunk's survivors, compacted
  __shared__ int wave_hits[DBT_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.z;
  const int tx0 = blockIdx.x * DBT_TX, ty0 = blockIdx.y * DBT_TY;
  const int tx1 = min(tx0 + DBT_TX, W) - 1, ty1 = min(ty0 + DBT_TY, H) - 1;   // inclusive
  const int x = tx0 + lane;
  int used = count[n];
  used = used < 0 ? 0 : (used > G ? G : used);
  const DbRecord* recs = records + (long long)n * G;

  bool o_gt[DBT_PPT], o_ign[DBT_PPT], o_tm[DBT_PPT];
  float o_c[DBT_PPT];
#pragma unroll
  for (int j = 0; j < DBT_PPT; ++j) {
    o_gt[j] = o_ign[j] = o_tm[j] = false;
    o_c[j] = 0.0f;
  }

  for (int base = 0; base < used; base += DBT_CHUNK) {
    // cull this chunk against the tile and compact the survivors into LDS
    const int g = base + tid;
    bool hit = false;
    if (g < used) {
      const DbRecord* r = recs + g;
      hit = r->state != DB_UNUSED && r->x0 - 1 <= tx1 && r->x1 + 1 >= tx0 && r->y0 - 1 <= ty1 && r->y1 + 1 >= ty0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_hits[wave] = __popcll(m);
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull)), nlist = 0;
#pragma unroll
    for (int w = 0; w < DBT_THREADS / 64; ++w) {
      const int c = wave_hits[w];
      if (w < wave) pos += c;
      nlist += c;
    }
    if (hit) {
      DbRecord r = recs[g];
      if (r.state == DB_IGNORED) {                     // astype(int32): the mask is filled over the truncated points
#pragma unroll
        for (int c = 0; c < 8; ++c) r.p[c] = trunc(r.p[c]);
      }
      list[pos] = r;
    }
    __syncthreads();

    if (x < W) {
      for (int i = 0; i < nlist; ++i) {                // the same record in every lane: LDS broadcast, uniform branches
        const DbRecord& r = list[i];
        double p[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) p[c] = r.p[c];
        const int state = r.state, bx0 = r.x0, bx1 = r.x1, by0 = r.y0, by1 = r.y1;
        const double D = r.D, D2 = r.D2;
#pragma unroll
        for (int j = 0; j < DBT_PPT; ++j) {
          const int y = ty0 + wave + (DBT_THREADS / 64) * j;
          if (y >= H || x < bx0 - 1 || x > bx1 + 1 || y < by0 - 1 || y > by1 + 1) continue;
          const double px = (double)x, py = (double)y;
          bool inside = false;
          double d2 = INFINITY, e = INFINITY;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const double ax = p[2 * k], ay = p[2 * k + 1], bx = p[2 * k1], by = p[2 * k1 + 1];
            if (crosses(ax, ay, bx, by, px, py)) inside = !inside;
            const double s = sq(bx - ax) + sq(by - ay);
            if (s > 0.0) {
              d2 = fmin(d2, seg_dist2(ax, ay, bx, by, s, px, py));
              if (state == DB_KEPT) e = fmin(e, border_dist(sq(px - ax) + sq(py - ay), sq(px - bx) + sq(py - by), s));
            }
          }
          if (state == DB_KEPT) {
            if (inside && d2 >= D2) o_gt[j] = true;
            if (inside || d2 <= D2) o_tm[j] = true;
            if (x >= bx0 && x <= bx1 && y >= by0 && y <= by1) {
              const float ratio = (float)fmin(e / D, 1.0);   // distance_map is float32
              o_c[j] = fmaxf(o_c[j], 1.0f - ratio);
            }
          } else if (inside || d2 <= 0.25) {
            o_ign[j] = true;
          }
        }
      }
    }
    __syncthreads();                                   // the list is rewritten by the next chunk
  }

  if (x < W) {
#pragma unroll
    for (int j = 0; j < DBT_PPT; ++j) {
      const int y = ty0 + wave + (DBT_THREADS / 64) * j;
      if (y < H) {
        const long long o = ((long long)n * H + y) * W + x;
        gt[o] = o_gt[j] ? 1.0f : 0.0f;
        mask[o] = o_ign[j] ? 0.0f : 1.0f;
        thresh_mask[o] = o_tm[j] ? 1.0f : 0.0f;
        thresh_map[o] = o_c[j] * thresh_scale + thresh_base;
      }
    }
  }
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_db_record(void) { return (int)sizeof(DbRecord); }

int mr_db_targets(const double* polys, const int* count, const int* ignore_in, int N, int G, int H, int W,
                  double min_text_size, double shrink_ratio, double thresh_min, double thresh_max, void* records,
                  int* ignore_out, double* dist, float* gt, float* mask, float* thresh_map, float* thresh_mask,
                  hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && G >= 0 && H > 0 && W > 0, "mr_db_targets: bad shape N=%d G=%d H=%d W=%d", N, G, H, W);
  if (G > DBT_MAX) {
    set_error("mr_db_targets: G=%d polygon slots per image exceed the %d supported", G, DBT_MAX);
    return MR_ERR_UNSUPPORTED;
  }
  MR_CHECK_ARG((long long)H * W < (1ll << 31) && N <= 65535 && (H + DBT_TY - 1) / DBT_TY <= 65535,
               "mr_db_targets: N=%d H=%d W=%d exceed the launch grid", N, H, W);
  if (N == 0) return MR_OK;
  if (G > 0)
    hipLaunchKernelGGL(db_prep_kernel, dim3((unsigned)((long long)N * G)), dim3(64), 0, stream, polys, count, ignore_in, G, H, W,
                       min_text_size, shrink_ratio, (DbRecord*)records, ignore_out, dist);
  // thresh_map = canvas * (thresh_max - thresh_min) + thresh_min on a float32 canvas (make_border_map.py:42)
  hipLaunchKernelGGL(db_map_kernel, dim3((W + DBT_TX - 1) / DBT_TX, (H + DBT_TY - 1) / DBT_TY, N), dim3(DBT_THREADS), 0, stream,
                     (const DbRecord*)records, count, G, H, W, (float)(thresh_max - thresh_min), (float)thresh_min, gt, mask,
                     thresh_map, thresh_mask);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
