// Detection metrics of the DB detector on the GPU: the polygon work of concern/icdar2015_eval/detection/iou.py
// (`DetectionIoUEvaluator.evaluate_image`), which the reference does with one shapely call per (ground truth, detection)
// pair, per don't-care test and per validity check, for QUADRILATERALS (structure/measurers/quad_measurer.py).
//   mr_quad_iou   : validity + shoelace area of every quad, intersection area and IoU of every (gt, det) pair of an image;
//   mr_poly_iou   : the same tables for simple polygons of 3 .. 64 vertices (curved text), by signed fans of triangles;
//   mr_quad_match : the per-image bookkeeping -- don't-care sets, the greedy matching in the reference's (g, d) order,
//                   gtCare / detCare / detMatched and precision / recall / hmean.
// All arithmetic is float64 and is NOT contracted into FMAs, so that the plain float64 restatement the tests compare
// with (tests/_quad_eval_ref.py) rounds the same way; what remains open against GEOS is stated in
// megreader_amd/structure/quad_measurer.py ("parity unpinned").
//
// Validity (shapely's `is_valid and is_simple` restated for a 4-gon): the shoelace area is non-zero (and finite) and neither pair
// of opposite edges (0-1 / 2-3, 1-2 / 3-0) intersects or touches.
// Intersection area, exact for every pair of valid quads, either orientation, convex or not: each quad is split into two
// triangles along the diagonal for which both triangles keep the quad's orientation (a simple 4-gon has one), each of
// the four triangle pairs is clipped with Sutherland-Hodgman (a convex clip polygon: at most 6 vertices) and the four
// areas are summed -- the triangles of one quad do not overlap, so nothing is counted twice.
// A few thousand pairs per validation batch: latency-bound, a handful of microseconds per launch.
#include "common.h"
#include "../../include/megreader_hip.h"

#pragma clang fp contract(off)

namespace mr {

constexpr int QM_MAX = 1024;   // quads per image and side that mr_quad_match keeps in LDS
constexpr int QP_THREADS = 128; // threads of a pair block: every thread owns two 8-vertex polygons in LDS (32 KB per block)
constexpr int QP_VERTS = 8;

// twice the signed area of the triangle (p, q, r): > 0 counter-clockwise (y up)
__device__ __forceinline__ double orient2(double px, double py, double qx, double qy, double rx, double ry) {
  return (qx - px) * (ry - py) - (qy - py) * (rx - px);
}

__device__ __forceinline__ bool in_box(double ax, double ay, double bx, double by, double px, double py) {
  return px >= fmin(ax, bx) && px <= fmax(ax, bx) && py >= fmin(ay, by) && py <= fmax(ay, by);
}

// do the closed segments a-b and c-d share a point?
__device__ __forceinline__ bool segments_touch(double ax, double ay, double bx, double by, double cx, double cy, double dx,
                                               double dy) {
  const double o1 = orient2(ax, ay, bx, by, cx, cy), o2 = orient2(ax, ay, bx, by, dx, dy);
  const double o3 = orient2(cx, cy, dx, dy, ax, ay), o4 = orient2(cx, cy, dx, dy, bx, by);
  if (((o1 > 0.0 && o2 < 0.0) || (o1 < 0.0 && o2 > 0.0)) && ((o3 > 0.0 && o4 < 0.0) || (o3 < 0.0 && o4 > 0.0))) return true;
  if (o1 == 0.0 && in_box(ax, ay, bx, by, cx, cy)) return true;
  if (o2 == 0.0 && in_box(ax, ay, bx, by, dx, dy)) return true;
  if (o3 == 0.0 && in_box(cx, cy, dx, dy, ax, ay)) return true;
  if (o4 == 0.0 && in_box(cx, cy, dx, dy, bx, by)) return true;
  return false;
}

// twice the signed shoelace area of the quad q = (x0, y0, ..., x3, y3)
__device__ __forceinline__ double quad_area2(const double* q) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int k1 = (k + 1) & 3;
    s += q[2 * k] * q[2 * k1 + 1] - q[2 * k1] * q[2 * k + 1];
  }
  return s;
}

// valid / area of every slot: i over [N][G + D], the gts of an image first.  Padding slots: valid 0, area 0.
__global__ void quad_prep_kernel(const double* __restrict__ gt, const int* __restrict__ gt_count, const double* __restrict__ det,
                                 const int* __restrict__ det_count, int N, int G, int D, int* __restrict__ gt_valid,
                                 int* __restrict__ det_valid, double* __restrict__ gt_area, double* __restrict__ det_area) {
  const long long total = (long long)N * (G + D);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i / (G + D)), k = (int)(i - (long long)n * (G + D));
    const bool is_gt = k < G;
    const int j = is_gt ? k : k - G;
    const long long slot = is_gt ? (long long)n * G + j : (long long)n * D + j;
    const int count = is_gt ? gt_count[n] : det_count[n];
    int valid = 0;
    double area = 0.0;
    if (j < count) {
      const double* src = (is_gt ? gt : det) + slot * 8;
      double q[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) q[c] = src[c];
      const double a2 = fabs(quad_area2(q));
      if (a2 > 0.0 && a2 < INFINITY && !segments_touch(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]) &&
          !segments_touch(q[2], q[3], q[4], q[5], q[6], q[7], q[0], q[1])) {
        valid = 1;
        area = 0.5 * a2;
      }
    }
    (is_gt ? gt_valid : det_valid)[slot] = valid;
    (is_gt ? gt_area : det_area)[slot] = area;
  }
}

// The two counter-clockwise triangles of a simple quad: t[0..5] and t[6..11] as (x, y) triples.
__device__ __forceinline__ void quad_triangles(const double* q, double* t) {
  const double sgn = quad_area2(q) > 0.0 ? 1.0 : -1.0;
  const double t1 = sgn * orient2(q[0], q[1], q[2], q[3], q[4], q[5]);
  const double t2 = sgn * orient2(q[0], q[1], q[4], q[5], q[6], q[7]);
  const bool d02 = t1 >= 0.0 && t2 >= 0.0;      // diagonal 0-2 lies inside; otherwise 1-3 does
  // (0,1,2) + (0,2,3)  or  (1,2,3) + (1,3,0)
  const int cw = sgn < 0.0;                      // clockwise input: swap the last two vertices of each triangle
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double a0 = d02 ? q[0 + c] : q[2 + c];
    const double a1 = d02 ? q[2 + c] : q[4 + c];
    const double a2 = d02 ? q[4 + c] : q[6 + c];
    const double b1 = d02 ? q[4 + c] : q[6 + c];
    const double b2 = d02 ? q[6 + c] : q[0 + c];
    t[0 + c] = a0;
    t[2 + c] = cw ? a2 : a1;
    t[4 + c] = cw ? a1 : a2;
    t[6 + c] = a0;
    t[8 + c] = cw ? b2 : b1;
    t[10 + c] = cw ? b1 : b2;
  }
}

// One Sutherland-Hodgman step: keep the part of the polygon (ix, iy)[0..n) on the left of (or on) the line a -> b.
// Vertex k of this thread's polygon is at [k * STRIDE], STRIDE = the threads of the block.  A convex polygon gains at most
// one vertex per step (3 -> 4 -> 5 -> 6); the bound QP_VERTS is enforced all the same.
template <int STRIDE = QP_THREADS>
__device__ __forceinline__ int clip_left_of(const double* ix, const double* iy, int n, double ax, double ay, double bx, double by,
                                            double* ox, double* oy) {
  if (n == 0) return 0;
  int m = 0;
  double px = ix[(n - 1) * STRIDE], py = iy[(n - 1) * STRIDE];
  double dp = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
  for (int k = 0; k < n; ++k) {
    const double qx = ix[k * STRIDE], qy = iy[k * STRIDE];
    const double dq = (bx - ax) * (qy - ay) - (by - ay) * (qx - ax);
    if (((dp > 0.0 && dq < 0.0) || (dp < 0.0 && dq > 0.0)) && m < QP_VERTS) {
      const double t = dp / (dp - dq);
      ox[m * STRIDE] = px + t * (qx - px);
      oy[m * STRIDE] = py + t * (qy - py);
      ++m;
    }
    if (dq >= 0.0 && m < QP_VERTS) {
      ox[m * STRIDE] = qx;
      oy[m * STRIDE] = qy;
      ++m;
    }
    px = qx; py = qy; dp = dq;
  }
  return m;
}

// area of (counter-clockwise triangle s) intersected with (counter-clockwise triangle c); s, c = (x, y) triples
template <int STRIDE = QP_THREADS>
__device__ __forceinline__ double triangle_overlap(const double* s, const double* c, double* x0, double* y0, double* x1,
                                                   double* y1) {
  if (orient2(s[0], s[1], s[2], s[3], s[4], s[5]) == 0.0 || orient2(c[0], c[1], c[2], c[3], c[4], c[5]) == 0.0) return 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x0[k * STRIDE] = s[2 * k];
    y0[k * STRIDE] = s[2 * k + 1];
  }
  int n = clip_left_of<STRIDE>(x0, y0, 3, c[0], c[1], c[2], c[3], x1, y1);
  n = clip_left_of<STRIDE>(x1, y1, n, c[2], c[3], c[4], c[5], x0, y0);
  n = clip_left_of<STRIDE>(x0, y0, n, c[4], c[5], c[0], c[1], x1, y1);
  if (n < 3) return 0.0;
  const double bx = x1[0], by = y1[0];
  double sum = 0.0;
  for (int k = 1; k + 1 < n; ++k)
    sum += (x1[k * STRIDE] - bx) * (y1[(k + 1) * STRIDE] - by) -
           (x1[(k + 1) * STRIDE] - bx) * (y1[k * STRIDE] - by);
  return 0.5 * fabs(sum);
}

// one thread per (n, g, d)
__global__ __launch_bounds__(QP_THREADS) void quad_pair_kernel(const double* __restrict__ gt, const double* __restrict__ det,
                                                               int N, int G, int D, const int* __restrict__ gt_valid,
                                                               const int* __restrict__ det_valid,
                                                               const double* __restrict__ gt_area,
                                                               const double* __restrict__ det_area, double* __restrict__ inter,
                                                               double* __restrict__ iou) {
  __shared__ double poly[4][QP_VERTS][QP_THREADS];      // x0, y0, x1, y1 of the two clip buffers
  double* x0 = &poly[0][0][threadIdx.x];
  double* y0 = &poly[1][0][threadIdx.x];
  double* x1 = &poly[2][0][threadIdx.x];
  double* y1 = &poly[3][0][threadIdx.x];
  const long long total = (long long)N * G * D;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const long long ng = i / D;                          // n * G + g
    const long long nd = (ng / G) * D + d;               // n * D + d
    double a = 0.0, r = 0.0;
    if (gt_valid[ng] != 0 && det_valid[nd] != 0) {
      double p[8], q[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        p[c] = gt[ng * 8 + c];
        q[c] = det[nd * 8 + c];
      }
      const double pxl = fmin(fmin(p[0], p[2]), fmin(p[4], p[6])), pxh = fmax(fmax(p[0], p[2]), fmax(p[4], p[6]));
      const double pyl = fmin(fmin(p[1], p[3]), fmin(p[5], p[7])), pyh = fmax(fmax(p[1], p[3]), fmax(p[5], p[7]));
      const double qxl = fmin(fmin(q[0], q[2]), fmin(q[4], q[6])), qxh = fmax(fmax(q[0], q[2]), fmax(q[4], q[6]));
      const double qyl = fmin(fmin(q[1], q[3]), fmin(q[5], q[7])), qyh = fmax(fmax(q[1], q[3]), fmax(q[5], q[7]));
      if (pxl <= qxh && qxl <= pxh && pyl <= qyh && qyl <= pyh) {       // disjoint boxes: exactly zero
        double tp[12], tq[12];
        quad_triangles(p, tp);
        quad_triangles(q, tq);
        a = triangle_overlap(tp, tq, x0, y0, x1, y1);
        a += triangle_overlap(tp, tq + 6, x0, y0, x1, y1);
        a += triangle_overlap(tp + 6, tq, x0, y0, x1, y1);
        a += triangle_overlap(tp + 6, tq + 6, x0, y0, x1, y1);
      }
      r = a / (gt_area[ng] + det_area[nd] - a);
    }
    inter[i] = a;
    iou[i] = r;
  }
}

// One wavefront per image.  Indices are positions in the compacted lists of valid quads (original order), as the
// reference's gtPols / detPols.  state of a detection: 0 free, 1 don't-care, 2 matched.
__global__ __launch_bounds__(64) void quad_match_kernel(const int* __restrict__ gt_valid, const int* __restrict__ det_valid,
                                                        const int* __restrict__ gt_ignore, const double* __restrict__ det_area,
                                                        const double* __restrict__ inter, const double* __restrict__ iou, int G,
                                                        int D, double iou_constraint, double area_precision_constraint,
                                                        int* __restrict__ counts, double* __restrict__ scores,
                                                        int* __restrict__ match_det, int* __restrict__ gt_dontcare,
                                                        int* __restrict__ det_dontcare) {
  __shared__ int gmap[QM_MAX], dmap[QM_MAX];            // compacted index -> slot
  __shared__ unsigned char gdc[QM_MAX], dstate[QM_MAX];
  const long long n = blockIdx.x;
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  int ng = 0, ngdc = 0, nd = 0, nddc = 0, matched = 0;
  for (int base = 0; base < G; base += 64) {
    const int g = base + lane;
    const bool v = g < G && gt_valid[n * G + g] != 0;
    const bool dc = v && gt_ignore[n * G + g] != 0;
    const unsigned long long m = __ballot(v);
    if (v) {
      const int pos = ng + __popcll(m & below);
      gmap[pos] = g;
      gdc[pos] = dc ? 1 : 0;
    }
    ng += __popcll(m);
    ngdc += __popcll(__ballot(dc));
  }
  for (int base = 0; base < D; base += 64) {
    const int d = base + lane;
    const bool v = d < D && det_valid[n * D + d] != 0;
    const unsigned long long m = __ballot(v);
    if (v) dmap[nd + __popcll(m & below)] = d;
    nd += __popcll(m);
  }
  __syncthreads();
  // a detection is don't-care when a don't-care gt covers more than the constraint of ITS area
  for (int base = 0; base < nd; base += 64) {
    const int cd = base + lane;
    bool dc = false;
    if (cd < nd && ngdc > 0) {
      const int d = dmap[cd];
      const double a = det_area[n * D + d];
      for (int cg = 0; cg < ng; ++cg)
        if (gdc[cg] && a != 0.0 && inter[(n * G + gmap[cg]) * D + d] / a > area_precision_constraint) dc = true;
    }
    if (cd < nd) dstate[cd] = dc ? 1 : 0;
    nddc += __popcll(__ballot(dc));
  }
  __syncthreads();
  // greedy matching: g ascending, per g the lowest free care detection above the constraint
  for (int cg = 0; cg < ng; ++cg) {
    int md = -1;
    if (!gdc[cg]) {
      const double* row = iou + (n * G + gmap[cg]) * D;
      for (int base = 0; base < nd && md < 0; base += 64) {
        const int cd = base + lane;
        const bool ok = cd < nd && dstate[cd] == 0 && row[dmap[cd]] > iou_constraint;
        const unsigned long long m = __ballot(ok);
        if (m) {
          const int first = __ffsll((long long)m) - 1;
          md = base + first;
          if (lane == first) dstate[cd] = 2;
        }
      }
    }
    if (md >= 0) ++matched;
    if (lane == 0) match_det[n * G + cg] = md;
    __syncthreads();                                     // the state written by one lane is read by all for the next g
  }
  for (int g = lane; g < G; g += 64) {
    if (g >= ng) match_det[n * G + g] = -1;
    gt_dontcare[n * G + g] = g < ng ? gdc[g] : 0;
  }
  for (int d = lane; d < D; d += 64) det_dontcare[n * D + d] = d < nd ? (dstate[d] == 1 ? 1 : 0) : 0;
  if (lane == 0) {
    const int gt_care = ng - ngdc, det_care = nd - nddc;
    double precision, recall;
    if (gt_care == 0) {
      recall = 1.0;
      precision = det_care > 0 ? 0.0 : 1.0;
    } else {
      recall = (double)matched / gt_care;
      precision = det_care == 0 ? 0.0 : (double)matched / det_care;
    }
    const double hmean = precision + recall == 0.0 ? 0.0 : 2.0 * precision * recall / (precision + recall);
    counts[n * 4 + 0] = gt_care;
    counts[n * 4 + 1] = det_care;
    counts[n * 4 + 2] = matched;
    counts[n * 4 + 3] = ng;
    scores[n * 3 + 0] = precision;
    scores[n * 3 + 1] = recall;
    scores[n * 3 + 2] = hmean;
  }
}

// ---- simple polygons of 3 .. MR_POLY_MAX_VERTS vertices (mr_poly_iou; the rule is written out in include/megreader_hip.h) --------

constexpr int PV_MAX = MR_POLY_MAX_VERTS;     // a lane per vertex / edge: one wavefront holds a polygon
constexpr int PP_SPLIT = 4;                   // wavefronts that share the surviving detections of one ground truth

// valid / area of every slot, one wavefront (= one block) per slot: i over [N][G + D], the gts of an image first.  Lane e owns the
// edge e -> e + 1 and tests it against every other edge.  Padding slots and counts outside 3 .. V: valid 0, area 0.
__global__ __launch_bounds__(PV_MAX) void poly_prep_kernel(const double* __restrict__ gt, const int* __restrict__ gt_verts,
                                                           const int* __restrict__ gt_count, const double* __restrict__ det,
                                                           const int* __restrict__ det_verts, const int* __restrict__ det_count,
                                                           int N, int G, int D, int V, int* __restrict__ gt_valid,
                                                           int* __restrict__ det_valid, double* __restrict__ gt_area,
                                                           double* __restrict__ det_area) {
  __shared__ double vx[PV_MAX], vy[PV_MAX];
  const int lane = threadIdx.x;
  const long long total = (long long)N * (G + D);
  for (long long i = blockIdx.x; i < total; i += gridDim.x) {
    const int n = (int)(i / (G + D)), k = (int)(i - (long long)n * (G + D));
    const bool is_gt = k < G;
    const int j = is_gt ? k : k - G;
    const long long slot = is_gt ? (long long)n * G + j : (long long)n * D + j;
    const int count = is_gt ? gt_count[n] : det_count[n];
    const int m = j < count ? (is_gt ? gt_verts : det_verts)[slot] : 0;
    int valid = 0;
    double area = 0.0;
    if (m >= 3 && m <= V) {                              // (uniform: the block is one wavefront)
      const double* src = (is_gt ? gt : det) + slot * V * 2;
      __syncthreads();                                   // the previous slot's reads are done
      if (lane < m) {
        vx[lane] = src[2 * lane];
        vy[lane] = src[2 * lane + 1];
      }
      __syncthreads();
      double s = 0.0;                                    // twice the signed shoelace area, edges 0, 1, ... in turn
      for (int e = 0; e < m; ++e) {
        const int e1 = e + 1 == m ? 0 : e + 1;
        s += vx[e] * vy[e1] - vx[e1] * vy[e];
      }
      const double a2 = fabs(s);
      bool bad = !(a2 > 0.0 && a2 < INFINITY);
      if (!bad && lane < m) {
        const int e1 = lane + 1 == m ? 0 : lane + 1;
        const double ax = vx[lane], ay = vy[lane], bx = vx[e1], by = vy[e1];
        for (int f = 0; f < m; ++f) {
          if (f == lane) continue;
          const int f1 = f + 1 == m ? 0 : f + 1;
          const double cx = vx[f], cy = vy[f], dx = vx[f1], dy = vy[f1];
          if (cx == ax && cy == ay) {
            bad = true;                                  // a repeated vertex
          } else if (f == e1) {                          // the next edge b -> d: only b may be shared, no fold back onto a - b
            if (orient2(ax, ay, bx, by, dx, dy) == 0.0 && (ax - bx) * (dx - bx) + (ay - by) * (dy - by) > 0.0) bad = true;
          } else if (f1 != lane) {                       // (the previous edge tests this one as its next)
            if (segments_touch(ax, ay, bx, by, cx, cy, dx, dy)) bad = true;
          }
        }
      }
      if (__ballot(bad) == 0ull) {
        valid = 1;
        area = 0.5 * a2;
      }
    }
    if (lane == 0) {
      (is_gt ? gt_valid : det_valid)[slot] = valid;
      (is_gt ? gt_area : det_area)[slot] = area;
    }
  }
}

// PP_SPLIT wavefronts (blocks of one) per ground truth (n, g).  A lane per detection d tests the boxes; the surviving d are dealt
// to the wavefronts in turn, and for each of its d a wavefront sums the signed overlaps of the fan triangles, lanes striding over
// the (i, j) triangle pairs.  The first wavefront writes the zeros of the pairs that end at the box test.
__global__ __launch_bounds__(PV_MAX) void poly_pair_kernel(const double* __restrict__ gt, const int* __restrict__ gt_verts,
                                                           const double* __restrict__ det, const int* __restrict__ det_verts,
                                                           int N, int G, int D, int V, const int* __restrict__ gt_valid,
                                                           const int* __restrict__ det_valid, const double* __restrict__ gt_area,
                                                           const double* __restrict__ det_area, double* __restrict__ inter,
                                                           double* __restrict__ iou) {
  __shared__ double clip[4][QP_VERTS][PV_MAX];          // x0, y0, x1, y1 of the two clip buffers, a column per lane
  __shared__ double px[PV_MAX], py[PV_MAX], qx[PV_MAX], qy[PV_MAX];
  const int lane = threadIdx.x;
  double* x0 = &clip[0][0][lane];
  double* y0 = &clip[1][0][lane];
  double* x1 = &clip[2][0][lane];
  double* y1 = &clip[3][0][lane];
  const int part = blockIdx.y;                           // of PP_SPLIT: the row's survivors are dealt out in turn
  const long long rows = (long long)N * G;
  for (long long ng = blockIdx.x; ng < rows; ng += gridDim.x) {
    const long long n = ng / G;
    if (gt_valid[ng] == 0) {
      for (int d = lane; d < D && part == 0; d += PV_MAX) {
        inter[ng * D + d] = 0.0;
        iou[ng * D + d] = 0.0;
      }
      continue;
    }
    const int m = gt_verts[ng];                          // 3 .. V: the polygon is valid
    __syncthreads();                                     // the previous row's reads are done
    if (lane < m) {
      px[lane] = gt[(ng * V + lane) * 2];
      py[lane] = gt[(ng * V + lane) * 2 + 1];
    }
    __syncthreads();
    const double ox = px[0], oy = py[0];
    double pxl = ox, pxh = ox, pyl = oy, pyh = oy;
    for (int v = 1; v < m; ++v) {
      pxl = fmin(pxl, px[v]); pxh = fmax(pxh, px[v]);
      pyl = fmin(pyl, py[v]); pyh = fmax(pyh, py[v]);
    }
    __syncthreads();
    if (lane < m) {                                      // translated: the first vertex is the origin
      px[lane] -= ox;
      py[lane] -= oy;
    }
    const double ga = gt_area[ng];
    int turn = 0;
    for (int base = 0; base < D; base += PV_MAX) {
      const int d = base + lane;
      int nq = 0;
      bool live = false;
      if (d < D) {
        const long long nd = n * D + d;
        if (det_valid[nd] != 0) {
          nq = det_verts[nd];
          const double* q = det + nd * V * 2;
          double qxl = q[0], qxh = q[0], qyl = q[1], qyh = q[1];
          for (int v = 1; v < nq; v += 4) {              // four vertices' loads in flight; past the end the last one again
            double x[4], y[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int w = v + u < nq ? v + u : nq - 1;
              x[u] = q[2 * w];
              y[u] = q[2 * w + 1];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              qxl = fmin(qxl, x[u]); qxh = fmax(qxh, x[u]);
              qyl = fmin(qyl, y[u]); qyh = fmax(qyh, y[u]);
            }
          }
          live = pxl <= qxh && qxl <= pxh && pyl <= qyh && qyl <= pyh;
        }
        if (!live && part == 0) {                        // an invalid member or disjoint boxes: exactly zero
          inter[ng * D + d] = 0.0;
          iou[ng * D + d] = 0.0;
        }
      }
      unsigned long long todo = __ballot(live);
      while (todo != 0ull) {                             // (uniform)
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        if (turn++ % PP_SPLIT != part) continue;
        const long long nd = n * D + base + src;
        const int mq = __shfl(nq, src);
        __syncthreads();                                 // px / py are translated; the previous pair's reads of qx / qy are done
        if (lane < mq) {
          qx[lane] = det[(nd * V + lane) * 2] - ox;
          qy[lane] = det[(nd * V + lane) * 2 + 1] - oy;
        }
        __syncthreads();
        const int tq = mq - 2, pairs = (m - 2) * tq;
        double acc = 0.0;
        for (int t = lane; t < pairs; t += PV_MAX) {
          const int i = t / tq, j = t - i * tq;
          const double os = orient2(px[0], py[0], px[i + 1], py[i + 1], px[i + 2], py[i + 2]);
          const double oc = orient2(qx[0], qy[0], qx[j + 1], qy[j + 1], qx[j + 2], qy[j + 2]);
          if (os == 0.0 || oc == 0.0) continue;
          const int sa = os > 0.0 ? i + 1 : i + 2, sb = os > 0.0 ? i + 2 : i + 1;      // stored counter-clockwise
          const int ca = oc > 0.0 ? j + 1 : j + 2, cb = oc > 0.0 ? j + 2 : j + 1;
          const double s[6] = {px[0], py[0], px[sa], py[sa], px[sb], py[sb]};
          const double c[6] = {qx[0], qy[0], qx[ca], qy[ca], qx[cb], qy[cb]};
          if (fmax(fmax(s[0], s[2]), s[4]) < fmin(fmin(c[0], c[2]), c[4]) ||
              fmax(fmax(c[0], c[2]), c[4]) < fmin(fmin(s[0], s[2]), s[4]) ||
              fmax(fmax(s[1], s[3]), s[5]) < fmin(fmin(c[1], c[3]), c[5]) ||
              fmax(fmax(c[1], c[3]), c[5]) < fmin(fmin(s[1], s[3]), s[5]))
            continue;
          const double a = triangle_overlap<PV_MAX>(s, c, x0, y0, x1, y1);
          acc += (os > 0.0) == (oc > 0.0) ? a : -a;
        }
        for (int step = PV_MAX / 2; step > 0; step >>= 1) acc += __shfl_xor(acc, step);
        if (lane == 0) {
          const double a = fabs(acc);
          inter[ng * D + base + src] = a;
          iou[ng * D + base + src] = a / (ga + det_area[nd] - a);
        }
      }
    }
  }
}

static inline int quad_grid(long long n, int block) {
  const long long b = (n + block - 1) / block;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_quad_iou(const double* gt, const int* gt_count, const double* det, const int* det_count, int N, int G, int D,
                int* gt_valid, int* det_valid, double* gt_area, double* det_area, double* inter, double* iou,
                hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && G >= 0 && D >= 0, "mr_quad_iou: bad shape N=%d G=%d D=%d", N, G, D);
  if (N == 0 || G + D == 0) return MR_OK;
  hipLaunchKernelGGL(quad_prep_kernel, dim3(quad_grid((long long)N * (G + D), 256)), dim3(256), 0, stream, gt, gt_count, det,
                     det_count, N, G, D, gt_valid, det_valid, gt_area, det_area);
  if (G > 0 && D > 0)
    hipLaunchKernelGGL(quad_pair_kernel, dim3(quad_grid((long long)N * G * D, QP_THREADS)), dim3(QP_THREADS), 0, stream, gt,
                       det, N, G, D, gt_valid, det_valid, gt_area, det_area, inter, iou);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_poly_iou(const double* gt, const int* gt_verts, const int* gt_count, const double* det, const int* det_verts,
                const int* det_count, int N, int G, int D, int V, int* gt_valid, int* det_valid, double* gt_area,
                double* det_area, double* inter, double* iou, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && G >= 0 && D >= 0 && V >= 3, "mr_poly_iou: bad shape N=%d G=%d D=%d V=%d", N, G, D, V);
  if (V > PV_MAX) {
    set_error("mr_poly_iou: V=%d padded vertices exceed the %d (MR_POLY_MAX_VERTS) a wavefront holds", V, PV_MAX);
    return MR_ERR_UNSUPPORTED;
  }
  if (N == 0 || G + D == 0) return MR_OK;
  const long long slots = (long long)N * (G + D), rows = (long long)N * G;
  hipLaunchKernelGGL(poly_prep_kernel, dim3((unsigned)(slots < 65536 ? slots : 65536)), dim3(PV_MAX), 0, stream, gt, gt_verts,
                     gt_count, det, det_verts, det_count, N, G, D, V, gt_valid, det_valid, gt_area, det_area);
  if (G > 0 && D > 0)
    hipLaunchKernelGGL(poly_pair_kernel, dim3((unsigned)(rows < 65536 ? rows : 65536), PP_SPLIT), dim3(PV_MAX), 0, stream, gt, gt_verts,
                       det, det_verts, N, G, D, V, gt_valid, det_valid, gt_area, det_area, inter, iou);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

int mr_quad_match(const int* gt_valid, const int* det_valid, const int* gt_ignore, const double* det_area, const double* inter,
                  const double* iou, int N, int G, int D, double iou_constraint, double area_precision_constraint, int* counts,
                  double* scores, int* match_det, int* gt_dontcare, int* det_dontcare, hipStream_t stream) {
  MR_CHECK_ARG(N >= 0 && G >= 0 && D >= 0, "mr_quad_match: bad shape N=%d G=%d D=%d", N, G, D);
  if (G > QM_MAX || D > QM_MAX) {
    set_error("mr_quad_match: G=%d / D=%d quads per image exceed the %d the matching kernel holds", G, D, QM_MAX);
    return MR_ERR_UNSUPPORTED;
  }
  if (N == 0) return MR_OK;
  hipLaunchKernelGGL(quad_match_kernel, dim3(N), dim3(64), 0, stream, gt_valid, det_valid, gt_ignore, det_area, inter, iou, G, D,
                     iou_constraint, area_precision_constraint, counts, scores, match_det, gt_dontcare, det_dontcare);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
