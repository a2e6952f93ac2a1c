// DB (differentiable binarization) detector post-processing: the per-pixel stages on the GPU.
// Replaces the cv2 calls of structure/representers/seg_detector_representer.py:63-168 (`boxes_from_bitmap`):
//   cv2.findContours(bitmap)           -> connected components (8-connectivity) by union-find, then the RUN END POINTS of
//                                         every component (the only pixels that can be convex-hull vertices), compacted
//                                         into a list the host turns into min-area rectangles (cv2.minAreaRect);
//   box_score_fast (fillPoly + mean)   -> mean of the probability map over the pixels inside each candidate box.
// The geometry on a few hundred hull points per image (hull, rotating calipers, unclip, ordering) is O(components), not O(pixels).
// It runs on the host (megreader_amd/structure/db_geometry.py) between mr_db_components and mr_db_box_scores, or -- second half of
// this file -- on the device behind the same labelling: mr_db_boxes, the whole of `boxes_from_bitmap` without a host synchronisation.
// HBM-bound on one H x W map per image (640 x 640 = 1.6 MB f32): a few microseconds of traffic, launch-latency-bound.
#include <limits.h>

#include "common.h"
#include "../../include/megreader_hip.h"

namespace mr {

__device__ __forceinline__ int cc_find(const int* __restrict__ L, int a) {
  int p = L[a];
  while (p != a) {
    a = p;
    p = L[a];
  }
  return a;
}

// lock-free union by smaller root index (Playne & Hawick style): the root of a component ends up its raster-first pixel
__device__ __forceinline__ void cc_union(int* __restrict__ L, int a, int b) {
  while (true) {
    a = cc_find(L, a);
    b = cc_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);      // hang the larger root under the smaller one
    if (old == a) return;
    a = old;                                   // somebody re-rooted a meanwhile: retry from there
  }
}

// labels[n][p] = p (image-local pixel index) where prob > thresh, else -1
__global__ void db_cc_init_kernel(const float* __restrict__ prob, float thresh, int* __restrict__ labels,
                                  long long total, int hw) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x)
    labels[i] = prob[i] > thresh ? (int)(i % hw) : -1;
}

// union every foreground pixel with its already-visited 8-neighbours (W, NW, N, NE)
__global__ void db_cc_merge_kernel(int* __restrict__ labels, int N, int H, int W) {
  const long long total = (long long)N * H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int hw = H * W;
    const int n = (int)(i / hw), p = (int)(i - (long long)n * hw);
    int* L = labels + (long long)n * hw;
    if (L[p] < 0) continue;
    const int y = p / W, x = p - y * W;
    if (x > 0 && L[p - 1] >= 0) cc_union(L, p, p - 1);
    if (y > 0) {
      if (L[p - W] >= 0) cc_union(L, p, p - W);
      if (x > 0 && L[p - W - 1] >= 0) cc_union(L, p, p - W - 1);
      if (x < W - 1 && L[p - W + 1] >= 0) cc_union(L, p, p - W + 1);
    }
  }
}

// flatten + emit the run end points: pixel p is listed when its left or right neighbour is not foreground.
// points[k] = (image n, root, x, y); *count is advanced atomically (wave-aggregated); entries beyond `cap` are dropped
// (the count still says how many there were).
__global__ void db_cc_points_kernel(int* __restrict__ labels, int N, int H, int W, int4* __restrict__ points,
                                    int* __restrict__ count, int cap) {
  const long long total = (long long)N * H * W;
  const long long rounds = (total + (long long)gridDim.x * blockDim.x - 1) / ((long long)gridDim.x * blockDim.x);
  for (long long r = 0; r < rounds; ++r) {
    const long long i = r * (long long)gridDim.x * blockDim.x + blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool emit = false;
    int n = 0, x = 0, y = 0, root = -1;
    if (i < total) {
      const int hw = H * W;
      n = (int)(i / hw);
      const int p = (int)(i - (long long)n * hw);
      int* L = labels + (long long)n * hw;
      if (L[p] >= 0) {
        root = cc_find(L, p);
        y = p / W;
        x = p - y * W;
        emit = x == 0 || x == W - 1 || L[p - 1] < 0 || L[p + 1] < 0;
      }
    }
    // all neighbours' labels were read before anybody writes the flattened one? not needed: cc_find tolerates both
    const unsigned long long m = __ballot(emit);
    if (m) {
      const int lane = threadIdx.x & 63;
      int base = 0;
      if (lane == __ffsll((long long)m) - 1) base = atomicAdd(count, __popcll(m));
      base = __shfl(base, __ffsll((long long)m) - 1, 64);
      if (emit) {
        const int k = base + __popcll(m & ((1ull << lane) - 1ull));
        if (k < cap) points[k] = make_int4(n, root, x, y);
      }
    }
    if (i < total && root >= 0) labels[i] = root;   // flattened label (a root keeps itself; others point at a root)
  }
}

// sum of prob and pixel count inside (or on the border of) one convex quadrilateral, by the 256 threads of a workgroup; every
// thread returns the totals.  rs / rc: 4 floats of LDS each.  ONE body for db_box_score_kernel and db_boxes_kernel: the order of
// the additions (256 strided threads, wave_sum, four partials left to right) is the same, so are the bits.
__device__ __forceinline__ void box_score_sums(const float* __restrict__ pm, int H, int W, const float (&vx)[4],
                                               const float (&vy)[4], float* rs, float* rc, float& sum, float& cnt) {
  float xmin = 1e30f, xmax = -1e30f, ymin = 1e30f, ymax = -1e30f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    xmin = fminf(xmin, vx[k]); xmax = fmaxf(xmax, vx[k]);
    ymin = fminf(ymin, vy[k]); ymax = fmaxf(ymax, vy[k]);
  }
  const int x0 = max(0, (int)floorf(xmin)), x1 = min(W - 1, (int)ceilf(xmax));
  const int y0 = max(0, (int)floorf(ymin)), y1 = min(H - 1, (int)ceilf(ymax));
  // orientation of the vertex order (sign of twice the area)
  float area2 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) area2 += vx[k] * vy[(k + 1) & 3] - vx[(k + 1) & 3] * vy[k];
  const float sgn = area2 >= 0.f ? 1.f : -1.f;
  float s = 0.f, c = 0.f;
  const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
  for (int t = threadIdx.x; t < bw * bh; t += 256) {
    const int y = y0 + t / bw, x = x0 + t % bw;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float ex = vx[(k + 1) & 3] - vx[k], ey = vy[(k + 1) & 3] - vy[k];
      in &= sgn * (ex * ((float)y - vy[k]) - ey * ((float)x - vx[k])) >= 0.f;
    }
    if (in) {
      s += pm[(long long)y * W + x];
      c += 1.f;
    }
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rc[threadIdx.x >> 6] = c; }
  __syncthreads();
  sum = rs[0] + rs[1] + rs[2] + rs[3];
  cnt = rc[0] + rc[1] + rc[2] + rc[3];
}

// mean of prob inside (or on the border of) each convex quadrilateral: one workgroup per box.
// boxes: [B][9] floats = image index, then 4 vertices (x, y) in order around the quad.  out: [B][2] = sum, count.
__global__ __launch_bounds__(256) void db_box_score_kernel(const float* __restrict__ prob, int H, int W,
                                                            const float* __restrict__ boxes, float* __restrict__ out) {
  const float* b = boxes + (long long)blockIdx.x * 9;
  const int n = (int)b[0];
  float vx[4], vy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    vx[k] = b[1 + 2 * k];
    vy[k] = b[2 + 2 * k];
  }
  __shared__ float rs[4], rc[4];
  float s, c;
  box_score_sums(prob + (long long)n * H * W, H, W, vx, vy, rs, rc, s, c);
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = s;
    out[2 * blockIdx.x + 1] = c;
  }
}

static inline int grid_for(long long n, int block, int max_blocks = 4096) {
  const long long b = (n + block - 1) / block;
  return (int)(b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

}  // namespace mr

// ---- Boxes on the device (mr_db_boxes): everything `SegDetectorRepresenter.boxes_from_bitmap` does after the labelling --------
// candidates = the first K components in raster order of their root; per candidate and image row the extreme x (every hull
// vertex of a pixel set is the left-most or right-most pixel of its row); then ONE workgroup per (image, candidate) restates
// megreader_amd/structure/db_geometry.py operation for operation in float64: hull, calipers with the host's sequential choice,
// `mini_box` order, box score (box_score_sums above), unclip, second `mini_box`, scaling.  Integer atomics only: the same bits
// every run.
// float64 expressions must round like the host's Python floats: no fused multiply-add from here on.
#pragma clang fp contract(off)

namespace mr {

constexpr int DBX_MAX_H = 2048;     // 2 H points of 8 bytes + three 2 H index stacks of 2 bytes in LDS
constexpr int DBX_MAX_K = 1024;
// slot status
constexpr int DBX_NONE = 0, DBX_SHORT = 1, DBX_WEAK = 2, DBX_SMALL = 3, DBX_KEPT = 4;

// one wavefront per image row: flatten the labels (labels[p] = root) and count the row's roots (labels[p] == p)
__global__ __launch_bounds__(256) void db_row_roots_kernel(int* __restrict__ labels, int rows, int H, int W,
                                                            int* __restrict__ rowcnt) {
  const int lane = threadIdx.x & 63;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
    const int y = row % H;
    int* L = labels + (long long)(row / H) * H * W;
    int cnt = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
      const int x = x0 + lane, p = y * W + x;
      bool isroot = false;
      if (x < W && L[p] >= 0) {
        const int root = cc_find(L, p);
        L[p] = root;
        isroot = root == p;
      }
      cnt += __popcll(__ballot(isroot));
    }
    if (lane == 0) rowcnt[row] = cnt;
  }
}

// one workgroup per image: rowcnt[H] -> exclusive prefix in place (rank of the row's first root), comps[n] = number of components
__global__ __launch_bounds__(256) void db_row_scan_kernel(int* __restrict__ rowcnt, int H, int* __restrict__ comps) {
  __shared__ int wsum[4];
  int* r = rowcnt + (long long)blockIdx.x * H;
  const int per = (H + 255) / 256, lo = min(H, (int)threadIdx.x * per), hi = min(H, lo + per);
  int s = 0;
  for (int y = lo; y < hi; ++y) s += r[y];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = inc - s;
  for (int i = 0; i < w; ++i) base += wsum[i];
  for (int y = lo; y < hi; ++y) {
    const int c = r[y];
    r[y] = base;
    base += c;
  }
  if (threadIdx.x == 255) comps[blockIdx.x] = base;
}

// one wavefront per image row: rank[root pixel] = raster rank of the component among its image's (prefix of the row + ballot)
__global__ __launch_bounds__(256) void db_root_rank_kernel(const int* __restrict__ labels, int rows, int H, int W,
                                                            const int* __restrict__ rowbase, int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
    const long long img = (long long)(row / H) * H * W;
    const int y = row % H;
    int base = rowbase[row];
    for (int x0 = 0; x0 < W; x0 += 64) {
      const int x = x0 + lane, p = y * W + x;
      const bool isroot = x < W && labels[img + p] == p;
      const unsigned long long m = __ballot(isroot);
      if (isroot) rank[img + p] = base + __popcll(m & ((1ull << lane) - 1ull));
      base += __popcll(m);
    }
  }
}

__global__ void db_extremes_fill_kernel(int2* __restrict__ ext, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    ext[i] = make_int2(INT_MAX, -1);
}

// ext[n][k][y] = (min x, max x) of candidate k in row y: only run end points can be extremes, only they touch the table
__global__ void db_extremes_kernel(const int* __restrict__ labels, const int* __restrict__ rank, int N, int H, int W, int K,
                                   int* __restrict__ ext) {
  const long long total = (long long)N * H * W;
  const int hw = H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int root = labels[i];
    if (root < 0) continue;
    const int n = (int)(i / hw), p = (int)(i - (long long)n * hw);
    const int y = p / W, x = p - y * W;
    const bool left = x == 0 || labels[i - 1] < 0, right = x == W - 1 || labels[i + 1] < 0;
    if (!left && !right) continue;
    const int k = rank[(long long)n * hw + root];
    if (k >= K) continue;
    int* e = ext + (((long long)n * K + k) * H + y) * 2;
    if (left) atomicMin(e, x);
    if (right) atomicMax(e + 1, x);
  }
}

// LDS of db_boxes_kernel, all of it dynamic (offsets in bytes; every double 8-aligned)
constexpr int DBX_AREA = 0;                       // double[256] areas of one round of hull edges
constexpr int DBX_RECT = DBX_AREA + 256 * 8;      // double[8]   x0, y0, ux, uy, lo_u, hi_u, lo_v, hi_v of the chosen edge
constexpr int DBX_TMP = DBX_RECT + 64;            // double[8]   corners sorted by x
constexpr int DBX_BOX = DBX_TMP + 64;             // double[8]   ordered box of the candidate
constexpr int DBX_BOX2 = DBX_BOX + 64;            // double[8]   ordered box after unclip
constexpr int DBX_SP = DBX_BOX2 + 64;             // double[8]   the 4 unclipped points, sorted
constexpr int DBX_LO = DBX_SP + 64;               // double[8]   lower chain
constexpr int DBX_UP = DBX_LO + 64;               // double[8]   upper chain
constexpr int DBX_H2 = DBX_UP + 64;               // double[8]   their hull
constexpr int DBX_VAL = DBX_H2 + 64;              // double[8]   short sides
constexpr int DBX_KEY = DBX_VAL + 64;             // u64[2]      smallest (x, y) key of the hull
constexpr int DBX_MISC = DBX_KEY + 16;            // int[8]
constexpr int DBX_RS = DBX_MISC + 32;             // float[4] + float[4]
constexpr int DBX_PTS = DBX_RS + 32;              // int2[2 H], then three unsigned short [2 H]
enum { DBX_PICK = 0, DBX_YMIN, DBX_YMAX, DBX_LA, DBX_LB, DBX_START, DBX_H2N };
static inline int dbx_lds_bytes(int H) { return DBX_PTS + 2 * H * 8 + 3 * 2 * H * 2; }

// half of a monotone chain over pts[0..m) (forward or backward), strict turns; st receives indices into pts
__device__ __forceinline__ int dbx_chain(const int2* pts, int m, bool backward, unsigned short* st) {
  int len = 0;
  for (int i = 0; i < m; ++i) {
    const int idx = backward ? m - 1 - i : i;
    const int2 p = pts[idx];
    if (p.x == INT_MAX) continue;                       // (a row without pixels: cannot happen inside a component)
    if (len > 0) {
      const int2 t = pts[st[len - 1]];
      if (t.x == p.x && t.y == p.y) continue;
    }
    while (len >= 2) {
      const int2 o = pts[st[len - 2]], a = pts[st[len - 1]];
      const long long cross = (long long)(a.x - o.x) * (p.y - o.y) - (long long)(a.y - o.y) * (p.x - o.x);
      if (cross > 0) break;
      --len;
    }
    st[len++] = (unsigned short)idx;
  }
  return len;
}

struct DbxIntHull {          // hull vertex i of the candidate, host order
  const int2* pts;
  const unsigned short* hull;
  __device__ __forceinline__ void operator()(int i, double& x, double& y) const {
    const int2 p = pts[hull[i]];
    x = (double)p.x;
    y = (double)p.y;
  }
};
struct DbxDblHull {          // hull vertex i of the unclipped rectangle
  const double* h;
  __device__ __forceinline__ void operator()(int i, double& x, double& y) const {
    x = h[2 * i];
    y = h[2 * i + 1];
  }
};

// db_geometry.min_area_rect for a hull of h >= 3 vertices: the areas of 256 edges at a time in parallel, the host's sequential
// choice (`area < best - 1e-12`, in hull order) by thread 0; the thread that owns the chosen edge leaves its frame in rect
template <class P>
__device__ __forceinline__ void dbx_calipers(const P& pt, int h, double* area, int* pick, double* rect) {
  double best = 0.0;
  bool have = false;
  for (int r0 = 0; r0 < h; r0 += 256) {
    const int i = r0 + (int)threadIdx.x;
    double x0 = 0, y0 = 0, ux = 0, uy = 0, lo_u = 0, hi_u = 0, lo_v = 0, hi_v = 0;
    if (i < h) {
      double x1, y1;
      pt(i, x0, y0);
      pt(i + 1 == h ? 0 : i + 1, x1, y1);
      const double ex = x1 - x0, ey = y1 - y0;
      const double ln = sqrt(ex * ex + ey * ey);
      double a = __builtin_nan("");                     // ln == 0: the host skips the edge
      if (ln != 0.0) {
        ux = ex / ln;
        uy = ey / ln;
        for (int j = 0; j < h; ++j) {
          double px, py;
          pt(j, px, py);
          const double pu = (px - x0) * ux + (py - y0) * uy;
          const double pv = -(px - x0) * uy + (py - y0) * ux;
          if (j == 0) {
            lo_u = hi_u = pu;
            lo_v = hi_v = pv;
          } else {
            lo_u = pu < lo_u ? pu : lo_u;
            hi_u = pu > hi_u ? pu : hi_u;
            lo_v = pv < lo_v ? pv : lo_v;
            hi_v = pv > hi_v ? pv : hi_v;
          }
        }
        a = (hi_u - lo_u) * (hi_v - lo_v);
      }
      area[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int p = -1;
      const int m = min(256, h - r0);
      for (int t = 0; t < m; ++t) {
        const double a = area[t];
        if (a != a) continue;
        if (!have || a < best - 1e-12) {
          best = a;
          have = true;
          p = t;
        }
      }
      *pick = p;
    }
    __syncthreads();
    if ((int)threadIdx.x == *pick) {
      rect[0] = x0; rect[1] = y0; rect[2] = ux; rect[3] = uy;
      rect[4] = lo_u; rect[5] = hi_u; rect[6] = lo_v; rect[7] = hi_v;
    }
  }
  __syncthreads();
}

// thread 0: `mini_box` of a hull of h vertices whose frame (h >= 3) is in rect: the ordered corners -> box[8]; returns min(sides)
template <class P>
__device__ __forceinline__ double dbx_mini_box(const P& pt, int h, const double* rect, double* tmp, double* box) {
  double cx[4], cy[4], sa, sb;
  if (h == 1) {
    double x, y;
    pt(0, x, y);
    cx[0] = cx[1] = cx[2] = cx[3] = x;
    cy[0] = cy[1] = cy[2] = cy[3] = y;
    sa = 0.0; sb = 0.0;
  } else if (h == 2) {
    double ax, ay, bx, by;
    pt(0, ax, ay);
    pt(1, bx, by);
    cx[0] = ax; cy[0] = ay; cx[1] = bx; cy[1] = by; cx[2] = bx; cy[2] = by; cx[3] = ax; cy[3] = ay;
    const double ex = bx - ax, ey = by - ay;
    sa = sqrt(ex * ex + ey * ey); sb = 0.0;
  } else {
    const double x0 = rect[0], y0 = rect[1], ux = rect[2], uy = rect[3];
    const double lo_u = rect[4], hi_u = rect[5], lo_v = rect[6], hi_v = rect[7];
    cx[0] = x0 + lo_u * ux - lo_v * uy; cy[0] = y0 + lo_u * uy + lo_v * ux;
    cx[1] = x0 + hi_u * ux - lo_v * uy; cy[1] = y0 + hi_u * uy + lo_v * ux;
    cx[2] = x0 + hi_u * ux - hi_v * uy; cy[2] = y0 + hi_u * uy + hi_v * ux;
    cx[3] = x0 + lo_u * ux - hi_v * uy; cy[3] = y0 + lo_u * uy + hi_v * ux;
    sa = hi_u - lo_u; sb = hi_v - lo_v;
  }
  // stable sort by x: the position of corner i is the number of corners in front of it
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r += (cx[j] < cx[i] || (cx[j] == cx[i] && j < i)) ? 1 : 0;
    tmp[2 * r] = cx[i];
    tmp[2 * r + 1] = cy[i];
  }
  const bool a = tmp[3] > tmp[1], b = tmp[7] > tmp[5];
  const int i1 = a ? 0 : 1, i4 = a ? 1 : 0, i2 = b ? 2 : 3, i3 = b ? 3 : 2;
  box[0] = tmp[2 * i1]; box[1] = tmp[2 * i1 + 1];
  box[2] = tmp[2 * i2]; box[3] = tmp[2 * i2 + 1];
  box[4] = tmp[2 * i3]; box[5] = tmp[2 * i3 + 1];
  box[6] = tmp[2 * i4]; box[7] = tmp[2 * i4 + 1];
  return sb < sa ? sb : sa;
}

// thread 0: db_geometry.unclip(box) -> db_geometry.convex_hull of the four points -> h2 (LDS); returns the number of vertices
__device__ __forceinline__ int dbx_unclip_hull(const double* box, double* sp, double* lo, double* up, double* h2) {
  double qx[4], qy[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { qx[i] = box[2 * i]; qy[i] = box[2 * i + 1]; }
  double ex = qx[1] - qx[0], ey = qy[1] - qy[0], fx = qx[3] - qx[0], fy = qy[3] - qy[0];
  double a = sqrt(ex * ex + ey * ey), b = sqrt(fx * fx + fy * fy);
  if (a != 0.0 && b != 0.0) {
    const double d = a * b * 1.5 / (2.0 * (a + b));
#pragma unroll
    for (int i = 0; i < 4; ++i) { qx[i] = (double)(int)qx[i]; qy[i] = (double)(int)qy[i]; }   // pyclipper: integer coordinates
    ex = qx[1] - qx[0]; ey = qy[1] - qy[0]; fx = qx[3] - qx[0]; fy = qy[3] - qy[0];
    a = sqrt(ex * ex + ey * ey); b = sqrt(fx * fx + fy * fy);
    if (a != 0.0 && b != 0.0) {
      const double ux = ex / a, uy = ey / a, vx = fx / b, vy = fy / b;
      const double su[4] = {-1.0, 1.0, 1.0, -1.0}, sv[4] = {-1.0, -1.0, 1.0, 1.0};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double nx = qx[i] + d * (su[i] * ux + sv[i] * vx), ny = qy[i] + d * (su[i] * uy + sv[i] * vy);
        qx[i] = nx;
        qy[i] = ny;
      }
    }
  }
  // sorted(set(points)): position by (x, y), equal points side by side, then dropped
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      r += (qx[j] < qx[i] || (qx[j] == qx[i] && (qy[j] < qy[i] || (qy[j] == qy[i] && j < i)))) ? 1 : 0;
    lo[2 * r] = qx[i];
    lo[2 * r + 1] = qy[i];
  }
  int m = 0;
  for (int i = 0; i < 4; ++i) {
    if (m > 0 && sp[2 * m - 2] == lo[2 * i] && sp[2 * m - 1] == lo[2 * i + 1]) continue;
    sp[2 * m] = lo[2 * i];
    sp[2 * m + 1] = lo[2 * i + 1];
    ++m;
  }
  if (m <= 2) {
    for (int i = 0; i < 2 * m; ++i) h2[i] = sp[i];
    return m;
  }
  int nl = 0, nu = 0;
  for (int i = 0; i < m; ++i) {
    const double px = sp[2 * i], py = sp[2 * i + 1];
    while (nl >= 2 && (lo[2 * nl - 2] - lo[2 * nl - 4]) * (py - lo[2 * nl - 3]) -
                              (lo[2 * nl - 1] - lo[2 * nl - 3]) * (px - lo[2 * nl - 4]) <= 0.0)
      --nl;
    lo[2 * nl] = px;
    lo[2 * nl + 1] = py;
    ++nl;
  }
  for (int i = m - 1; i >= 0; --i) {
    const double px = sp[2 * i], py = sp[2 * i + 1];
    while (nu >= 2 && (up[2 * nu - 2] - up[2 * nu - 4]) * (py - up[2 * nu - 3]) -
                              (up[2 * nu - 1] - up[2 * nu - 3]) * (px - up[2 * nu - 4]) <= 0.0)
      --nu;
    up[2 * nu] = px;
    up[2 * nu + 1] = py;
    ++nu;
  }
  int h = 0;
  for (int i = 0; i < nl - 1; ++i, ++h) { h2[2 * h] = lo[2 * i]; h2[2 * h + 1] = lo[2 * i + 1]; }
  for (int i = 0; i < nu - 1; ++i, ++h) { h2[2 * h] = up[2 * i]; h2[2 * h + 1] = up[2 * i + 1]; }
  return h;
}

// one workgroup per (image, candidate slot).  Writes the slot's status, and for a kept box its scaled corners and score into the
// staging arrays that db_boxes_compact_kernel packs; cand / cand_sums / status_out are the optional per-slot outputs.
__global__ __launch_bounds__(256) void db_boxes_kernel(const float* __restrict__ prob, int H, int W, int K,
                                                        const int* __restrict__ comps, const int2* __restrict__ ext,
                                                        const int* __restrict__ dest, double box_thresh, double min_size,
                                                        double* __restrict__ sbox, float* __restrict__ sscore,
                                                        int* __restrict__ status, double* __restrict__ cand,
                                                        float* __restrict__ cand_sums, int* __restrict__ status_out,
                                                        double* __restrict__ kept_cand) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* area = (double*)(lds + DBX_AREA);
  double* rect = (double*)(lds + DBX_RECT);
  double* tmp = (double*)(lds + DBX_TMP);
  double* box = (double*)(lds + DBX_BOX);
  double* box2 = (double*)(lds + DBX_BOX2);
  double* val = (double*)(lds + DBX_VAL);
  unsigned long long* key = (unsigned long long*)(lds + DBX_KEY);
  int* misc = (int*)(lds + DBX_MISC);
  float* rs = (float*)(lds + DBX_RS);
  int2* pts = (int2*)(lds + DBX_PTS);
  unsigned short* stA = (unsigned short*)(pts + 2 * H);
  unsigned short* stB = stA + 2 * H;
  unsigned short* hull = stB + 2 * H;

  const int tid = threadIdx.x;
  const long long slot = blockIdx.x;
  const int n = (int)(slot / K);
  if (tid < 8 && cand != nullptr) cand[slot * 8 + tid] = 0.0;
  if (tid < 2 && cand_sums != nullptr) cand_sums[slot * 2 + tid] = 0.f;
  auto finish = [&](int st) {
    if (tid == 0) {
      status[slot] = st;
      if (status_out != nullptr) status_out[slot] = st;
    }
  };
  if ((int)(slot - (long long)n * K) >= comps[n]) {
    finish(DBX_NONE);
    return;
  }
  // rows of the candidate (an 8-connected component occupies consecutive rows)
  const int2* e = ext + slot * H;
  if (tid == 0) {
    misc[DBX_YMIN] = INT_MAX;
    misc[DBX_YMAX] = -1;
    key[0] = ~0ull;
  }
  __syncthreads();
  {
    int lo = INT_MAX, hi = -1;
    for (int y = tid; y < H; y += 256)
      if (e[y].y >= 0) {
        lo = min(lo, y);
        hi = max(hi, y);
      }
    if (hi >= 0) {
      atomicMin(&misc[DBX_YMIN], lo);
      atomicMax(&misc[DBX_YMAX], hi);
    }
  }
  __syncthreads();
  const int ymin = misc[DBX_YMIN], nrows = misc[DBX_YMAX] - ymin + 1;
  if (nrows <= 0) {                                     // (a ranked component has at least its root pixel)
    finish(DBX_NONE);
    return;
  }
  // points in (y ascending, x descending) order: a monotone chain over them with strict left turns walks the hull in the
  // orientation of db_geometry.convex_hull (the same cross products, all integers), from the top row's right-most pixel
  const int m = 2 * nrows;
  for (int j = tid; j < nrows; j += 256) {
    const int2 v = e[ymin + j];
    const bool ok = v.y >= 0;
    pts[2 * j] = make_int2(ok ? v.y : INT_MAX, ymin + j);
    pts[2 * j + 1] = make_int2(ok ? v.x : INT_MAX, ymin + j);
  }
  __syncthreads();
  if (tid == 0) misc[DBX_LA] = dbx_chain(pts, m, false, stA);
  if (tid == 64) misc[DBX_LB] = dbx_chain(pts, m, true, stB);
  __syncthreads();
  const int la = misc[DBX_LA], lb = misc[DBX_LB];
  const int h = la <= 1 ? 1 : la + lb - 2;
  // convex_hull starts at the smallest (x, y): rotate
  {
    unsigned long long mine = ~0ull;
    for (int i = tid; i < h; i += 256) {
      const int2 p = pts[i < la - 1 || la <= 1 ? stA[i] : stB[i - (la - 1)]];
      const unsigned long long kk = ((unsigned long long)(unsigned)p.x << 32) | (unsigned)p.y;
      mine = kk < mine ? kk : mine;
    }
    if (mine != ~0ull) atomicMin(&key[0], mine);
    __syncthreads();
    const unsigned long long least = key[0];
    for (int i = tid; i < h; i += 256) {
      const int2 p = pts[i < la - 1 || la <= 1 ? stA[i] : stB[i - (la - 1)]];
      if ((((unsigned long long)(unsigned)p.x << 32) | (unsigned)p.y) == least) misc[DBX_START] = i;
    }
    __syncthreads();
    const int start = misc[DBX_START];
    for (int i = tid; i < h; i += 256) {
      const int to = i - start + (i < start ? h : 0);
      hull[to] = i < la - 1 || la <= 1 ? stA[i] : stB[i - (la - 1)];
    }
    __syncthreads();
  }
  const DbxIntHull P1{pts, hull};
  if (h >= 3) dbx_calipers(P1, h, area, &misc[DBX_PICK], rect);
  if (tid == 0) val[0] = dbx_mini_box(P1, h, rect, tmp, box);
  __syncthreads();
  if (tid < 8 && cand != nullptr) cand[slot * 8 + tid] = box[tid];
  if (tid < 8) kept_cand[slot * 8 + tid] = box[tid];    // stays in ws for mr_db_ribbons (read where the status is kept)
  if (val[0] < min_size) {
    finish(DBX_SHORT);
    return;
  }
  // box_score_fast: corners truncated toward zero
  float vx[4], vy[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    vx[i] = (float)(int)box[2 * i];
    vy[i] = (float)(int)box[2 * i + 1];
  }
  float s, c;
  box_score_sums(prob + (long long)n * H * W, H, W, vx, vy, rs, rs + 4, s, c);
  if (tid == 0 && cand_sums != nullptr) {
    cand_sums[slot * 2] = s;
    cand_sums[slot * 2 + 1] = c;
  }
  const double score = c > 0.f ? (double)s / (double)c : 0.0;
  if (box_thresh > score) {
    finish(DBX_WEAK);
    return;
  }
  double* h2 = (double*)(lds + DBX_H2);
  if (tid == 0)
    misc[DBX_H2N] = dbx_unclip_hull(box, (double*)(lds + DBX_SP), (double*)(lds + DBX_LO), (double*)(lds + DBX_UP), h2);
  __syncthreads();
  const int h2n = misc[DBX_H2N];
  const DbxDblHull P2{h2};
  if (h2n >= 3) dbx_calipers(P2, h2n, area, &misc[DBX_PICK], rect);
  if (tid == 0) val[1] = dbx_mini_box(P2, h2n, rect, tmp, box2);
  __syncthreads();
  if (val[1] < min_size + 2.0) {
    finish(DBX_SMALL);
    return;
  }
  if (tid < 8) {
    const double full = (double)((tid & 1) ? H : W), to = (double)dest[2 * n + (tid & 1)];
    double v = rint(box2[tid] / full * to);
    v = v < 0.0 ? 0.0 : (v > to ? to : v);
    sbox[slot * 8 + tid] = v;
  }
  if (tid == 0) sscore[slot] = (float)score;
  finish(DBX_KEPT);
}

// one workgroup per image: the kept slots in candidate order -> boxes / scores, their number -> count; the rest zero
__global__ __launch_bounds__(256) void db_boxes_compact_kernel(const int* __restrict__ status, const double* __restrict__ sbox,
                                                                const float* __restrict__ sscore, int K,
                                                                double* __restrict__ boxes, float* __restrict__ scores,
                                                                int* __restrict__ count) {
  __shared__ int wtot[4];
  const long long n0 = (long long)blockIdx.x * K;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int base = 0;
  for (int k0 = 0; k0 < K; k0 += 256) {
    const int k = k0 + (int)threadIdx.x;
    const bool keep = k < K && status[n0 + k] == DBX_KEPT;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wtot[w] = __popcll(m);
    __syncthreads();
    int off = base + __popcll(m & ((1ull << lane) - 1ull));
    for (int i = 0; i < w; ++i) off += wtot[i];
    if (keep) {
#pragma unroll
      for (int i = 0; i < 8; ++i) boxes[(n0 + off) * 8 + i] = sbox[(n0 + k) * 8 + i];
      scores[n0 + off] = sscore[n0 + k];
    }
    base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  for (int j = base + (int)threadIdx.x; j < K; j += 256) {
#pragma unroll
    for (int i = 0; i < 8; ++i) boxes[(n0 + j) * 8 + i] = 0.0;
    scores[n0 + j] = 0.f;
  }
  if (threadIdx.x == 0) count[blockIdx.x] = base;
}

// ---- Ribbons (mr_db_ribbons): the curve a kept candidate follows, from what mr_db_boxes left in its workspace -------------------
// One workgroup per (image, candidate slot), as db_boxes_kernel: two scans of the candidate's pixels between its row extremes
// (the count, then six exact integer sums per slab along the rectangle's long axis: LDS atomics on 64-bit integers, one table per
// wavefront, a thread flushes its sums when the slab changes), then one lane per slab / knot restates the rule of
// include/megreader_hip.h in float64.  No global atomics; the same bits every run.
constexpr int RB_NONE = 0, RB_SHORT = 1, RB_EMPTY = 2, RB_STEEP = 3, RB_FOLDED = 4;
constexpr int RB_S = MR_RIBBON_MAX_SLABS, RB_K = MR_RIBBON_MAX_KNOTS, RB_ROW = RB_K * 4;
enum { RB_BEFORE = 0, RB_TOTAL, RB_YMIN, RB_YMAX, RB_XMIN, RB_XMAX, RB_PIX, RB_SE, RB_FLAG };

__global__ __launch_bounds__(256) void db_ribbons_kernel(const int* __restrict__ labels, const int2* __restrict__ ext,
                                                          const int* __restrict__ status, const double* __restrict__ cand,
                                                          const int* __restrict__ dest, int H, int W, int K, int S, double ratio,
                                                          long long* __restrict__ sums, double* __restrict__ ribbons,
                                                          int* __restrict__ knots, int* __restrict__ why) {
  __shared__ unsigned long long acc[4][RB_S][6];
  __shared__ double mean[RB_S][2], cov[RB_S][3], tan_[RB_S][2], cosv[RB_S], half[RB_S];
  __shared__ double kc[RB_K][2], kt[RB_K][2], kh[RB_K], top[RB_K][2], bot[RB_K][2];
  __shared__ double geo[8];                             // o.x, o.y, e.x, e.y, sw, d
  __shared__ int misc[12];
  const int tid = threadIdx.x;
  const long long slot = blockIdx.x;
  const int n = (int)(slot / K), k = (int)(slot - (long long)n * K);
  if (tid < 12) misc[tid] = tid == RB_YMIN || tid == RB_XMIN ? INT_MAX : (tid == RB_YMAX || tid == RB_XMAX ? -1 : 0);
  for (int i = tid; i < 4 * RB_S * 6; i += 256) (&acc[0][0][0])[i] = 0ull;
  __syncthreads();
  // the row of this slot in the compacted order of db_boxes_compact_kernel, and how many rows the image has
  {
    int before = 0, total = 0;
    for (int j = tid; j < K; j += 256) {
      const int kept = status[(long long)n * K + j] == DBX_KEPT ? 1 : 0;
      total += kept;
      before += j < k ? kept : 0;
    }
    if (total) atomicAdd(&misc[RB_TOTAL], total);
    if (before) atomicAdd(&misc[RB_BEFORE], before);
  }
  __syncthreads();
  if (k >= misc[RB_TOTAL]) {                            // a row behind the last box: zeros
    for (int i = tid; i < RB_ROW; i += 256) ribbons[slot * RB_ROW + i] = 0.0;
    if (tid == 0) { knots[slot] = 0; why[slot] = RB_NONE; }
  }
  if (status[slot] != DBX_KEPT) return;
  const long long row = (long long)n * K + misc[RB_BEFORE];
  auto none = [&](int reason) {                         // (every thread of the workgroup comes here together)
    for (int i = tid; i < RB_ROW; i += 256) ribbons[row * RB_ROW + i] = 0.0;
    if (tid == 0) { knots[row] = 0; why[row] = reason; }
  };
  // rows and columns of the candidate; its label is its raster-first pixel: the left-most one of its first row
  const int2* e = ext + slot * H;
  {
    int ylo = INT_MAX, yhi = -1, xlo = INT_MAX, xhi = -1;
    for (int y = tid; y < H; y += 256) {
      const int2 v = e[y];
      if (v.y >= 0) {
        ylo = min(ylo, y); yhi = max(yhi, y);
        xlo = min(xlo, v.x); xhi = max(xhi, v.y);
      }
    }
    if (yhi >= 0) {
      atomicMin(&misc[RB_YMIN], ylo); atomicMax(&misc[RB_YMAX], yhi);
      atomicMin(&misc[RB_XMIN], xlo); atomicMax(&misc[RB_XMAX], xhi);
    }
  }
  __syncthreads();
  const int ymin = misc[RB_YMIN], nrows = misc[RB_YMAX] - ymin + 1, xmin = misc[RB_XMIN];
  if (nrows <= 0) {                                     // (a kept candidate has pixels)
    none(RB_SHORT);
    return;
  }
  const int root = ymin * W + e[ymin].x;
  const int* L = labels + (long long)n * H * W;
  const int chunks = (misc[RB_XMAX] - xmin) / 8 + 1;    // 8 pixels of one row per thread and step
  const long long items = (long long)nrows * chunks;
  {
    int cnt = 0;
    for (long long t = tid; t < items; t += 256) {
      const int r = (int)(t / chunks), y = ymin + r, c0 = xmin + (int)(t - (long long)r * chunks) * 8;
      const int2 v = e[y];                              // (a row without pixels holds (INT_MAX, -1): an empty range)
      const int x0 = max(c0, v.x), xe = min(c0 + 7, v.y);
      for (int x = x0; x <= xe; ++x) cnt += L[(long long)y * W + x] == root ? 1 : 0;
    }
    if (cnt) atomicAdd(&misc[RB_PIX], cnt);
  }
  __syncthreads();
  if (tid == 0) {                                       // 1. axis, 2. slabs
    const double* p = cand + slot * 8;
    const double ax = p[2] - p[0], ay = p[3] - p[1], bx = p[6] - p[0], by = p[7] - p[1];
    const double a = sqrt(ax * ax + ay * ay), b = sqrt(bx * bx + by * by);
    double ox, oy, ex, ey, len;
    if ((double)max((int)b, 1) > 1.5 * (double)max((int)a, 1)) {
      ox = p[2]; oy = p[3]; ex = (p[4] - p[2]) / b; ey = (p[5] - p[3]) / b; len = b;
    } else {
      ox = p[0]; oy = p[1]; ex = ax / a; ey = ay / a; len = a;
    }
    int se = 0;
    double sw = 0.0;
    if (len > 0.0) {
      const double tbar = (double)misc[RB_PIX] / (len + 1.0);
      se = min(S, (int)((len + 1.0) / fmax(4.0, tbar)));
      if (se >= 3) sw = (len + 1.0) / (double)se;
    }
    geo[0] = ox; geo[1] = oy; geo[2] = ex; geo[3] = ey; geo[4] = sw;
    misc[RB_SE] = se;
  }
  __syncthreads();
  const int se = misc[RB_SE];
  if (se < 3) {
    none(RB_SHORT);
    return;
  }
  const double ox = geo[0], oy = geo[1], ex = geo[2], ey = geo[3], sw = geo[4];
  // 3. moments
  {
    unsigned long long (*mine)[6] = acc[tid >> 6];
    for (long long t = tid; t < items; t += 256) {
      const int r = (int)(t / chunks), y = ymin + r, c0 = xmin + (int)(t - (long long)r * chunks) * 8;
      const int2 v = e[y];
      const int x0 = max(c0, v.x), xe = min(c0 + 7, v.y);
      int cur = -1;
      unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
      auto flush = [&]() {
        if (cur < 0) return;
        atomicAdd(&mine[cur][0], s0); atomicAdd(&mine[cur][1], s1); atomicAdd(&mine[cur][2], s2);
        atomicAdd(&mine[cur][3], s3); atomicAdd(&mine[cur][4], s4); atomicAdd(&mine[cur][5], s5);
      };
      for (int x = x0; x <= xe; ++x) {
        if (L[(long long)y * W + x] != root) continue;
        const double u = ((double)x - ox) * ex + ((double)y - oy) * ey;
        const double f = floor((u + 0.5) / sw);
        const int j = f >= (double)(se - 1) ? se - 1 : (f > 0.0 ? (int)f : 0);      // (a NaN falls to slab 0)
        if (j != cur) {
          flush();
          cur = j;
          s0 = s1 = s2 = s3 = s4 = s5 = 0;
        }
        const unsigned long long xx = (unsigned long long)x, yy = (unsigned long long)y;
        s0 += 1; s1 += xx; s2 += yy; s3 += xx * xx; s4 += xx * yy; s5 += yy * yy;
      }
      flush();
    }
  }
  __syncthreads();
  if (tid < se * 6) {
    const int j = tid / 6, q = tid - j * 6;
    const unsigned long long v = acc[0][j][q] + acc[1][j][q] + acc[2][j][q] + acc[3][j][q];
    acc[0][j][q] = v;
    sums[(slot * RB_S + j) * 6 + q] = (long long)v;
  }
  __syncthreads();
  if (tid < se) {
    const double cnt = (double)(long long)acc[0][tid][0];
    if (acc[0][tid][0] == 0ull) {
      atomicOr(&misc[RB_FLAG], 1);
    } else {
      const double mx = (double)(long long)acc[0][tid][1] / cnt, my = (double)(long long)acc[0][tid][2] / cnt;
      mean[tid][0] = mx; mean[tid][1] = my;
      cov[tid][0] = (double)(long long)acc[0][tid][3] / cnt - mx * mx;
      cov[tid][1] = (double)(long long)acc[0][tid][4] / cnt - mx * my;
      cov[tid][2] = (double)(long long)acc[0][tid][5] / cnt - my * my;
    }
  }
  __syncthreads();
  if (misc[RB_FLAG]) {
    none(RB_EMPTY);
    return;
  }
  const int l = se - 1, kn = se + 2;
  if (tid < se) {                                       // 4. tangents
    double tx, ty;
    if (tid == 0) {
      tx = -3.0 * mean[0][0] + 4.0 * mean[1][0] - mean[2][0];
      ty = -3.0 * mean[0][1] + 4.0 * mean[1][1] - mean[2][1];
    } else if (tid == l) {
      tx = 3.0 * mean[l][0] - 4.0 * mean[l - 1][0] + mean[l - 2][0];
      ty = 3.0 * mean[l][1] - 4.0 * mean[l - 1][1] + mean[l - 2][1];
    } else {
      tx = mean[tid + 1][0] - mean[tid - 1][0];
      ty = mean[tid + 1][1] - mean[tid - 1][1];
    }
    const double len = sqrt(tx * tx + ty * ty);
    tx = tx / len; ty = ty / len;
    const double c = tx * ex + ty * ey;
    if (!(c > 0.25)) atomicOr(&misc[RB_FLAG], 1);
    tan_[tid][0] = tx; tan_[tid][1] = ty; cosv[tid] = c;
    const double nx = -ty, ny = tx;                     // 5. half thickness
    const double var = nx * nx * cov[tid][0] + 2.0 * nx * ny * cov[tid][1] + ny * ny * cov[tid][2];
    half[tid] = (sqrt(12.0 * fmax(var, 0.0) + 1.0) - 1.0) / 2.0;
  }
  __syncthreads();
  if (misc[RB_FLAG]) {
    none(RB_STEEP);
    return;
  }
  if (tid < kn) {                                       // 6. knots
    const int j = min(max(tid - 1, 0), l), jh = min(max(j, 1), l - 1);
    const double tx = tan_[j][0], ty = tan_[j][1];
    double cx = mean[j][0], cy = mean[j][1];
    if (tid == 0) {
      const double back = (sw / 2.0) / cosv[0];
      cx = cx - tx * back; cy = cy - ty * back;
    } else if (tid == kn - 1) {
      const double on = (sw / 2.0) / cosv[l];
      cx = cx + tx * on; cy = cy + ty * on;
    }
    const double h = half[jh], nx = -ty, ny = tx;
    kc[tid][0] = cx; kc[tid][1] = cy; kt[tid][0] = tx; kt[tid][1] = ty; kh[tid] = h;
    top[tid][0] = cx - nx * h; top[tid][1] = cy - ny * h;
    bot[tid][0] = cx + nx * h; bot[tid][1] = cy + ny * h;
  }
  __syncthreads();
  if (tid == 0) {                                       // 7. unclip distance: shoelace area and perimeter of the outline
    double a2 = 0.0, per = 0.0;
    const int m = 2 * kn;
    for (int i = 0; i < m; ++i) {
      const int i1 = i + 1 == m ? 0 : i + 1;
      const double* p = i < kn ? top[i] : bot[m - 1 - i];
      const double* q = i1 < kn ? top[i1] : bot[m - 1 - i1];
      a2 = a2 + (p[0] * q[1] - q[0] * p[1]);
      const double dx = q[0] - p[0], dy = q[1] - p[1];
      per = per + sqrt(dx * dx + dy * dy);
    }
    geo[5] = fabs(a2) / 2.0 * ratio / per;
  }
  __syncthreads();
  if (tid < kn) {
    const double d = geo[5], tx = kt[tid][0], ty = kt[tid][1], nx = -ty, ny = tx;
    double cx = kc[tid][0], cy = kc[tid][1];
    if (tid == 0) {
      cx = cx - d * tx; cy = cy - d * ty;
    } else if (tid == kn - 1) {
      cx = cx + d * tx; cy = cy + d * ty;
    }
    const double h = kh[tid] + d;
    top[tid][0] = cx - nx * h; top[tid][1] = cy - ny * h;
    bot[tid][0] = cx + nx * h; bot[tid][1] = cy + ny * h;
  }
  __syncthreads();
  if (tid < kn - 1) {                                   // 8. fold: every cell strictly convex
    const double qx[4] = {top[tid][0], top[tid + 1][0], bot[tid + 1][0], bot[tid][0]};
    const double qy[4] = {top[tid][1], top[tid + 1][1], bot[tid + 1][1], bot[tid][1]};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int j1 = (j + 1) & 3, j2 = (j + 2) & 3;
      ok &= (qx[j1] - qx[j]) * (qy[j2] - qy[j1]) - (qy[j1] - qy[j]) * (qx[j2] - qx[j1]) > 0.0;
    }
    if (!ok) atomicOr(&misc[RB_FLAG], 1);
  }
  __syncthreads();
  if (misc[RB_FLAG]) {
    none(RB_FOLDED);
    return;
  }
  if (tid < RB_K) {                                     // 9. scale
    double* o = ribbons + row * RB_ROW + tid * 4;
    if (tid < kn) {
      const double dw = (double)dest[2 * n], dh = (double)dest[2 * n + 1];
      o[0] = top[tid][0] / (double)W * dw; o[1] = top[tid][1] / (double)H * dh;
      o[2] = bot[tid][0] / (double)W * dw; o[3] = bot[tid][1] / (double)H * dh;
    } else {
      o[0] = o[1] = o[2] = o[3] = 0.0;
    }
  }
  if (tid == 0) { knots[row] = kn; why[row] = RB_NONE; }
}

// workspace of mr_db_boxes, every part 16-byte aligned
struct DbxWorkspace {
  long long sbox, labels, rank, ext, rowcnt, sscore, status, cand, bytes;
};
static inline DbxWorkspace dbx_workspace(int N, int H, int W, int K) {
  auto up = [](long long b) { return (b + 15) / 16 * 16; };
  DbxWorkspace w;
  long long off = 0;
  w.sbox = off;   off += up((long long)N * K * 8 * 8);
  w.labels = off; off += up((long long)N * H * W * 4);
  w.rank = off;   off += up((long long)N * H * W * 4);
  w.ext = off;    off += up((long long)N * K * H * 2 * 4);
  w.rowcnt = off; off += up((long long)N * H * 4);
  w.sscore = off; off += up((long long)N * K * 4);
  w.status = off; off += up((long long)N * K * 4);
  w.cand = off;   off += up((long long)N * K * 8 * 8);    // the candidate rectangles, for mr_db_ribbons
  w.bytes = off;
  return w;
}
static inline const char* dbx_bad_shape(int N, int H, int W, int K) {
  if (!(N > 0 && H > 0 && W > 0)) return "N, H, W must be positive";
  if (!((long long)H * W < (1ll << 31))) return "H * W must be below 2^31";
  if (!(K >= 1 && K <= DBX_MAX_K)) return "K must be in [1, 1024]";
  if (!(H <= DBX_MAX_H)) return "H must be at most 2048 (the hull points of a candidate are staged in LDS)";
  if (!((long long)N * H < (1ll << 31) && (long long)N * K < (1ll << 31))) return "N * H and N * K must be below 2^31";
  return nullptr;
}

}  // namespace mr

using namespace mr;

extern "C" {

// prob f32 [N][H][W] -> labels i32 [N][H][W] (root pixel index of the 8-connected component, -1 = background),
// points int4 [cap] = (n, root, x, y) of every run end point, *count = how many (may exceed cap: enlarge and re-run).
// *count must be zero on entry.
int mr_db_components(const float* prob, float thresh, int* labels, void* points, int* count, int cap, int N, int H, int W,
                     hipStream_t stream) {
  MR_CHECK_ARG(N > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) && cap >= 0, "mr_db_components: bad shape");
  const long long total = (long long)N * H * W;
  hipLaunchKernelGGL(db_cc_init_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, prob, thresh, labels, total,
                     H * W);
  hipLaunchKernelGGL(db_cc_merge_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, labels, N, H, W);
  hipLaunchKernelGGL(db_cc_points_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, labels, N, H, W,
                     (int4*)points, count, cap);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

// boxes f32 [B][9] (image index, 4 vertices in order), out f32 [B][2] = (sum of prob, pixel count) inside each box
int mr_db_box_scores(const float* prob, const float* boxes, float* out, int B, int N, int H, int W, hipStream_t stream) {
  MR_CHECK_ARG(B >= 0 && N > 0 && H > 0 && W > 0, "mr_db_box_scores: bad shape");
  if (B == 0) return MR_OK;
  hipLaunchKernelGGL(db_box_score_kernel, dim3(B), dim3(256), 0, stream, prob, H, W, boxes, out);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

// bytes of workspace mr_db_boxes wants: labels, rank map, row counts, extremes table, the uncompacted boxes / scores / statuses /
// candidate rectangles
int mr_db_boxes_ws_bytes(int N, int H, int W, int K, long long* bytes) {
  MR_CHECK_ARG(bytes != nullptr, "mr_db_boxes_ws_bytes: bytes is null");
  const char* bad = dbx_bad_shape(N, H, W, K);
  MR_CHECK_ARG(bad == nullptr, "mr_db_boxes_ws_bytes: %s", bad);
  *bytes = dbx_workspace(N, H, W, K).bytes;
  return MR_OK;
}

// the whole of `boxes_from_bitmap` for a batch: 9 launches on `stream`, no host synchronisation (include/megreader_hip.h)
int mr_db_boxes(const float* prob, const float* seg, float thresh, const int* dest, int N, int H, int W, int K,
                double box_thresh, double min_size, void* ws, double* boxes, float* scores, int* count, int* components,
                double* cand, float* cand_sums, int* status, hipStream_t stream) {
  const char* bad = dbx_bad_shape(N, H, W, K);
  MR_CHECK_ARG(bad == nullptr, "mr_db_boxes: %s", bad);
  MR_CHECK_ARG(prob && seg && dest && ws && boxes && scores && count && components, "mr_db_boxes: null pointer");
  MR_CHECK_ARG(((unsigned long long)ws & 15ull) == 0, "mr_db_boxes: ws must be 16-byte aligned");
  const DbxWorkspace w = dbx_workspace(N, H, W, K);
  char* base = (char*)ws;
  double* sbox = (double*)(base + w.sbox);
  int* labels = (int*)(base + w.labels);
  int* rank = (int*)(base + w.rank);
  int* ext = (int*)(base + w.ext);
  int* rowcnt = (int*)(base + w.rowcnt);
  float* sscore = (float*)(base + w.sscore);
  int* st = (int*)(base + w.status);
  const long long total = (long long)N * H * W;
  const int rows = N * H;
  hipLaunchKernelGGL(db_cc_init_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, seg, thresh, labels, total, H * W);
  hipLaunchKernelGGL(db_cc_merge_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, labels, N, H, W);
  hipLaunchKernelGGL(db_row_roots_kernel, dim3(grid_for(rows, 4)), dim3(256), 0, stream, labels, rows, H, W, rowcnt);
  hipLaunchKernelGGL(db_row_scan_kernel, dim3(N), dim3(256), 0, stream, rowcnt, H, components);
  hipLaunchKernelGGL(db_root_rank_kernel, dim3(grid_for(rows, 4)), dim3(256), 0, stream, labels, rows, H, W, rowcnt, rank);
  hipLaunchKernelGGL(db_extremes_fill_kernel, dim3(grid_for((long long)N * K * H, 256)), dim3(256), 0, stream, (int2*)ext,
                     (long long)N * K * H);
  hipLaunchKernelGGL(db_extremes_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, labels, rank, N, H, W, K, ext);
  hipLaunchKernelGGL(db_boxes_kernel, dim3(N * K), dim3(256), dbx_lds_bytes(H), stream, prob, H, W, K, components,
                     (const int2*)ext, dest, box_thresh, min_size, sbox, sscore, st, cand, cand_sums, status,
                     (double*)(base + w.cand));
  hipLaunchKernelGGL(db_boxes_compact_kernel, dim3(N), dim3(256), 0, stream, st, sbox, sscore, K, boxes, scores, count);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

// bytes of workspace mr_db_ribbons wants: the six integer sums of every slab, i64 [N][K][MR_RIBBON_MAX_SLABS][6]
int mr_db_ribbons_ws_bytes(int N, int K, long long* bytes) {
  MR_CHECK_ARG(bytes != nullptr, "mr_db_ribbons_ws_bytes: bytes is null");
  MR_CHECK_ARG(N > 0 && K >= 1 && K <= DBX_MAX_K && (long long)N * K < (1ll << 31), "mr_db_ribbons_ws_bytes: bad shape");
  *bytes = (long long)N * K * RB_S * 6 * 8;
  return MR_OK;
}

// a ribbon beside every box of the preceding mr_db_boxes (same shapes, same ws, same stream): one launch (include/megreader_hip.h)
int mr_db_ribbons(const int* dest, int N, int H, int W, int K, int slabs, double ratio, const void* ws, void* rws,
                  double* ribbons, int* knots, int* why, hipStream_t stream) {
  const char* bad = dbx_bad_shape(N, H, W, K);
  MR_CHECK_ARG(bad == nullptr, "mr_db_ribbons: %s", bad);
  MR_CHECK_ARG(slabs >= 3 && slabs <= RB_S, "mr_db_ribbons: slabs must be in [3, %d], got %d", RB_S, slabs);
  MR_CHECK_ARG(ratio >= 0.0 && ratio <= 1e6, "mr_db_ribbons: ratio must be in [0, 1e6]");
  MR_CHECK_ARG(dest && ws && rws && ribbons && knots && why, "mr_db_ribbons: null pointer");
  MR_CHECK_ARG(((unsigned long long)ws & 15ull) == 0 && ((unsigned long long)rws & 7ull) == 0,
               "mr_db_ribbons: ws must be 16-byte aligned, rws 8-byte aligned");
  const DbxWorkspace w = dbx_workspace(N, H, W, K);
  const char* base = (const char*)ws;
  hipLaunchKernelGGL(db_ribbons_kernel, dim3(N * K), dim3(256), 0, stream, (const int*)(base + w.labels),
                     (const int2*)(base + w.ext), (const int*)(base + w.status), (const double*)(base + w.cand), dest, H, W, K,
                     slabs, ratio, (long long*)rws, ribbons, knots, why);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // extern "C"
