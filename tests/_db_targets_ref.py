"""numpy float64 restatement of mr_db_targets (include/megreader_hip.h; csrc/db_targets.hip) -- the checker of
tests/test_db_targets_cpu.py and tests/test_db_targets_gpu.py.  No tests are collected from this module.

Every expression is written in the operation order of the kernels (which are compiled without FMA contraction), so the
two agree to the last bit except in `sqrt` / divide of the device, which the comparison tolerance of thresh_map covers.
Each polygon is evaluated only over its own box (grown by one pixel, as the map kernel culls), so it stays fast.

Besides the maps, `db_targets_ref` returns `skip`: per map, the pixels whose decision a perturbation of 1e-9 (relative to
max(1, D^2)) of the deciding quantity could flip -- |d^2 - D^2| for gt / thresh_mask, |d^2 - 0.25| for mask, and a crossing
abscissa within that margin of x where the inside test can still change the result.
"""
import numpy as np

MARGIN = 1e-9


def polygon_area(q):
    """make_seg_detection_data.py:92-99, same summation order."""
    a = 0.0
    for k in range(4):
        k1 = (k + 1) & 3
        a = a + (q[k1, 0] - q[k, 0]) * (q[k1, 1] + q[k, 1])
    return a / 2.0


def rnd_away(v):
    """pyclipper's Round(): half away from zero."""
    return float(np.copysign(np.floor(np.abs(v) + 0.5), v))


def inside_dist2(p, x, y, tol):
    """(inside by the even-odd rule, min squared distance to the closed non-degenerate edges, crossing within tol of x)
    of the points (x, y) (arrays) for the quad p [4, 2]."""
    inside = np.zeros(x.shape, dtype=bool)
    close = np.zeros(x.shape, dtype=bool)
    d2 = np.full(x.shape, np.inf)
    for k in range(4):
        ax, ay = p[k]
        bx, by = p[(k + 1) & 3]
        cond = (ay > y) != (by > y)
        if cond.any():
            with np.errstate(divide='ignore', invalid='ignore'):
                xc = ax + (y - ay) * (bx - ax) / (by - ay)
            inside ^= cond & (x < xc)
            close |= cond & (np.abs(xc - x) <= tol)
        s = (bx - ax) * (bx - ax) + (by - ay) * (by - ay)
        if s > 0.0:
            t = ((x - ax) * (bx - ax) + (y - ay) * (by - ay)) / s
            t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
            qx = ax + t * (bx - ax)
            qy = ay + t * (by - ay)
            d2 = np.fmin(d2, (x - qx) * (x - qx) + (y - qy) * (y - qy))
    return inside, d2, close


def border_dist(p, x, y):
    """MakeBorderMap.distance (make_border_map.py:95-120), minimised over the non-degenerate edges; 1 - cosin^2 is
    clamped at 0 and the result is 0 where an end point is hit."""
    e = np.full(x.shape, np.inf)
    for k in range(4):
        ax, ay = p[k]
        bx, by = p[(k + 1) & 3]
        s = (bx - ax) * (bx - ax) + (by - ay) * (by - ay)
        if not s > 0.0:
            continue
        s1 = (x - ax) * (x - ax) + (y - ay) * (y - ay)
        s2 = (x - bx) * (x - bx) + (y - by) * (y - by)
        with np.errstate(divide='ignore', invalid='ignore'):
            cosin = (s - s1 - s2) / (2.0 * np.sqrt(s1 * s2))
            sin2 = np.fmax(1.0 - cosin * cosin, 0.0)
            r = np.sqrt(s1 * s2 * sin2 / s)
        r = np.where(cosin < 0.0, np.sqrt(np.fmin(s1, s2)), r)
        r = np.where((s1 == 0.0) | (s2 == 0.0), 0.0, r)
        e = np.fmin(e, r)
    return e


def prepare(poly, ignore_in, H, W, min_text_size, shrink_ratio):
    """Steps 1 to 5 for one polygon: (clipped reordered points, D, ignored)."""
    q = np.array(poly, dtype=np.float64).reshape(4, 2)
    q[:, 0] = np.fmin(np.fmax(q[:, 0], 0.0), float(W - 1))
    q[:, 1] = np.fmin(np.fmax(q[:, 1], 0.0), float(H - 1))
    a = polygon_area(q)
    ignored = bool(ignore_in) or abs(a) < 1.0
    if a > 0.0:
        q = q[[0, 3, 2, 1]]
    edge = [float(np.sqrt((q[k, 0] - q[(k + 1) & 3, 0]) * (q[k, 0] - q[(k + 1) & 3, 0])
                          + (q[k, 1] - q[(k + 1) & 3, 1]) * (q[k, 1] - q[(k + 1) & 3, 1]))) for k in range(4)]
    height, width = min(edge[3], edge[1]), min(edge[0], edge[2])
    if min(height, width) < min_text_size:
        ignored = True
    if ignored:
        return q, 0.0, True
    D = abs(a) * (1.0 - shrink_ratio * shrink_ratio) / (edge[0] + edge[1] + edge[2] + edge[3])
    x0, x1 = int(np.ceil(q[:, 0].min())), int(np.floor(q[:, 0].max()))
    y0, y1 = int(np.ceil(q[:, 1].min())), int(np.floor(q[:, 1].max()))
    if x1 >= x0 and y1 >= y0:
        ys, xs = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.float64), np.arange(x0, x1 + 1, dtype=np.float64), indexing='ij')
        inside, d2, _ = inside_dist2(q, xs, ys, 0.0)
        if (inside & (d2 >= D * D)).any():
            return q, D, False
    return q, 0.0, True


def _grid(x0, x1, y0, y1, H, W):
    x0, x1, y0, y1 = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
    if x1 < x0 or y1 < y0:
        return None
    ys, xs = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.float64), np.arange(x0, x1 + 1, dtype=np.float64), indexing='ij')
    return slice(y0, y1 + 1), slice(x0, x1 + 1), xs, ys


def db_targets_ref(polys, count, ignore_in, H, W, min_text_size=8.0, shrink_ratio=0.4, thresh_min=0.3, thresh_max=0.7):
    polys = np.asarray(polys, dtype=np.float64)
    N, G = polys.shape[0], polys.shape[1]
    ignore_in = np.asarray(ignore_in).reshape(N, G)
    gt = np.zeros((N, 1, H, W), dtype=np.float32)
    mask = np.ones((N, H, W), dtype=np.float32)
    tmask = np.zeros((N, H, W), dtype=np.float32)
    canvas = np.zeros((N, H, W), dtype=np.float32)
    ignore_out = np.zeros((N, G), dtype=np.int32)
    dist = np.zeros((N, G), dtype=np.float64)
    skip = {k: np.zeros((N, H, W), dtype=bool) for k in ('gt', 'mask', 'thresh_mask')}
    for n in range(N):
        for g in range(min(max(int(count[n]), 0), G)):
            q, D, ignored = prepare(polys[n, g], ignore_in[n, g], H, W, min_text_size, shrink_ratio)
            ignore_out[n, g] = 1 if ignored else 0
            dist[n, g] = D
            if ignored:
                q = np.trunc(q)
                r = _grid(int(q[:, 0].min()) - 1, int(q[:, 0].max()) + 1, int(q[:, 1].min()) - 1, int(q[:, 1].max()) + 1, H, W)
                if r is None:
                    continue
                sy, sx, xs, ys = r
                inside, d2, close = inside_dist2(q, xs, ys, MARGIN)
                near = d2 <= 0.25
                near_m = np.abs(d2 - 0.25) <= MARGIN
                mask[n, sy, sx][inside | near] = 0.0
                skip['mask'][n, sy, sx] |= (near_m & (~inside | close)) | (close & (~near | near_m))
                continue
            D2 = D * D
            bx0, bx1 = int(rnd_away(q[:, 0].min() - D)), int(rnd_away(q[:, 0].max() + D))
            by0, by1 = int(rnd_away(q[:, 1].min() - D)), int(rnd_away(q[:, 1].max() + D))
            r = _grid(bx0 - 1, bx1 + 1, by0 - 1, by1 + 1, H, W)
            if r is None:
                continue
            sy, sx, xs, ys = r
            tol = MARGIN * max(1.0, D2)
            inside, d2, close = inside_dist2(q, xs, ys, tol)
            far, near = d2 >= D2, d2 <= D2
            edge_m = np.abs(d2 - D2) <= tol
            gt[n, 0, sy, sx][inside & far] = 1.0
            tmask[n, sy, sx][inside | near] = 1.0
            skip['gt'][n, sy, sx] |= (edge_m & (inside | close)) | (close & (far | edge_m))
            skip['thresh_mask'][n, sy, sx] |= (edge_m & (~inside | close)) | (close & (~near | edge_m))
            e = border_dist(q, xs, ys)
            ratio = np.fmin(e / D, 1.0).astype(np.float32)           # distance_map is float32
            c = np.float32(1.0) - ratio
            inbox = (xs >= bx0) & (xs <= bx1) & (ys >= by0) & (ys <= by1)
            canvas[n, sy, sx] = np.where(inbox, np.fmax(canvas[n, sy, sx], c), canvas[n, sy, sx])
    thresh_map = canvas * np.float32(thresh_max - thresh_min) + np.float32(thresh_min)
    return {'gt': gt, 'mask': mask, 'thresh_map': thresh_map.astype(np.float32), 'thresh_mask': tmask,
            'ignore_out': ignore_out, 'dist': dist, 'skip': skip}
