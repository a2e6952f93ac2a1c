"""`mr_db_boxes` (csrc/db_post.hip) restated in pure Python / numpy, in the kernels' operation order.  TEST INFRASTRUCTURE ONLY.

What the device does differently from the host path of `SegDetectorRepresenter.boxes_from_maps`, and what this file mirrors:
  * candidates are ranked by the raster position of their first pixel (a prefix count), cut at K;
  * a candidate's points are its row extremes (min x, max x per row), laid out (y ascending, x descending); a monotone chain over
    them with the cross products of db_geometry.convex_hull, rotated to start at the smallest (x, y);
  * calipers per hull edge with sqrt(ex*ex + ey*ey), the host's sequential `area < best - 1e-12` choice;
  * the score is (double)s / (double)c of float32 sums s, c: `box_sums` restates the kernel's summation order (256 strided
    threads, butterfly over 64 lanes, four partials left to right); sums may also be given;
  * unclip with sqrt instead of math.hypot; rint, clamp by comparison.
Python floats are float64 and never fused, which is what `#pragma clang fp contract(off)` makes of the kernel."""
import math

import numpy as np

NONE, SHORT, WEAK, SMALL, KEPT = 0, 1, 2, 3, 4


def label_components(mask):
    """[H, W] bool -> (root [H, W] int32: raster index of the component's first pixel or -1, roots in raster order)."""
    H, W = mask.shape
    root = np.full((H, W), -1, np.int32)
    roots = []
    for y in range(H):
        for x in range(W):
            if not mask[y, x] or root[y, x] >= 0:
                continue
            r = y * W + x
            roots.append(r)
            root[y, x] = r
            stack = [(x, y)]
            while stack:
                cx, cy = stack.pop()
                for ny in range(max(0, cy - 1), min(H, cy + 2)):
                    for nx in range(max(0, cx - 1), min(W, cx + 2)):
                        if mask[ny, nx] and root[ny, nx] < 0:
                            root[ny, nx] = r
                            stack.append((nx, ny))
    return root, roots


def row_extremes(root, r):
    """[(y, min x, max x)] of component r, rows ascending."""
    ys, xs = np.nonzero(root == r)
    return [(int(y), int(xs[ys == y].min()), int(xs[ys == y].max())) for y in range(int(ys.min()), int(ys.max()) + 1)]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _chain(seq):
    st = []
    for p in seq:
        if st and st[-1] == p:
            continue
        while len(st) >= 2 and _cross(st[-2], st[-1], p) <= 0:
            st.pop()
        st.append(p)
    return st


def hull_from_extremes(rows):
    """The vertex sequence of db_geometry.convex_hull(all pixels), from the row extremes alone; integer points."""
    pts = []
    for y, lo, hi in rows:
        pts += [(hi, y), (lo, y)]
    a, b = _chain(pts), _chain(pts[::-1])
    if len(a) == 1:
        return [a[0]]
    hull = a[:-1] + b[:-1]
    start = hull.index(min(hull))
    return hull[start:] + hull[:start]


def hull_of_points(points):
    """db_geometry.convex_hull on float points (the four unclipped corners)."""
    pts = sorted(set((float(x), float(y)) for x, y in points))
    if len(pts) <= 2:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def sequential_choice(areas):
    """Index the host's scan keeps: `best` is replaced when area < best - 1e-12 (NOT an arg-min with a tolerance)."""
    best, pick = None, -1
    for i, a in enumerate(areas):
        if best is None or a < best - 1e-12:
            best, pick = a, i
    return pick


def min_area_rect(hull):
    hull = [(float(x), float(y)) for x, y in hull]
    if len(hull) == 1:
        x, y = hull[0]
        return [[x, y]] * 4, (0.0, 0.0)
    if len(hull) == 2:
        (x0, y0), (x1, y1) = hull
        ex, ey = x1 - x0, y1 - y0
        return [[x0, y0], [x1, y1], [x1, y1], [x0, y0]], (math.sqrt(ex * ex + ey * ey), 0.0)
    frames, n = [], len(hull)
    for i in range(n):
        x0, y0 = hull[i]
        x1, y1 = hull[(i + 1) % n]
        ex, ey = x1 - x0, y1 - y0
        ln = math.sqrt(ex * ex + ey * ey)
        ux, uy = ex / ln, ey / ln
        lo_u = hi_u = lo_v = hi_v = None
        for j, (px, py) in enumerate(hull):
            pu = (px - x0) * ux + (py - y0) * uy
            pv = -(px - x0) * uy + (py - y0) * ux
            if j == 0:
                lo_u = hi_u = pu
                lo_v = hi_v = pv
            else:
                lo_u = pu if pu < lo_u else lo_u
                hi_u = pu if pu > hi_u else hi_u
                lo_v = pv if pv < lo_v else lo_v
                hi_v = pv if pv > hi_v else hi_v
        frames.append(((hi_u - lo_u) * (hi_v - lo_v), x0, y0, ux, uy, lo_u, hi_u, lo_v, hi_v))
    _, x0, y0, ux, uy, lo_u, hi_u, lo_v, hi_v = frames[sequential_choice([f[0] for f in frames])]
    corners = [[x0 + a * ux - b * uy, y0 + a * uy + b * ux] for a, b in
               ((lo_u, lo_v), (hi_u, lo_v), (hi_u, hi_v), (lo_u, hi_v))]
    return corners, (hi_u - lo_u, hi_v - lo_v)


def mini_box(hull):
    corners, (sa, sb) = min_area_rect(hull)
    p = sorted(corners, key=lambda c: c[0])
    i1, i4 = (0, 1) if p[1][1] > p[0][1] else (1, 0)
    i2, i3 = (2, 3) if p[3][1] > p[2][1] else (3, 2)
    return [p[i1], p[i2], p[i3], p[i4]], (sb if sb < sa else sa)


def unclip(box):
    (x0, y0), (x1, y1), _, (x3, y3) = box
    a = math.sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0))
    b = math.sqrt((x3 - x0) * (x3 - x0) + (y3 - y0) * (y3 - y0))
    if a == 0.0 or b == 0.0:
        return [list(p) for p in box]
    d = a * b * 1.5 / (2.0 * (a + b))
    q = [(float(int(x)), float(int(y))) for x, y in box]
    (x0, y0), (x1, y1), _, (x3, y3) = q
    a = math.sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0))
    b = math.sqrt((x3 - x0) * (x3 - x0) + (y3 - y0) * (y3 - y0))
    if a == 0.0 or b == 0.0:
        return [list(p) for p in q]
    ux, uy, vx, vy = (x1 - x0) / a, (y1 - y0) / a, (x3 - x0) / b, (y3 - y0) / b
    return [[px + d * (su * ux + sv * vx), py + d * (su * uy + sv * vy)]
            for (px, py), (su, sv) in zip(q, ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)))]


def box_sums(pred, box):
    """(sum, count) as float32, in the order of `box_score_sums` of csrc/db_post.hip.  The inside test runs on small integers
    (truncated corners, pixel coordinates), so it is exact in any precision."""
    H, W = pred.shape
    v = [(int(x), int(y)) for x, y in box]
    xs, ys = [p[0] for p in v], [p[1] for p in v]
    x0, x1, y0, y1 = max(0, min(xs)), min(W - 1, max(xs)), max(0, min(ys)), min(H - 1, max(ys))
    area2 = sum(v[k][0] * v[(k + 1) % 4][1] - v[(k + 1) % 4][0] * v[k][1] for k in range(4))
    sgn = 1 if area2 >= 0 else -1
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    if bw <= 0 or bh <= 0:
        return np.float32(0), np.float32(0)
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    inside = np.ones((bh, bw), bool)
    for k in range(4):
        ex, ey = v[(k + 1) % 4][0] - v[k][0], v[(k + 1) % 4][1] - v[k][1]
        inside &= sgn * (ex * (yy - v[k][1]) - ey * (xx - v[k][0])) >= 0
    vals = np.where(inside, pred[y0:y1 + 1, x0:x1 + 1], np.float32(0)).astype(np.float32).reshape(-1)
    ones = inside.astype(np.float32).reshape(-1)
    pad = (-len(vals)) % 256
    vals = np.concatenate([vals, np.zeros(pad, np.float32)]).reshape(-1, 256)
    ones = np.concatenate([ones, np.zeros(pad, np.float32)]).reshape(-1, 256)

    def total(rounds):
        acc = np.zeros(256, np.float32)
        for r in rounds:                      # thread t adds its elements t, t + 256, ... in order
            acc = acc + r
        lanes = acc.reshape(4, 64)
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):        # wave_sum: v += shfl_xor(v, o)
            lanes = lanes + lanes[:, idx ^ o]
        part = lanes[:, 0]
        return np.float32(np.float32(np.float32(part[0] + part[1]) + part[2]) + part[3])
    return total(vals), total(ones)


def db_boxes(prob, seg_mask, dest, K=100, box_thresh=0.7, min_size=3, sums=None):
    """prob f32 [N, H, W], seg_mask bool [N, H, W], dest [(width, height)] per image.  `sums(n, k, box) -> (s, c)` replaces
    `box_sums`.  Returns the outputs of mr_db_boxes as numpy arrays: boxes f64 [N, K, 4, 2], scores f32 [N, K], count [N],
    components [N], cand f64 [N, K, 4, 2], cand_sums f32 [N, K, 2], status i32 [N, K]."""
    N, H, W = seg_mask.shape
    out = {'boxes': np.zeros((N, K, 4, 2)), 'scores': np.zeros((N, K), np.float32), 'count': np.zeros(N, np.int32),
           'components': np.zeros(N, np.int32), 'cand': np.zeros((N, K, 4, 2)),
           'cand_sums': np.zeros((N, K, 2), np.float32), 'status': np.zeros((N, K), np.int32)}
    for n in range(N):
        root, roots = label_components(seg_mask[n])
        out['components'][n] = len(roots)
        dw, dh = float(dest[n][0]), float(dest[n][1])
        for k, r in enumerate(roots[:K]):
            box, sside = mini_box(hull_from_extremes(row_extremes(root, r)))
            out['cand'][n, k] = box
            if sside < min_size:
                out['status'][n, k] = SHORT
                continue
            s, c = box_sums(prob[n], box) if sums is None else sums(n, k, box)
            out['cand_sums'][n, k] = (s, c)
            score = float(s) / float(c) if c > 0 else 0.0
            if box_thresh > score:
                out['status'][n, k] = WEAK
                continue
            box2, sside = mini_box(hull_of_points(unclip(box)))
            if sside < min_size + 2.0:
                out['status'][n, k] = SMALL
                continue
            out['status'][n, k] = KEPT
            j = out['count'][n]
            for i, (x, y) in enumerate(box2):
                vx, vy = float(np.rint(x / float(W) * dw)), float(np.rint(y / float(H) * dh))
                out['boxes'][n, j, i] = (0.0 if vx < 0.0 else (dw if vx > dw else vx),
                                         0.0 if vy < 0.0 else (dh if vy > dh else vy))
            out['scores'][n, j] = np.float32(score)
            out['count'][n] = j + 1
    return out


def box_lists(out):
    """The representer's return format from the arrays above."""
    return [out['boxes'][n, :int(out['count'][n])].tolist() for n in range(len(out['count']))]


def lens_outline(half=66):
    """bool [2 * half, W]: the connected OUTLINE of a lens whose every row end is a hull vertex -- row y starts at T(k) and ends at
    W - 1 - T(k), T(k) = k (k + 1) / 2, k the distance to the two middle rows -- so the hull has 4 * half vertices (264: more
    than the 256 edges the calipers of the kernel take per round) while only ~ 17 000 pixels are set."""
    t = [k * (k + 1) // 2 for k in range(half)]
    W = 2 * t[-1] + 40
    left = [t[half - 1 - y] for y in range(half)] + [t[y] for y in range(half)]
    m = np.zeros((2 * half, W), bool)
    m[0, left[0]:W - left[0]] = True
    m[-1, left[-1]:W - left[-1]] = True
    for y in range(2 * half):
        m[y, left[y]] = m[y, W - 1 - left[y]] = True
        for other in (y - 1, y + 1):                    # reach over to the neighbour row that starts further in
            if 0 <= other < 2 * half and left[other] > left[y]:
                m[y, left[y]:left[other] + 1] = True
                m[y, W - 1 - left[other]:W - left[y]] = True
    return m
