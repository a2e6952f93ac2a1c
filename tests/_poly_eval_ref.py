"""Float64 restatement, in plain Python, of `mr_poly_iou` (csrc/quad_measure.hip) after the rule written out in
include/megreader_hip.h: validity and area of a simple polygon of any vertex count, the area of the intersection of two such
polygons as a sum of signed triangle overlaps in the kernel's order, and -- through the bookkeeping of tests/_quad_eval_ref.py --
what `polygon_measure` and `PolygonMeasurer` return.  The checker of tests/test_polygon_measure_gpu.py, itself checked against
exact rational arithmetic, point counting and hand-computed answers in tests/test_polygon_measure_cpu.py.  Helper module: no
tests are collected from it."""
import math
import random
import types

import _quad_eval_ref as R
from _quad_eval_ref import MARGIN, orient2, segments_touch  # noqa: F401

MAX_VERTS = 64
LANES = 64
EPS = 2.0 ** -52


def poly_valid(q):
    """The stated rule for a ring of m >= 3 vertices."""
    m = len(q)
    if m < 3 or m > MAX_VERTS:
        return False
    a2 = abs(R.area2(q))
    if not (a2 > 0.0 and a2 < math.inf):
        return False
    for e in range(m):
        a, b = q[e], q[(e + 1) % m]
        for f in range(m):
            if f == e:
                continue
            c, d = q[f], q[(f + 1) % m]
            if c[0] == a[0] and c[1] == a[1]:
                return False                                     # a repeated vertex
            if f == (e + 1) % m:                                 # the next edge: no fold back onto a - b
                if orient2(a, b, d) == 0.0 and (a[0] - b[0]) * (d[0] - b[0]) + (a[1] - b[1]) * (d[1] - b[1]) > 0.0:
                    return False
            elif (f + 1) % m != e:
                if segments_touch(a, b, c, d):
                    return False
    return True


def poly_area(q):
    return 0.5 * abs(R.area2(q))


def _disjoint(p, q):
    return max(v[0] for v in p) < min(v[0] for v in q) or max(v[0] for v in q) < min(v[0] for v in p) or \
        max(v[1] for v in p) < min(v[1] for v in q) or max(v[1] for v in q) < min(v[1] for v in p)


def fan(P):
    """[(orientation o, the triangle stored counter-clockwise)] of the fan from P[0]; o == 0 marks a triangle to skip."""
    out = []
    for i in range(len(P) - 2):
        o = orient2(P[0], P[i + 1], P[i + 2])
        out.append((o, [P[0], P[i + 1], P[i + 2]] if o > 0.0 else [P[0], P[i + 2], P[i + 1]]))
    return out


def poly_intersection(p, q):
    """Area of the intersection of two valid polygons (any orientation, convex or not), in the kernel's order."""
    if _disjoint(p, q):
        return 0.0
    ox, oy = p[0]
    S = fan([(x - ox, y - oy) for x, y in p])
    C = fan([(x - ox, y - oy) for x, y in q])
    lanes = [0.0] * LANES
    for t in range(len(S) * len(C)):
        (os, s), (oc, c) = S[t // len(C)], C[t % len(C)]
        if os == 0.0 or oc == 0.0 or _disjoint(s, c):
            continue
        a = R.triangle_overlap(s, c)
        lanes[t % LANES] = lanes[t % LANES] + (a if (os > 0.0) == (oc > 0.0) else -a)
    step = LANES // 2
    while step > 0:
        for l in range(step):
            lanes[l] = lanes[l] + lanes[l + step]
        step //= 2
    return abs(lanes[0])


# the bookkeeping of _quad_eval_ref.evaluate_image, word for word, over the three polygon functions above
evaluate_image = types.FunctionType(
    R.evaluate_image.__code__,
    dict(vars(R), quad_valid=poly_valid, quad_area=poly_area, quad_intersection=poly_intersection),
    "evaluate_image", R.evaluate_image.__defaults__)


def extent(p, q):
    """E of the tolerance: the larger side of the box around both polygons."""
    xs, ys = [v[0] for v in p] + [v[0] for v in q], [v[1] for v in p] + [v[1] for v in q]
    return max(max(xs) - min(xs), max(ys) - min(ys))


def area_tol(p, q):
    """100 * m * n * 2^-52 * E^2 (tests/test_polygon_measure_cpu.py derives it)."""
    return 100.0 * len(p) * len(q) * EPS * extent(p, q) ** 2


# ---- committed cases ----------------------------------------------------------------------------------------------------------------

L_SHAPE = [(0, 0), (6, 0), (6, 2), (2, 2), (2, 6), (0, 6)]                                       # area 12 + 8
COMB = [(0, 0), (7, 0), (7, 5), (6, 5), (6, 1), (4, 1), (4, 5), (3, 5), (3, 1), (1, 1), (1, 5), (0, 5)]      # 7 + 3 * 4
STAR = [(4, 0), (1, 1), (0, 4), (-1, 1), (-4, 0), (-1, -1), (0, -4), (1, -1)]                   # 8 triangles of area 2
ARROW = [(0, 0), (4, 1), (0, 2), (1, 1)]                                                         # a concave quad, area 3
# name -> (p, q, area of p, area of q, area of the intersection), all by hand
HAND = {
    # the rectangle cuts x in [1, 5], y in [1, 2] (4) and x in [1, 2], y in [2, 5] (3) out of the L
    'l_shape_and_rectangle': (L_SHAPE, R.box(1, 1, 5, 5), 20, 16, 7),
    # the bar crosses the three teeth and misses the back: three disconnected 1 x 2 pieces (the convex hull would give 14)
    'comb_and_bar': (COMB, R.box(-1, 2, 8, 4), 19, 18, 6),
    'l_shape_inside_a_box': (L_SHAPE, R.box(-5, -5, 10, 10), 20, 225, 20),
    'box_around_the_comb': (R.box(-5, -5, 10, 10), COMB, 225, 19, 19),
    'star_and_its_inner_square': (STAR, R.box(-1, -1, 1, 1), 16, 4, 4),
    'star_and_a_half_plane_box': (STAR, R.box(0, -4, 4, 4), 16, 32, 8),
    'comb_with_itself': (COMB, COMB, 19, 19, 19),
    'star_with_itself': (STAR, STAR, 16, 16, 16),
    # the second comb upside down and 1.5 to the right: teeth x in [1.5, 2.5], [4.5, 5.5], [7.5, 8.5] between the first one's teeth
    # x in [0, 1], [3, 4], [6, 7], its back y in [5, 6] above their tips: boundaries touch, nothing overlaps
    'two_combs_interleaved': (COMB, [(x + 1.5, 6 - y) for x, y in COMB], 19, 19, 0),
    'triangle_in_the_l': ([(0, 0), (6, 0), (0, 6)], L_SHAPE, 18, 20, 16),
    # x in [0, 1] of the dart: between y = x / 4 and y = x, and its mirror image about y = 1: 2 * 3 / 8
    'arrow_and_box': (ARROW, R.box(0, 0, 1, 2), 3, 2, 0.75),
    'disjoint': (STAR, R.box(10, 10, 12, 12), 16, 4, 0),
    'touching_along_an_edge': (R.box(0, 0, 2, 2), R.box(2, 0, 4, 2), 4, 4, 0),
}


INVALID = {
    'bow_tie_5_gon': [(0, 0), (4, 4), (4, 0), (0, 4), (-1, 2)],                     # edges 0-1 and 2-3 cross at (2, 2)
    'bow_tie_8_gon': [(0, 0), (2, -1), (4, 0), (5, 2), (4, 4), (0, 4), (6, 1), (-1, 2)],
    'repeated_vertex_in_a_row': [(0, 0), (4, 0), (4, 0), (4, 4), (0, 4)],
    'repeated_vertex_apart': [(0, 0), (2, 2), (4, 0), (4, 4), (2, 2), (0, 4)],    # two triangles pinched at (2, 2)
    'collinear_spike': [(0, 0), (4, 0), (4, 4), (2, 4), (3, 4), (0, 6)],           # 2-3 runs back along 3-4
    'collinear_spike_overshooting': [(0, 0), (4, 0), (4, 4), (2, 4), (6, 4), (0, 6)],
    'vertex_on_a_far_edge': [(0, 0), (4, 0), (4, 4), (2, 0), (0, 4)],              # (2, 0) lies on the edge 0-1
    'zero_area': [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)],
    'zero_area_triangle': [(0, 0), (4, 0), (2, 0)],
    'infinite_coordinate': [(0, 0), (4, 0), (math.inf, 4), (0, 4), (-1, 2)],
    'nan_coordinate': [(0, 0), (4, 0), (4, math.nan), (0, 4), (-1, 2)],
    'two_points': [(0, 0), (4, 0)],
}
VALID = {'l_shape': L_SHAPE, 'comb': COMB, 'star': STAR, 'arrow': ARROW, 'triangle': [(0, 0), (4, 0), (0, 3)],
         'collinear_vertex_going_on': [(0, 0), (2, 0), (4, 0), (4, 4), (0, 4)]}   # a flat vertex is no spike


# ---- seeded polygons ----------------------------------------------------------------------------------------------------------------

STAR_VERTS = (3, 4, 5, 36, 63, 64)


def _finish(rng, q):
    k = rng.randrange(len(q))
    q = q[k:] + q[:k]
    if rng.random() < 0.5:
        q.reverse()
    return q


def random_star(rng, cx, cy, radius, verts):
    """A star-shaped (hence simple) polygon of `verts` vertices around (cx, cy): increasing angles, radii in [0.45, 1] * radius, so
    most of its vertices are reflex or nearly so.  Random orientation and start vertex."""
    while True:
        angles = sorted(rng.uniform(0.0, 2.0 * math.pi) for _ in range(verts))
        q = [(cx + r * math.cos(a), cy + r * math.sin(a)) for a, r in
             zip(angles, (rng.uniform(0.45, 1.0) * radius for _ in range(verts)))]
        if poly_valid(q) and poly_area(q) >= 16.0:
            return _finish(rng, q)


def random_ribbon(rng, cx, cy, radius, rulings):
    """The outline of a word on an arc: `rulings` (4 .. 18) top points forward, then the bottom points backward."""
    while True:
        half = rng.uniform(0.08, 0.2) * radius
        span, mid = rng.uniform(0.6, 2.4), rng.uniform(0.0, 2.0 * math.pi)
        angles = [mid + span * (k / (rulings - 1.0) - 0.5) for k in range(rulings)]
        top = [(cx + (radius + half) * math.cos(a), cy + (radius + half) * math.sin(a)) for a in angles]
        bot = [(cx + (radius - half) * math.cos(a), cy + (radius - half) * math.sin(a)) for a in angles]
        q = top + bot[::-1]
        if poly_valid(q) and poly_area(q) >= 16.0:
            return _finish(rng, q)


def random_polygon(rng, cx, cy, radius, verts=None):
    if verts is None and rng.random() < 0.5:
        return random_ribbon(rng, cx, cy, radius, rng.randrange(4, 19))
    return random_star(rng, cx, cy, radius, verts or rng.choice(STAR_VERTS))


def random_image(seed, n_gt, n_det, star_verts=()):
    """`_quad_eval_ref.random_image` with polygons, coordinates inside [0, 2048]: ground truths scattered over the canvas, some
    ignored (the first ones take their vertex counts from `star_verts`); detections that are a ground truth with jittered
    vertices, or moved and scaled (IoUs and covered fractions on both sides of the constraints), other polygons drawn over a
    ground truth, and strays."""
    rng = random.Random(seed)
    gts, dets = [], []
    for k in range(n_gt):
        gts.append(random_polygon(rng, rng.uniform(400, 1648), rng.uniform(400, 1648), rng.uniform(30, 150),
                                  star_verts[k] if k < len(star_verts) else None))
    ignores = [rng.random() < 0.25 for _ in gts]
    for _ in range(n_det):
        kind = rng.random()
        if kind < 0.85 and gts:
            base = gts[rng.randrange(len(gts))]
            cx, cy = sum(v[0] for v in base) / len(base), sum(v[1] for v in base) / len(base)
            size = max(math.hypot(v[0] - cx, v[1] - cy) for v in base)
        if kind < 0.3 and gts:
            while True:
                jitter = rng.uniform(0.0, 0.04) * size
                q = [(x + rng.uniform(-jitter, jitter), y + rng.uniform(-jitter, jitter)) for x, y in base]
                if poly_valid(q) and poly_area(q) >= 16.0:
                    break
            dets.append(q)
        elif kind < 0.6 and gts:
            scale, shift, ang = rng.uniform(0.7, 1.2), rng.uniform(0.0, 0.3) * size, rng.uniform(0.0, 2.0 * math.pi)
            dx, dy = shift * math.cos(ang), shift * math.sin(ang)
            dets.append([(cx + dx + scale * (x - cx), cy + dy + scale * (y - cy)) for x, y in base])
        elif kind < 0.85 and gts:
            dets.append(random_polygon(rng, cx + rng.uniform(-0.5, 0.5) * size, cy + rng.uniform(-0.5, 0.5) * size,
                                       size * rng.uniform(0.5, 1.2)))
        else:
            dets.append(random_polygon(rng, rng.uniform(400, 1648), rng.uniform(400, 1648), rng.uniform(30, 150)))
    assert all(0.0 <= c <= 2048.0 for q in gts + dets for v in q for c in v)
    return gts, ignores, dets


def image_with_margin(seed, n_gt, n_det, star_verts=()):
    """The image of `seed`, redrawn from seed + 1000 while an IoU or a covered fraction lies within MARGIN of 0.5:
    (gts, ignores, dets, evaluate_image(...), times redrawn)."""
    redrawn = 0
    while True:
        gts, ignores, dets = random_image(seed, n_gt, n_det, star_verts)
        want = evaluate_image(gts, ignores, dets)
        if want['margin'] >= MARGIN:
            return gts, ignores, dets, want, redrawn
        redrawn += 1
        seed += 1000
