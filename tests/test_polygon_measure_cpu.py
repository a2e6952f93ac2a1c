"""The float64 restatement of `mr_poly_iou` (tests/_poly_eval_ref.py) checked on its own, without a GPU, two independent ways:
against the same signed-fan sum in exact rational arithmetic (`fractions.Fraction`: what the restatement would give without
rounding) and against point counting on a fine grid with an even-odd test (another algorithm, which knows nothing of fans or
clipping), with hand-computed answers for the shapes a convex-only method gets wrong.

Tolerance of an intersection area, derived, not measured.  Both polygons are translated by the ground truth's first vertex
before any product, so every coordinate the arithmetic sees is at most E, the larger side of the box around the pair, and every
product of two coordinate differences at most 2 E^2.  One triangle-triangle clip is about 50 such operations, each rounded by at
most 2^-53 relative to a value of at most 2 E^2, with a factor 2 for the values that pass through an interpolated vertex:
50 * 2 * 2^-53 * 2 E^2 = 100 * 2^-52 * E^2 per term.  A pair of polygons of m and n vertices has (m - 2)(n - 2) < m n terms, whose
errors add at worst: tol(m, n, E) = 100 * m * n * 2^-52 * E^2 (`_poly_eval_ref.area_tol`).  An IoU is a / U with U = gt_area +
det_area - a >= a: its error is at most da / U + a dU / U^2 <= 4 tol / U (dU <= 3 tol), plus the division's own rounding."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import _poly_eval_ref as P
import _quad_eval_ref as R

L_SHAPE, COMB, STAR, ARROW, HAND, INVALID, VALID = P.L_SHAPE, P.COMB, P.STAR, P.ARROW, P.HAND, P.INVALID, P.VALID


def _exact_intersection(p, q):
    """The signed-fan sum in exact rational arithmetic, written on its own (plain double loop, no lanes, no box tests)."""
    def pts(a):
        return [(Fraction(x), Fraction(y)) for x, y in a]

    def o2(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])

    def cut(poly, a, b):
        out = []
        for k in range(len(poly)):
            u, v = poly[k - 1], poly[k]
            du, dv = o2(a, b, u), o2(a, b, v)
            if du * dv < 0:
                t = du / (du - dv)
                out.append((u[0] + t * (v[0] - u[0]), u[1] + t * (v[1] - u[1])))
            if dv >= 0:
                out.append(v)
        return out

    def area2(poly):
        return sum(poly[k - 1][0] * poly[k][1] - poly[k][0] * poly[k - 1][1] for k in range(len(poly))) if poly else Fraction(0)

    p, q = pts(p), pts(q)
    total = Fraction(0)
    for i in range(1, len(p) - 1):
        s = [p[0], p[i], p[i + 1]]
        so = o2(*s)
        if so == 0:
            continue
        if so < 0:
            s = [s[0], s[2], s[1]]
        for j in range(1, len(q) - 1):
            c = [q[0], q[j], q[j + 1]]
            co = o2(*c)
            if co == 0:
                continue
            if co < 0:
                c = [c[0], c[2], c[1]]
            piece = s
            for k in range(3):
                piece = cut(piece, c[k], c[(k + 1) % 3])
            total += abs(area2(piece)) * (1 if (so > 0) == (co > 0) else -1)
    return abs(total) / 2


def _exact_area(p):
    return abs(sum(Fraction(p[k - 1][0]) * Fraction(p[k][1]) - Fraction(p[k][0]) * Fraction(p[k - 1][1])
                   for k in range(len(p)))) / 2


def _inside(poly, xx, yy):
    """Even-odd point-in-polygon test of the grid points (xx, yy)."""
    inside = np.zeros(xx.shape, dtype=bool)
    for k in range(len(poly)):
        (x0, y0), (x1, y1) = poly[k - 1], poly[k]
        if y0 == y1:
            continue
        crosses = (y0 > yy) != (y1 > yy)
        inside ^= crosses & (xx < x0 + (yy - y0) * (x1 - x0) / (y1 - y0))
    return inside


def _counted(p, q, cells=1200):
    """(area of the intersection by counting cell centres, its tolerance).  A segment of length l crosses at most
    sqrt(2) l / h + 1 cells of side h, and only a cell that an edge of p or q crosses can be counted wrongly, by at most h^2:
    tol = h * (sqrt(2) * (perimeter of p + perimeter of q) + (m + n) * h)."""
    xs, ys = [v[0] for v in p + q], [v[1] for v in p + q]
    h = max(max(xs) - min(xs), max(ys) - min(ys)) / cells
    gx = min(xs) + h * (np.arange(int((max(xs) - min(xs)) / h) + 1) + 0.5)
    gy = min(ys) + h * (np.arange(int((max(ys) - min(ys)) / h) + 1) + 0.5)
    xx, yy = np.meshgrid(gx, gy)
    per = sum(math.hypot(a[k][0] - a[k - 1][0], a[k][1] - a[k - 1][1]) for a in (p, q) for k in range(len(a)))
    return float((_inside(p, xx, yy) & _inside(q, xx, yy)).sum()) * h * h, h * (math.sqrt(2.0) * per + (len(p) + len(q)) * h)


def _floats(p):
    return [(float(x), float(y)) for x, y in p]


def _variants(p):
    """The same polygon from other start vertices and in the other orientation."""
    p = list(p)
    k = len(p) // 2
    return [p, p[1:] + p[:1], p[k:] + p[:k], p[::-1], (p[k + 1:] + p[:k + 1])[::-1]]


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_computed_answers(name):
    p, q, area_p, area_q, want = HAND[name]
    assert _exact_area(p) == area_p and _exact_area(q) == area_q
    assert _exact_intersection(p, q) == want and _exact_intersection(q, p) == want
    for vp in _variants(_floats(p)):
        for vq in _variants(_floats(q)):
            assert P.poly_valid(vp) and P.poly_valid(vq)
            assert P.poly_area(vp) == area_p and P.poly_area(vq) == area_q
            assert abs(P.poly_intersection(vp, vq) - want) <= P.area_tol(vp, vq), (name, vp[0], vq[0])
            assert abs(P.poly_intersection(vq, vp) - want) <= P.area_tol(vp, vq), (name, vp[0], vq[0])
    counted, tol = _counted(_floats(p), _floats(q))
    assert abs(counted - want) <= tol and tol < 0.05 * (area_p + area_q), (counted, want, tol)


def test_a_polygon_with_itself_gives_its_area():
    rng = random.Random(5)
    for verts in (3, 5, 14, 36, 64):
        p = P.random_star(rng, 1000.0, 900.0, 120.0, verts)
        assert abs(P.poly_intersection(p, p) - P.poly_area(p)) <= P.area_tol(p, p)
        assert abs(P.poly_intersection(p, p[::-1]) - P.poly_area(p)) <= P.area_tol(p, p)
    p = P.random_ribbon(rng, 700.0, 1200.0, 140.0, 18)
    assert abs(P.poly_intersection(p, p[7:] + p[:7]) - P.poly_area(p)) <= P.area_tol(p, p)


def _integer_pairs():
    """Seeded overlapping pairs with INTEGER coordinates up to 2048 (exactly representable, so the rational sum is the truth):
    stars and ribbon outlines of 3 .. 64 vertices, the second one drawn over the first."""
    rng = random.Random(11)

    def draw(k, cx, cy, radius):
        if k % 2 == 0 and 8 <= k <= 36 and rng.random() < 0.6:
            return P.random_ribbon(rng, cx, cy, radius, k // 2)
        return P.random_star(rng, cx, cy, radius, k)
    pairs = []
    for m, n in ((3, 3), (4, 5), (5, 14), (14, 14), (36, 8), (12, 36), (28, 36), (64, 5), (36, 64), (63, 64)):
        while True:
            cx, cy, radius = rng.uniform(300, 1700), rng.uniform(300, 1700), rng.uniform(100, 250)
            p = [(float(round(x)), float(round(y))) for x, y in draw(m, cx, cy, radius)]
            q = [(float(round(x)), float(round(y))) for x, y in
                 draw(n, cx + rng.uniform(-0.4, 0.4) * radius, cy + rng.uniform(-0.4, 0.4) * radius, radius * rng.uniform(0.6, 1.2))]
            if P.poly_valid(p) and P.poly_valid(q) and not P._disjoint(p, q):
                break
        pairs.append((p, q))
    return pairs


def test_the_restatement_is_inside_the_derived_bound_of_exact_rational_arithmetic():
    worst = 0.0
    for p, q in _integer_pairs():
        want = _exact_intersection(p, q)
        got = P.poly_intersection(p, q)
        err, tol = abs(Fraction(got) - want), P.area_tol(p, q)
        worst = max(worst, float(err) / tol)
        print("m = %2d, n = %2d, E = %6.1f: exact %.6f, restatement off by %.3e (bound %.3e)"
              % (len(p), len(q), P.extent(p, q), float(want), float(err), tol))
        assert err <= tol
        assert abs(Fraction(P.poly_area(p)) - _exact_area(p)) <= tol and 0 <= want <= min(_exact_area(p), _exact_area(q))
    print("largest error / bound: %.3e" % worst)


def test_the_restatement_agrees_with_point_counting():
    """Float coordinates at the scale of a photo; the grid knows nothing of triangles."""
    rng = random.Random(23)
    for k in range(8):
        while True:                                              # (until the two overlap by more than a sliver)
            cx, cy, radius = rng.uniform(400, 1600), rng.uniform(400, 1600), rng.uniform(40, 150)
            p = P.random_polygon(rng, cx, cy, radius)
            q = P.random_polygon(rng, cx + rng.uniform(-0.4, 0.4) * radius, cy + rng.uniform(-0.4, 0.4) * radius,
                                 radius * rng.uniform(0.6, 1.2))
            got = P.poly_intersection(p, q)
            if got >= 0.05 * (P.poly_area(p) + P.poly_area(q)):
                break
        counted, tol = _counted(p, q)
        print("m = %2d, n = %2d: restatement %.3f, counted %.3f (tolerance %.3f)" % (len(p), len(q), got, counted, tol))
        assert abs(got - counted) <= tol and tol < 0.05 * (P.poly_area(p) + P.poly_area(q))
        area, tol_p = _counted(p, p)
        assert abs(P.poly_area(p) - area) <= tol_p


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_polygons(name):
    for v in _variants(_floats(INVALID[name])):
        assert not P.poly_valid(v), v


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_polygons(name):
    for v in _variants(_floats(VALID[name])):
        assert P.poly_valid(v), v


def test_quads_follow_the_quad_rule_and_its_known_answers():
    """On 4-gons the polygon rule is the quad rule, and the bookkeeping gives the known answers of _quad_eval_ref.CASES."""
    rng = random.Random(3)
    quads = [R.random_quad(rng, 1000.0, 1000.0, 80.0, k % 2 == 1) for k in range(20)]
    quads += [[(0, 0), (4, 4), (4, 0), (0, 2)], [(0, 0), (1, 1), (2, 2), (3, 3)], [(0, 0), (4, 0), (2, 0), (2, 3)],
              [(0, 0), (4, 0), (4, 0), (0, 3)], [(0, 0), (4, 0), (1, 0), (0, 3)]]
    for q in quads:
        q = _floats(q)
        assert P.poly_valid(q) == R.quad_valid(q), q
        if R.quad_valid(q):
            assert P.poly_area(q) == R.quad_area(q)
    for a in quads[:20]:
        for b in quads[:20]:
            assert abs(P.poly_intersection(a, b) - R.quad_intersection(a, b)) <= P.area_tol(a, b)
    for name, (gts, ignores, dets, want) in R.CASES.items():
        got = P.evaluate_image(gts, ignores, dets)
        for key, value in want.items():
            if key == 'iouMat':
                assert np.allclose(np.array(got[key]).reshape(-1), np.array(value).reshape(-1), rtol=0, atol=1e-12), name
            elif isinstance(value, float):
                assert abs(got[key] - value) <= 1e-15, (name, key)
            else:
                assert got[key] == value, (name, key)


def test_the_seeded_images_keep_their_margin():
    gts, ignores, dets, want, redrawn = P.image_with_margin(300, 5, 7, P.STAR_VERTS)
    assert [len(q) for q in gts][:5] == list(P.STAR_VERTS)[:5] and want['margin'] >= P.MARGIN and redrawn <= 2
    assert all(want['gt_valid']) and all(want['det_valid'])
