"""Float64 restatement, in plain Python, of what megreader_amd.ops.detection_measure computes: validity and area of a
quadrilateral, the area of the intersection of two quadrilaterals, and the per-image bookkeeping of the reference's
`DetectionIoUEvaluator.evaluate_image` (concern/icdar2015_eval/detection/iou.py) -- the checker of
tests/test_quad_measure_gpu.py, itself checked against hand-computed answers and point-counting estimates in
tests/test_quad_measure_cpu.py.  Helper module: no tests are collected from it.

Every operation is one IEEE float64 operation on Python floats, written in the order the description of the kernels
gives, so the device results may differ from these only by the rounding of differently ordered sums."""
import math
import random


def orient2(p, q, r):
    """Twice the signed area of the triangle p, q, r (> 0: counter-clockwise, y up)."""
    return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])


def _in_box(a, b, p):
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def segments_touch(a, b, c, d):
    """Do the closed segments a-b and c-d share a point?"""
    o1, o2, o3, o4 = orient2(a, b, c), orient2(a, b, d), orient2(c, d, a), orient2(c, d, b)
    if ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0)):
        return True
    return (o1 == 0 and _in_box(a, b, c)) or (o2 == 0 and _in_box(a, b, d)) or \
           (o3 == 0 and _in_box(c, d, a)) or (o4 == 0 and _in_box(c, d, b))


def area2(q):
    """Twice the signed shoelace area of a polygon given as [(x, y), ...]."""
    s = 0.0
    for k in range(len(q)):
        (x0, y0), (x1, y1) = q[k], q[(k + 1) % len(q)]
        s += x0 * y1 - x1 * y0
    return s


def quad_valid(q):
    """The stated rule for a 4-gon: non-zero (finite) area, and no pair of opposite edges intersects or touches."""
    a = abs(area2(q))
    if not (a > 0.0 and a < math.inf):
        return False
    return not segments_touch(q[0], q[1], q[2], q[3]) and not segments_touch(q[1], q[2], q[3], q[0])


def quad_area(q):
    return 0.5 * abs(area2(q))


def quad_triangles(q):
    """The two counter-clockwise triangles of a simple quad, split along the diagonal that lies inside it."""
    sgn = 1.0 if area2(q) > 0.0 else -1.0
    if sgn * orient2(q[0], q[1], q[2]) >= 0.0 and sgn * orient2(q[0], q[2], q[3]) >= 0.0:
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        tris = [[q[1], q[2], q[3]], [q[1], q[3], q[0]]]
    if sgn < 0.0:
        tris = [[t[0], t[2], t[1]] for t in tris]
    return tris


def clip_left_of(poly, a, b):
    """Sutherland-Hodgman step: the part of `poly` on the left of, or on, the line a -> b."""
    out = []
    if not poly:
        return out
    p = poly[-1]
    dp = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    for q in poly:
        dq = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
        if (dp > 0.0 and dq < 0.0) or (dp < 0.0 and dq > 0.0):
            t = dp / (dp - dq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if dq >= 0.0:
            out.append(q)
        p, dp = q, dq
    return out


def triangle_overlap(s, c):
    if orient2(*s) == 0.0 or orient2(*c) == 0.0:
        return 0.0
    poly = list(s)
    for k in range(3):
        poly = clip_left_of(poly, c[k], c[(k + 1) % 3])
    if len(poly) < 3:
        return 0.0
    bx, by = poly[0]
    total = 0.0
    for k in range(1, len(poly) - 1):
        total += (poly[k][0] - bx) * (poly[k + 1][1] - by) - (poly[k + 1][0] - bx) * (poly[k][1] - by)
    return 0.5 * abs(total)


def quad_intersection(p, q):
    """Area of the intersection of two valid quads (any orientation, convex or not)."""
    if max(v[0] for v in p) < min(v[0] for v in q) or max(v[0] for v in q) < min(v[0] for v in p) or \
            max(v[1] for v in p) < min(v[1] for v in q) or max(v[1] for v in q) < min(v[1] for v in p):
        return 0.0
    tp, tq = quad_triangles(p), quad_triangles(q)
    a = triangle_overlap(tp[0], tq[0])
    a += triangle_overlap(tp[0], tq[1])
    a += triangle_overlap(tp[1], tq[0])
    a += triangle_overlap(tp[1], tq[1])
    return a


def point_in_quad(q, x, y):
    """Even-odd rule; for the point-counting estimates of the CPU tests (independent of the clipping above)."""
    inside = False
    for k in range(4):
        (x0, y0), (x1, y1) = q[k], q[(k + 1) % 4]
        if (y0 > y) != (y1 > y) and x < x0 + (y - y0) * (x1 - x0) / (y1 - y0):
            inside = not inside
    return inside


def evaluate_image(gts, ignores, dets, iou_constraint=0.5, area_precision_constraint=0.5):
    """gts / dets: lists of quads [(x, y)] * 4, ignores: flags of the gts.  The reference's bookkeeping; indices are
    positions in the lists of valid quads.  Also returns the full matrices by GIVEN index for the comparison with the
    device arrays, and the margins of every decision taken from a threshold."""
    gts = [[(float(x), float(y)) for x, y in q] for q in gts]
    dets = [[(float(x), float(y)) for x, y in q] for q in dets]
    gt_valid = [quad_valid(q) for q in gts]
    det_valid = [quad_valid(q) for q in dets]
    gt_area = [quad_area(q) if v else 0.0 for q, v in zip(gts, gt_valid)]
    det_area = [quad_area(q) if v else 0.0 for q, v in zip(dets, det_valid)]
    inter = [[0.0] * len(dets) for _ in gts]
    iou = [[0.0] * len(dets) for _ in gts]
    for g, p in enumerate(gts):
        for d, q in enumerate(dets):
            if gt_valid[g] and det_valid[d]:
                a = quad_intersection(p, q)
                inter[g][d] = a
                iou[g][d] = a / (gt_area[g] + det_area[d] - a)
    gi = [g for g, v in enumerate(gt_valid) if v]
    di = [d for d, v in enumerate(det_valid) if v]
    gt_dontcare = [cg for cg, g in enumerate(gi) if ignores[g]]
    det_dontcare = []
    margin = math.inf
    for cd, d in enumerate(di):
        hit = False
        for cg in gt_dontcare:
            hit = hit or (det_area[d] != 0 and inter[gi[cg]][d] / det_area[d] > area_precision_constraint)
        if hit:
            det_dontcare.append(cd)
    for g in gi:
        for d in di:
            margin = min(margin, abs(iou[g][d] - iou_constraint),
                         abs(inter[g][d] / det_area[d] - area_precision_constraint))
    pairs, taken = [], set()
    for cg, g in enumerate(gi):
        if cg in gt_dontcare:
            continue
        for cd, d in enumerate(di):
            if cd not in taken and cd not in det_dontcare and iou[g][d] > iou_constraint:
                taken.add(cd)
                pairs.append({'gt': cg, 'det': cd})
                break
    gt_care, det_care, matched = len(gi) - len(gt_dontcare), len(di) - len(det_dontcare), len(pairs)
    if gt_care == 0:
        recall, precision = 1.0, (0.0 if det_care > 0 else 1.0)
    else:
        recall = float(matched) / gt_care
        precision = 0.0 if det_care == 0 else float(matched) / det_care
    hmean = 0.0 if precision + recall == 0 else 2.0 * precision * recall / (precision + recall)
    return {'precision': precision, 'recall': recall, 'hmean': hmean, 'pairs': pairs, 'gtCare': gt_care,
            'detCare': det_care, 'detMatched': matched, 'gtDontCare': gt_dontcare, 'detDontCare': det_dontcare,
            'iouMat': [[iou[g][d] for d in di] for g in gi],
            'gt_valid': gt_valid, 'det_valid': det_valid, 'gt_area': gt_area, 'det_area': det_area, 'inter': inter,
            'iou': iou, 'margin': margin}


def random_quad(rng, cx, cy, radius, concave):
    """A valid quad around (cx, cy) inside [0, 2048]^2 with area >= 16: four points at increasing angles (a star-shaped,
    hence simple, polygon); `concave` pulls one vertex towards the centre until it is a reflex vertex.  Orientation and
    starting vertex are random."""
    while True:
        angles = sorted(rng.uniform(0.0, 2.0 * math.pi) for _ in range(4))
        radii = [rng.uniform(0.5, 1.0) * radius for _ in range(4)]
        if concave:
            radii[rng.randrange(4)] *= rng.uniform(0.05, 0.3)
        q = [(min(2048.0, max(0.0, cx + r * math.cos(a))), min(2048.0, max(0.0, cy + r * math.sin(a))))
             for a, r in zip(angles, radii)]
        k = rng.randrange(4)
        q = q[k:] + q[:k]
        if rng.random() < 0.5:
            q.reverse()
        if not quad_valid(q) or quad_area(q) < 16.0:
            continue
        turns = [orient2(q[i], q[(i + 1) % 4], q[(i + 2) % 4]) for i in range(4)]
        is_concave = min(turns) < 0.0 < max(turns)
        if is_concave == concave:
            return q


def random_image(seed, n_gt, n_det):
    """Ground truths scattered over the canvas, some ignored; detections that are ground truths with jittered vertices
    (IoUs on both sides of the constraint), other quads drawn over a ground truth (covered fractions on both sides)
    and strays."""
    rng = random.Random(seed)
    gts, dets = [], []
    for _ in range(n_gt):
        gts.append(random_quad(rng, rng.uniform(100, 1948), rng.uniform(100, 1948), rng.uniform(20, 120),
                               rng.random() < 0.4))
    ignores = [rng.random() < 0.25 for _ in gts]
    for _ in range(n_det):
        kind = rng.random()
        if kind < 0.4 and gts:
            base = gts[rng.randrange(len(gts))]
            size = max(math.hypot(v[0] - base[0][0], v[1] - base[0][1]) for v in base)
            while True:
                jitter = rng.uniform(0.02, 0.25) * size
                q = [(min(2048.0, max(0.0, x + rng.uniform(-jitter, jitter))),
                      min(2048.0, max(0.0, y + rng.uniform(-jitter, jitter)))) for x, y in base]
                if quad_valid(q) and quad_area(q) >= 16.0:
                    break
            dets.append(q)
        elif kind < 0.75 and gts:
            base = gts[rng.randrange(len(gts))]
            cx, cy = sum(v[0] for v in base) / 4.0, sum(v[1] for v in base) / 4.0
            size = max(math.hypot(v[0] - cx, v[1] - cy) for v in base)
            shift = rng.uniform(0.0, 0.6) * size
            ang = rng.uniform(0.0, 2.0 * math.pi)
            dets.append(random_quad(rng, min(1948.0, max(100.0, cx + shift * math.cos(ang))),
                                    min(1948.0, max(100.0, cy + shift * math.sin(ang))),
                                    size * rng.uniform(0.5, 1.3), rng.random() < 0.4))
        else:
            dets.append(random_quad(rng, rng.uniform(100, 1948), rng.uniform(100, 1948), rng.uniform(20, 120),
                                    rng.random() < 0.4))
    return gts, ignores, dets


# The random-parity images of tests/test_quad_measure_gpu.py (case 8).  An image whose smallest distance of an IoU or of a
# covered fraction from 0.5 is below MARGIN is redrawn from the next seed (seed + 1000); at most REDRAW_CAP of the images
# may need that.
PARITY_SEEDS = tuple(range(200, 232))
PARITY_SHAPE = (8, 10)          # ground truths, detections per image: 32 * 18 = 576 quads, 2 560 pairs
MARGIN = 1e-3
REDRAW_CAP = 0.05


def parity_images():
    """[(gts, ignores, dets, evaluate_image(...))] for PARITY_SEEDS, the number of redrawn images, the smallest margin."""
    images, redrawn, smallest = [], 0, math.inf
    for seed in PARITY_SEEDS:
        while True:
            gts, ignores, dets = random_image(seed, *PARITY_SHAPE)
            want = evaluate_image(gts, ignores, dets)
            if want['margin'] >= MARGIN:
                break
            redrawn += 1
            seed += 1000
        smallest = min(smallest, want['margin'])
        images.append((gts, ignores, dets, want))
    return images, redrawn, smallest


def box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _pairs(*gd):
    return [{'gt': g, 'det': d} for g, d in gd]


# Known answers, all derivable by hand: name -> (gts, ignore flags, dets, expected values of evaluate_image / QuadMeasurer).
CASES = {
    # the self-test at the end of the reference's iou.py: the detection is the unit square with one corner pulled in
    'selftest': ([box(0, 0, 1, 1), box(2, 2, 3, 3)], [0, 0], [[(0.1, 0.1), (1, 0), (1, 1), (0, 1)]],
                 dict(precision=1.0, recall=0.5, hmean=2.0 / 3.0, pairs=_pairs((0, 0)), gtCare=2, detCare=1, detMatched=1,
                      gtDontCare=[], detDontCare=[], iouMat=[[0.9], [0.0]])),
    # greedy, not optimal: height-1 boxes on x-intervals, gt0 [1,10] gt1 [5,14], det0 [2,12] det1 [0,8]; gt0 takes det0
    # (8/11), which leaves gt1 only det1 (3/14); the optimal assignment gt0-det1 (7/10), gt1-det0 (7/12) would match 2
    'greedy': ([box(1, 0, 10, 1), box(5, 0, 14, 1)], [0, 0], [box(2, 0, 12, 1), box(0, 0, 8, 1)],
               dict(precision=0.5, recall=0.5, hmean=0.5, pairs=_pairs((0, 0)), gtCare=2, detCare=2, detMatched=1,
                    gtDontCare=[], detDontCare=[], iouMat=[[8.0 / 11.0, 7.0 / 10.0], [7.0 / 12.0, 3.0 / 14.0]])),
    # gt0 ignored; det0 has 80 % of its area in gt0 (don't-care), det1 40 % (care, false positive), det2 matches gt1
    'dontcare': ([box(0, 0, 10, 10), box(20, 0, 30, 10)], [1, 0], [box(2, 2, 12, 8), box(6, 1, 16, 9), box(21, 0, 30, 10)],
                 dict(precision=0.5, recall=1.0, hmean=2.0 / 3.0, pairs=_pairs((1, 2)), gtCare=1, detCare=2, detMatched=1,
                      gtDontCare=[0], detDontCare=[0])),
    # the don't-care detection (90 % inside the ignored gt0) is identical to the care gt1: it still must not match
    'dontcare_blocks_match': ([box(0, 0, 10, 10), box(1, 0, 11, 10)], [1, 0], [box(1, 0, 11, 10)],
                              dict(precision=0.0, recall=0.0, hmean=0.0, pairs=[], gtCare=1, detCare=0, detMatched=0,
                                   gtDontCare=[0], detDontCare=[0], iouMat=[[9.0 / 11.0], [1.0]])),
    'empty_both': ([], [], [], dict(precision=1.0, recall=1.0, hmean=1.0, pairs=[], gtCare=0, detCare=0, detMatched=0,
                                    gtDontCare=[], detDontCare=[], iouMat=[])),
    'empty_only_ignored_gts': ([box(0, 0, 10, 10), box(20, 0, 30, 10)], [1, 1], [box(50, 50, 60, 60)],
                               dict(precision=0.0, recall=1.0, hmean=0.0, pairs=[], gtCare=0, detCare=1, detMatched=0,
                                    gtDontCare=[0, 1], detDontCare=[], iouMat=[[0.0], [0.0]])),
    'empty_no_dets': ([box(0, 0, 10, 10), box(20, 0, 30, 10)], [0, 0], [],
                      dict(precision=0.0, recall=0.0, hmean=0.0, pairs=[], gtCare=2, detCare=0, detMatched=0,
                           gtDontCare=[], detDontCare=[], iouMat=[])),
    # a bow-tie gt (edges 0-1 and 2-3 cross) and a zero-area detection are dropped; the indices are those of the lists
    # of valid quads: gts (1, 2) -> (0, 1), dets (1, 2) -> (0, 1)
    'invalid': ([[(0, 0), (4, 4), (4, 0), (0, 2)], box(10, 0, 20, 10), box(30, 0, 40, 10)], [0, 0, 0],
                [[(0, 0), (1, 1), (2, 2), (3, 3)], box(30, 0, 40, 9), box(10, 0, 20, 9)],
                dict(precision=1.0, recall=1.0, hmean=1.0, pairs=_pairs((0, 1), (1, 0)), gtCare=2, detCare=2, detMatched=2,
                     gtDontCare=[], detDontCare=[], iouMat=[[0.0, 0.9], [0.9, 0.0]])),
}
EMPTY_BATCH = ('empty_both', 'empty_only_ignored_gts', 'empty_no_dets')
