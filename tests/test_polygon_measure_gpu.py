"""Polygon detection metrics on the GPU (csrc/quad_measure.hip: mr_poly_iou, then the mr_quad_match of the quads) through
megreader_amd.ops.detection_measure.polygon_measure and megreader_amd.structure.PolygonMeasurer, against the float64 restatement
of tests/_poly_eval_ref.py (itself checked against exact rational arithmetic, point counting and hand-computed answers in
tests/test_polygon_measure_cpu.py, where the tolerance is derived).

Tolerance, per pair: an intersection area within tol(m, n, E) = 100 * m * n * 2^-52 * E^2 (m, n the vertex counts, E the larger
side of the box around the pair), an IoU within 4 tol / union + 4 * 2^-52, a polygon's own area within tol(m, m, E).  Flags,
counts, pairs and don't-care sets must be equal: every image keeps its IoUs and covered fractions at least MARGIN = 1e-3 from the
constraints, asserted on the restatement's side."""
import functools
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _db_ribbon_ref as RR  # noqa: E402
import _poly_eval_ref as P  # noqa: E402
import _quad_eval_ref as R  # noqa: E402
from megreader_amd.ops.detection_measure import QuadOutputs, polygon_measure, quad_measure  # noqa: E402
from megreader_amd.structure import PolygonMeasurer, QuadMeasurer, Ribbon, SegDetectorRepresenter  # noqa: E402
from megreader_amd.structure.polygon_measurer import outlines_of  # noqa: E402

DEV = "cuda"
KEYS = ('precision', 'recall', 'hmean', 'pairs', 'gtCare', 'detCare', 'detMatched', 'gtDontCare', 'detDontCare')


def _floats(p):
    return [(float(x), float(y)) for x, y in p]


def _upload(images, V=None, G=None, D=None):
    """[(gts, ignores, dets)] -> the padded device arrays of polygon_measure (+ G, D, V)."""
    N = len(images)
    G = max([1] + [len(g) for g, _, _ in images]) if G is None else G
    D = max([1] + [len(d) for _, _, d in images]) if D is None else D
    V = max([3] + [len(q) for g, _, d in images for q in g + d]) if V is None else V
    gt, det = np.zeros((N, G, V, 2)), np.zeros((N, D, V, 2))
    gt_verts, det_verts = np.zeros((N, G), dtype=np.int32), np.zeros((N, D), dtype=np.int32)
    ignore = np.zeros((N, G), dtype=np.int32)
    for n, (gts, ignores, dets) in enumerate(images):
        for points, verts, polys in ((gt, gt_verts, gts), (det, det_verts, dets)):
            for k, q in enumerate(polys):
                points[n, k, :min(len(q), V)] = np.array(q, dtype=np.float64)[:V]
                verts[n, k] = len(q)
        ignore[n, :len(gts)] = np.array(ignores, dtype=np.int64) != 0
    counts = [np.array([len(im[k]) for im in images], dtype=np.int32) for k in (0, 2)]
    return [torch.from_numpy(a).to(DEV) for a in (gt, gt_verts, counts[0], ignore, det, det_verts, counts[1])], G, D, V


def _check_image(r, n, image, want, G, D):
    """Every slot of every output of image n against the restatement's values; padding slots against the stated zeros.  Returns
    the largest error as a share of its tolerance."""
    gts, dets = [_floats(q) for q in image[0]], [_floats(q) for q in image[2]]
    worst = 0.0
    for key, width, polys in (('gt_valid', G, gts), ('det_valid', D, dets)):
        expect = np.zeros(width, dtype=np.int32)
        expect[:len(polys)] = want[key]
        assert (r[key][n] == expect).all(), (n, key, r[key][n], expect)
    for key, width, polys in (('gt_area', G, gts), ('det_area', D, dets)):
        for k in range(width):
            if k < len(polys) and want[key.replace('area', 'valid')][k]:
                worst = max(worst, abs(r[key][n, k] - want[key][k]) / P.area_tol(polys[k], polys[k]))
            else:
                assert r[key][n, k] == 0.0, (n, key, k)
    for g in range(G):
        for d in range(D):
            if g < len(gts) and d < len(dets) and want['gt_valid'][g] and want['det_valid'][d]:
                tol = P.area_tol(gts[g], dets[d])
                union = want['gt_area'][g] + want['det_area'][d] - want['inter'][g][d]
                worst = max(worst, abs(r['inter'][n, g, d] - want['inter'][g][d]) / tol,
                            abs(r['iou'][n, g, d] - want['iou'][g][d]) / (4.0 * tol / union + 4.0 * P.EPS))
            else:
                assert r['inter'][n, g, d] == 0.0 and r['iou'][n, g, d] == 0.0, (n, g, d)
    assert worst <= 1.0, (n, worst)
    ng = sum(want['gt_valid'])
    assert r['counts'][n].tolist() == [want['gtCare'], want['detCare'], want['detMatched'], ng], n
    assert r['scores'][n].tolist() == [want['precision'], want['recall'], want['hmean']], n
    match = np.full(G, -1, dtype=np.int32)
    for pair in want['pairs']:
        match[pair['gt']] = pair['det']
    assert (r['match_det'][n] == match).all(), n
    for key, width, flagged in (('gt_dontcare', G, want['gtDontCare']), ('det_dontcare', D, want['detDontCare'])):
        expect = np.zeros(width, dtype=np.int32)
        expect[flagged] = 1
        assert (r[key][n] == expect).all(), (n, key)
    return worst


def _run(images, V=None):
    """polygon_measure into outputs pre-filled with a sentinel -> host arrays, G, D."""
    args, G, D, V = _upload(images, V)
    out = QuadOutputs(len(images), G, D, torch.device(DEV))
    out.packed.fill_(0xCD)                                    # i32 -842150451, f64 -6.3e66: every element must be written
    assert polygon_measure(*args, out=out) is out
    return out.to_host(), G, D


def _variants(p):
    p = list(p)
    k = len(p) // 2
    return [p, p[1:] + p[:1], p[k:] + p[:k], p[::-1], (p[k + 1:] + p[:k + 1])[::-1]]


def test_hand_computed_answers_in_every_orientation_and_from_every_start():
    """The committed pairs of the CPU test, each as an image of one ground truth and five detections (the second polygon from
    other start vertices and in the other orientation), and once more with the ground truth turned as well."""
    names = sorted(P.HAND)
    images = []
    for name in names:
        p, q = P.HAND[name][:2]
        images.append(([p], [0], _variants(q)))
        images.append(([_variants(p)[4]], [0], _variants(q)))
        images.append(([q], [0], _variants(p)))
    r, G, D = _run(images)
    for n, image in enumerate(images):
        p, q, area_p, area_q, inter = P.HAND[names[n // 3]]
        if n % 3 == 2:
            area_p, area_q = area_q, area_p
        want = P.evaluate_image(*image)
        _check_image(r, n, image, want, G, D)
        assert r['gt_area'][n, 0] == area_p and (r['det_area'][n] == area_q).all()
        assert np.abs(r['inter'][n, 0] - inter).max() <= P.area_tol(_floats(p), _floats(q)), names[n // 3]


def test_validity_cases():
    names_bad, names_good = sorted(P.INVALID), sorted(P.VALID)
    polys = [v for name in names_bad + names_good for v in _variants(P.INVALID.get(name) or P.VALID[name])]
    image = (polys, [0] * len(polys), polys[::-1])
    r, G, D = _run([image])
    expect = [0] * (5 * len(names_bad)) + [1] * (5 * len(names_good))
    assert r['gt_valid'][0].tolist() == expect and r['det_valid'][0].tolist() == expect[::-1]
    assert [int(P.poly_valid(_floats(v))) for v in polys] == expect
    assert (r['gt_area'][0][:5 * len(names_bad)] == 0.0).all() and (r['inter'][0][:5 * len(names_bad)] == 0.0).all()


# (ground truths, detections) per image: 0, 1, 5 and 7 of each; the star-shaped ground truths come first and take 3, 4, 5, 36, 63
# and 64 vertices in turn, the rest and the detections are stars and ribbon outlines of 4 .. 18 rulings
MIXED = (((5, 7), (7, 5), (1, 0)), ((0, 1), (7, 7)), ((0, 0), (1, 1), (5, 5)), ((7, 7), (7, 5), (5, 7)))


@functools.lru_cache(maxsize=None)
def _mixed(batch):
    images, redrawn = [], 0
    for k, (n_gt, n_det) in enumerate(MIXED[batch]):
        verts = P.STAR_VERTS if k % 2 == 0 else P.STAR_VERTS[::-1]
        gts, ignores, dets, want, again = P.image_with_margin(400 + 10 * batch + k, n_gt, n_det, verts)
        redrawn += again
        images.append(((gts, ignores, dets), want))
    return images, redrawn


@pytest.mark.parametrize("batch", range(len(MIXED)))
def test_random_parity_with_the_restatement_mixed_vertex_counts_and_padding(batch):
    images, redrawn = _mixed(batch)
    smallest = min(want['margin'] for _, want in images)
    print("redrawn %d of %d images, smallest margin %.3e" % (redrawn, len(images), smallest))
    assert smallest >= P.MARGIN and redrawn <= len(images)
    r, G, D = _run([im for im, _ in images], V=64)
    worst = max(_check_image(r, n, im, want, G, D) for n, (im, want) in enumerate(images))
    counts = sorted({len(q) for (g, _, d), _ in images for q in g + d})
    print("vertex counts %s; largest error / tolerance %.3e" % (counts, worst))
    if batch == 0:
        assert {3, 4, 5, 36, 63, 64} <= set(counts)
        assert max(a for _, want in images for row in want['inter'] for a in row) > 100.0
    got = PolygonMeasurer().measure({'polygons': [im[0] for im, _ in images], 'ignore_tags': [im[1] for im, _ in images]},
                                    ([im[2] for im, _ in images],))
    for g, (im, want) in zip(got, images):
        for key in KEYS:
            assert g[key] == want[key], key
        assert len(g['gtPolPoints']) == sum(want['gt_valid']) and len(g['detPolPoints']) == sum(want['det_valid'])


def test_no_images_and_the_vertex_limit():
    assert PolygonMeasurer().measure({'polygons': [], 'ignore_tags': []}, ([],)) == []
    args, _, _, _ = _upload([], V=8, G=3, D=2)
    r = polygon_measure(*args).to_host()
    assert r['inter'].shape == (0, 3, 2) and r['counts'].shape == (0, 4)
    # V = 65 is refused with a message, not truncated: nothing is written
    image = ([P.L_SHAPE], [0], [P.COMB])
    args, G, D, _ = _upload([image], V=65)
    out = QuadOutputs(1, G, D, torch.device(DEV))
    out.packed.fill_(0xCD)
    with pytest.raises(RuntimeError, match="V=65.*exceed"):
        polygon_measure(*args, out=out)
    assert (out.to_host()['gt_valid'] == -842150451).all()
    with pytest.raises(ValueError, match="65 vertices exceeds the 64"):
        PolygonMeasurer().measure({'polygons': [[np.zeros((65, 2))]], 'ignore_tags': [[0]]}, ([[]],))
    # a count outside 3 .. V makes that polygon invalid, not the call
    args, G, D, _ = _upload([([P.L_SHAPE, P.COMB, [(0, 0), (4, 0)]], [0, 0, 0], [P.L_SHAPE])], V=8)
    r = polygon_measure(*args).to_host()
    assert r['gt_valid'][0].tolist() == [1, 0, 0] and r['counts'][0].tolist() == [1, 1, 1, 1]


@functools.lru_cache(maxsize=None)
def _quad_images():
    names = sorted(R.CASES)
    images = [R.CASES[name][:3] for name in names] + [im[:3] for im in R.parity_images()[0][:6]]
    return names, images


def test_quads_give_the_tables_of_mr_quad_iou_and_the_dicts_of_quad_measurer():
    names, images = _quad_images()
    args, G, D, V = _upload(images)
    assert V == 4
    got = polygon_measure(*args).to_host()
    quads = quad_measure(args[0], args[2], args[3], args[4], args[6]).to_host()
    for key in ('gt_valid', 'det_valid', 'gt_area', 'det_area', 'counts', 'scores', 'match_det', 'gt_dontcare', 'det_dontcare'):
        assert (got[key] == quads[key]).all(), key
    worst = 0.0
    for n, (gts, _, dets) in enumerate(images):
        for g, p in enumerate(gts):
            for d, q in enumerate(dets):
                if got['gt_valid'][n, g] and got['det_valid'][n, d]:
                    tol = P.area_tol(_floats(p), _floats(q))
                    union = quads['gt_area'][n, g] + quads['det_area'][n, d] - quads['inter'][n, g, d]
                    worst = max(worst, abs(got['inter'][n, g, d] - quads['inter'][n, g, d]) / tol,
                                abs(got['iou'][n, g, d] - quads['iou'][n, g, d]) / (4.0 * tol / union + 4.0 * P.EPS))
    print("largest difference between the two kernels / tolerance: %.3e" % worst)
    assert worst <= 1.0
    batch = {'polygons': [np.array(g, dtype=np.float64).reshape(-1, 4, 2) for g, _, _ in images],
             'ignore_tags': [list(i) for _, i, _ in images]}
    output = ([d for _, _, d in images],)
    as_polygons, as_quads = PolygonMeasurer().measure(batch, output), QuadMeasurer().measure(batch, output)
    for a, b in zip(as_polygons, as_quads):
        assert set(a) == set(b)
        for key in KEYS:
            assert a[key] == b[key], key
        assert np.array(a['iouMat']).shape == np.array(b['iouMat']).shape
        assert np.allclose(np.array(a['iouMat']), np.array(b['iouMat']), rtol=0, atol=1e-12)
        assert all((np.array(x) == np.array(y)).all() for key in ('gtPolPoints', 'detPolPoints') for x, y in zip(a[key], b[key]))
    for name, a in zip(names, as_polygons):
        for key, value in R.CASES[name][3].items():
            if key == 'iouMat':
                assert np.allclose(np.array(a[key]).reshape(-1), np.array(value).reshape(-1), rtol=0, atol=1e-12), name
            elif isinstance(value, float):
                assert abs(a[key] - value) <= 1e-15, (name, key)
            else:
                assert a[key] == value, (name, key)


def test_one_image_mixes_quads_outlines_and_ribbons():
    """A block of quads, a 14-point outline and a `Ribbon` as the ground truths of ONE image; the detections are the same three
    given the other way round (ribbon first), through `gather_measure` and with custom constraints."""
    rng = random.Random(9)
    quads = np.array([R.box(10.0, 10.0, 60.0, 30.0), R.box(100.0, 10.0, 160.0, 30.0)])
    outline = np.array(P.random_ribbon(rng, 300.0, 300.0, 90.0, 7))
    ribbon = Ribbon.from_polygon(P.random_ribbon(rng, 600.0, 300.0, 90.0, 18))
    batch = {'polygons': [[quads, outline, ribbon]], 'ignore_tags': [[0, 1, 0, 0]]}
    output = ([[ribbon, outline.tolist(), torch.from_numpy(quads)]],)
    m = PolygonMeasurer()
    raw, interested = m.validate_measure(batch, output)
    assert interested == [0] and len(raw) == 1
    got = raw[0]
    assert got['pairs'] == [{'gt': 0, 'det': 2}, {'gt': 2, 'det': 1}, {'gt': 3, 'det': 0}]
    assert got['gtDontCare'] == [1] and got['detDontCare'] == [3] and (got['gtCare'], got['detCare'], got['detMatched']) == (3, 3, 3)
    assert [len(p) for p in got['gtPolPoints']] == [4, 4, 14, 36] and [len(p) for p in got['detPolPoints']] == [36, 14, 4, 4]
    ones = np.zeros((4, 4))
    ones[[0, 1, 2, 3], [2, 3, 1, 0]] = 1.0
    assert np.allclose(np.array(got['iouMat']), ones, rtol=0, atol=1e-6)
    total = m.gather_measure([raw])
    assert total['precision'].val == 1.0 and total['recall'].val == 1.0
    assert PolygonMeasurer(iou_constraint=0.5, area_precision_constraint=0.5).measure(batch, output)[0]['hmean'] == 1.0


def test_end_to_end_a_curved_word_matches_as_a_ribbon_and_not_as_a_box():
    """The README's arch (R = 80, 14 px thick, 100 degrees) painted as the detector's map -> represent_ribbons -> outlines_of ->
    PolygonMeasurer.  The map of a DB detector is the SHRUNK word, which the representer grows again by d = 1.5 * area /
    perimeter (as in test_quad_measure_gpu's end-to-end test, whose ground truths are the painted rectangles grown by the same
    rule): the ground truth is the sector's own outline grown by the d of its own area and perimeter.  The ribbon's outline
    matches it (hmean 1); the same detection's box, measured against the same ground truth, does not: its IoU, taken from
    the restatement, is below 0.5 -- what the quad metric could not tell apart."""
    H, W, centre, radius, thick, span = 240, 320, (160.0, 150.0), 80.0, 14.0, 100.0
    prob = torch.from_numpy(RR.paint_sector(H, W, centre, radius, thick, span).astype(np.float32))[None, None].to(DEV)
    represented = SegDetectorRepresenter(box_thresh=0.2).represent_ribbons({'image': prob, 'shape': [(H, W)]}, {'binary': prob})
    boxes, _, ribbons = represented
    assert len(boxes[0]) == 1 and ribbons[0][0] is not None
    theta = math.radians(span)
    d = 1.5 * (thick * radius * theta) / (2.0 * radius * theta + 2.0 * thick)
    angles = [(theta + 2.0 * d / radius) * (k / 13.0 - 0.5) for k in range(14)]
    outer = [(centre[0] + (radius + thick / 2.0 + d) * math.sin(a), centre[1] - (radius + thick / 2.0 + d) * math.cos(a)) for a in angles]
    inner = [(centre[0] + (radius - thick / 2.0 - d) * math.sin(a), centre[1] - (radius - thick / 2.0 - d) * math.cos(a)) for a in angles]
    truth = outer + inner[::-1]                                                     # 28 points, CTW1500's order
    batch = {'polygons': [[np.array(truth)]], 'ignore_tags': [[0]]}
    outlines = outlines_of(represented)
    assert len(outlines[0]) == 1 and 10 <= len(outlines[0][0]) <= 36
    curved = PolygonMeasurer().measure(batch, (outlines,))[0]
    assert curved['hmean'] == 1.0 and curved['pairs'] == [{'gt': 0, 'det': 0}]
    box = _floats(boxes[0][0])
    a = P.poly_intersection(truth, box)
    box_iou = a / (P.poly_area(truth) + P.poly_area(box) - a)
    print("ribbon outline: IoU %.3f; the box: IoU %.3f" % (curved['iouMat'][0][0], box_iou))
    assert curved['iouMat'][0][0] > 0.8 and box_iou < 0.5 - P.MARGIN
    as_box = PolygonMeasurer().measure(batch, (boxes,))[0]
    assert as_box['hmean'] == 0.0 and as_box['pairs'] == [] and abs(as_box['iouMat'][0][0] - box_iou) <= 1e-9
