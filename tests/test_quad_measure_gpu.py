"""Detection metrics on the GPU (csrc/quad_measure.hip: mr_quad_iou + mr_quad_match) through
megreader_amd.ops.detection_measure.quad_measure and megreader_amd.structure.QuadMeasurer, against the hand-derived
answers and the float64 restatement of tests/_quad_eval_ref.py (itself checked in tests/test_quad_measure_cpu.py).

Tolerance of the areas and IoUs, derived, not measured: an area is the sum of at most about 50 products and sums of
coordinates up to 2048, each rounded by at most 2^-52 * 2 * 2048^2 = 1.9e-9, so two correct float64 evaluations differ by
less than 1e-7 px^2; an IoU divides by a union of at least 16 px^2.  AREA_TOL = 1e-6 absolute covers both.  Counts, pairs
and flags must be equal: every image keeps its IoUs and covered fractions at least _quad_eval_ref.MARGIN = 1e-3 from 0.5."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _quad_eval_ref as R  # noqa: E402
from megreader_amd.ops.detection_measure import QuadOutputs, quad_measure  # noqa: E402
from megreader_amd.structure import QuadMeasurer, SegDetectorRepresenter  # noqa: E402
from megreader_amd.structure.db_geometry import unclip  # noqa: E402

DEV = "cuda"
AREA_TOL = 1e-6
KEYS = ('precision', 'recall', 'hmean', 'pairs', 'gtCare', 'detCare', 'detMatched', 'gtDontCare', 'detDontCare')


def _upload(images, G=None, D=None):
    """[(gts, ignores, dets)] -> the padded device arrays of quad_measure (+ G, D)."""
    N = len(images)
    G = max([1] + [len(g) for g, _, _ in images]) if G is None else G
    D = max([1] + [len(d) for _, _, d in images]) if D is None else D
    gt, det = np.zeros((N, G, 4, 2)), np.zeros((N, D, 4, 2))
    ignore = np.zeros((N, G), dtype=np.int32)
    for n, (gts, ignores, dets) in enumerate(images):
        if gts:
            gt[n, :len(gts)] = np.array(gts, dtype=np.float64)
            ignore[n, :len(gts)] = np.array(ignores) != 0
        if dets:
            det[n, :len(dets)] = np.array(dets, dtype=np.float64)
    counts = [np.array([len(im[k]) for im in images], dtype=np.int32) for k in (0, 2)]
    return [torch.from_numpy(a).to(DEV) for a in (gt, counts[0], ignore, det, counts[1])], G, D


def _check_image(r, n, image, want, G, D):
    """Every slot of every output of image n against the restatement's values; padding slots against the stated ones."""
    gts, _, dets = image
    ng_all, nd_all = len(gts), len(dets)
    worst = 0.0
    for key, width, used in (('gt_valid', G, ng_all), ('det_valid', D, nd_all)):
        expect = np.zeros(width, dtype=np.int32)
        expect[:used] = want[key]
        assert (r[key][n] == expect).all(), (n, key)
    for key, width, used in (('gt_area', G, ng_all), ('det_area', D, nd_all)):
        expect = np.zeros(width)
        expect[:used] = want[key]
        worst = max(worst, float(np.abs(r[key][n] - expect).max()))
        assert (r[key][n][used:] == 0.0).all(), (n, key)
    for key in ('inter', 'iou'):
        expect = np.zeros((G, D))
        if ng_all and nd_all:
            expect[:ng_all, :nd_all] = np.array(want[key])
        worst = max(worst, float(np.abs(r[key][n] - expect).max()))
        pad = np.ones((G, D), dtype=bool)
        pad[:ng_all, :nd_all] = False
        assert (r[key][n][pad] == 0.0).all(), (n, key)
    assert worst <= AREA_TOL, (n, worst)
    ng, nd = sum(want['gt_valid']), sum(want['det_valid'])
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


def _measure(images):
    """QuadMeasurer on a batch of (gts, ignores, dets) given the way a data loader and the representer give them."""
    batch = {'polygons': [np.array(g, dtype=np.float64).reshape(-1, 4, 2) for g, _, _ in images],
             'ignore_tags': [np.array(i, dtype=bool) for _, i, _ in images]}
    return QuadMeasurer().measure(batch, ([[[list(v) for v in q] for q in d] for _, _, d in images], None))


def _assert_case(got, want):
    for key, value in want.items():
        if key == 'iouMat':
            assert np.array(got[key]).shape == np.array(value).shape, key
            assert np.allclose(np.array(got[key]).reshape(-1), np.array(value).reshape(-1), rtol=0, atol=AREA_TOL), key
        elif isinstance(value, float):
            assert abs(got[key] - value) <= 1e-15, (key, got[key], value)
        else:
            assert got[key] == value, (key, got[key], value)


@pytest.mark.parametrize("name", ['selftest', 'greedy', 'dontcare', 'dontcare_blocks_match', 'invalid'])
def test_known_answers(name):
    gts, ignores, dets, want = R.CASES[name]
    got = _measure([(gts, ignores, dets)])
    assert len(got) == 1
    _assert_case(got[0], want)
    valid_g = [q for q in gts if R.quad_valid([(float(x), float(y)) for x, y in q])]
    assert len(got[0]['gtPolPoints']) == len(valid_g)
    assert all((np.array(a) == np.array(b, dtype=np.float64)).all() for a, b in zip(got[0]['gtPolPoints'], valid_g))


def test_self_test_of_the_reference_through_the_op_and_gather_measure():
    gts, ignores, dets, want = R.CASES['selftest']
    args, G, D = _upload([(gts, ignores, dets)])
    r = quad_measure(*args).to_host()
    assert abs(r['inter'][0, 0, 0] - 0.9) <= AREA_TOL and abs(r['iou'][0, 0, 0] - 0.9) <= AREA_TOL
    assert r['inter'][0, 1, 0] == 0.0 and abs(r['det_area'][0, 0] - 0.9) <= AREA_TOL
    assert r['scores'][0].tolist() == [1.0, 0.5, 2.0 / 3.0] and r['match_det'][0].tolist() == [0, -1]
    m = QuadMeasurer()
    raw, interested = m.validate_measure(*_batch_of([(gts, ignores, dets)]))
    assert interested == [0]
    total = m.gather_measure([raw])
    assert total['precision'].val == 1.0 and total['recall'].val == 0.5
    assert abs(total['fmeasure'].val - 2.0 / 3.0) < 1e-7                   # 2PR / (P + R + 1e-8)
    raw2, vis = m.evaluate_measure(dict(_batch_of([(gts, ignores, dets)])[0], image=torch.empty(1, 3, 8, 8)),
                                   _batch_of([(gts, ignores, dets)])[1])
    assert raw2[0]['pairs'] == want['pairs'] and vis == np.linspace(0, 1).tolist()


def _batch_of(images):
    return ({'polygons': [np.array(g, dtype=np.float64).reshape(-1, 4, 2) for g, _, _ in images],
             'ignore_tags': [list(i) for _, i, _ in images]}, ([d for _, _, d in images],))


def test_strict_comparisons_and_custom_constraints():
    """Both constraints are parameters; `greedy` has IoUs 8/11, 7/10, 7/12, 3/14."""
    gts, ignores, dets, _ = R.CASES['greedy']
    args, _, _ = _upload([(gts, ignores, dets)])
    assert quad_measure(*args, iou_constraint=0.75).to_host()['counts'][0].tolist() == [2, 2, 0, 2]
    r = quad_measure(*args, iou_constraint=0.2).to_host()            # now gt1 takes det1 (3/14 > 0.2)
    assert r['match_det'][0].tolist() == [0, 1] and r['scores'][0].tolist() == [1.0, 1.0, 1.0]
    gts, ignores, dets, _ = R.CASES['dontcare']
    args, _, _ = _upload([(gts, ignores, dets)])
    r = quad_measure(*args, area_precision_constraint=0.3).to_host()  # det1 (40 % inside gt0) is don't-care too
    assert r['det_dontcare'][0].tolist() == [1, 1, 0] and r['counts'][0].tolist() == [1, 1, 1, 2]
    r = quad_measure(*args, area_precision_constraint=0.9).to_host()  # nothing is
    assert r['det_dontcare'][0].tolist() == [0, 0, 0] and r['counts'][0].tolist() == [1, 3, 1, 2]


def test_empty_cases_in_one_batch():
    images = [R.CASES[name][:3] for name in R.EMPTY_BATCH]
    got = _measure(images)
    for g, name in zip(got, R.EMPTY_BATCH):
        _assert_case(g, R.CASES[name][3])
    assert [(g['precision'], g['recall'], g['hmean']) for g in got] == [(1.0, 1.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)]
    assert QuadMeasurer().measure({'polygons': [], 'ignore_tags': []}, ([],)) == []


def test_orientation_and_vertex_rotation_change_nothing():
    rng_images, _, _ = _parity()
    base = [(g, i, d) for g, i, d, _ in rng_images[:4]] + [R.CASES['dontcare'][:3], R.CASES['selftest'][:3]]

    def variants(q, k):
        q = [tuple(v) for v in q]
        return [q[::-1], q[1:] + q[:1], q[3:] + q[:3], (q[2:] + q[:2])[::-1]][k]
    images = list(base)
    for k in range(4):
        images += [([variants(q, k) for q in g], i, d) for g, i, d in base]
        images += [(g, i, [variants(q, (k + 1) % 4) for q in d]) for g, i, d in base]
    args, G, D = _upload(images)
    r = quad_measure(*args).to_host()
    worst = 0.0
    for v in range(1, 9):
        for b in range(len(base)):
            n = v * len(base) + b
            for key in ('gt_area', 'det_area', 'inter', 'iou'):
                worst = max(worst, float(np.abs(r[key][n] - r[key][b]).max()))
            for key in ('gt_valid', 'det_valid', 'counts', 'scores', 'match_det', 'gt_dontcare', 'det_dontcare'):
                assert (r[key][n] == r[key][b]).all(), (v, b, key)
    print("largest change of an area or IoU under reversal / rotation: %.3e" % worst)
    assert worst <= AREA_TOL


def _padding_images():
    """(G_i, D_i) = (1, 130), (70, 3), (0, 0): the decisions sit beyond the first 64 detections / ground truths."""
    def cell(k, size=8.0):
        return R.box(20.0 * (k % 50), 100.0 + 20.0 * (k // 50), 20.0 * (k % 50) + size, 100.0 + 20.0 * (k // 50) + size)
    # image 0: the gt is matched by detection 129 only; 64, 65 and 128 overlap it too little; 3 is invalid
    gt0 = R.box(500.0, 0.0, 540.0, 20.0)
    dets0 = [cell(k) for k in range(130)]
    dets0[3] = [(0.0, 0.0), (5.0, 5.0), (5.0, 0.0), (0.0, 5.0)]
    dets0[64] = R.box(500.0, 0.0, 515.0, 20.0)
    dets0[65] = R.box(530.0, 0.0, 580.0, 20.0)
    dets0[128] = R.box(490.0, 0.0, 519.0, 20.0)
    dets0[129] = R.box(502.0, 1.0, 540.0, 20.0)
    # image 1: 70 gts; 66 is ignored and swallows det 1; 5 is invalid; det 2 matches gt 69, det 0 matches gt 64
    gts1 = [cell(k, 10.0) for k in range(70)]
    gts1[5] = [(0.0, 0.0), (5.0, 5.0), (10.0, 10.0), (0.0, 0.0)]
    ignores1 = [0] * 70
    ignores1[66] = 1
    ignores1[2] = 1
    x66, y66 = gts1[66][0]
    x69, y69 = gts1[69][0]
    x64, y64 = gts1[64][0]
    dets1 = [R.box(x64, y64, x64 + 10.0, y64 + 9.0), R.box(x66 + 1.0, y66 + 1.0, x66 + 9.0, y66 + 12.0),
             R.box(x69 + 1.0, y69, x69 + 10.0, y69 + 10.0)]
    return [([gt0], [0], dets0), (gts1, ignores1, dets1), ([], [], [])]


def test_padding_and_sizes_every_slot_is_written():
    images = _padding_images()
    args, G, D = _upload(images)
    assert (G, D) == (70, 130)
    out = QuadOutputs(3, G, D, torch.device(DEV))
    out.packed.fill_(0xCD)                                    # i32 -842150451, f64 -6.3e66
    assert quad_measure(*args, out=out) is out
    r = out.to_host()
    wants = [R.evaluate_image(*im) for im in images]
    for n, (im, want) in enumerate(zip(images, wants)):
        _check_image(r, n, im, want, G, D)
    assert wants[0]['pairs'] == [{'gt': 0, 'det': 128}] and wants[0]['det_valid'][3] is False     # 129 compacted
    assert wants[1]['pairs'] == [{'gt': 63, 'det': 0}, {'gt': 68, 'det': 2}]                      # 64, 69 compacted
    assert wants[1]['gtDontCare'] == [2, 65] and wants[1]['detDontCare'] == [1]
    assert r['counts'].tolist() == [[1, 129, 1, 1], [67, 2, 2, 69], [0, 0, 0, 0]]
    assert r['scores'][2].tolist() == [1.0, 1.0, 1.0]


def test_limits_are_refused_not_truncated():
    """256 x 256 works; beyond the 1024 quads per image the matching kernel holds, the call fails with a message."""
    gts = [R.box(8.0 * k, 0.0, 8.0 * k + 6.0, 6.0) for k in range(256)]
    dets = [R.box(8.0 * k + 1.0, 0.0, 8.0 * k + 6.0, 6.0) for k in reversed(range(256))]
    args, G, D = _upload([(gts, [0] * 256, dets)])
    r = quad_measure(*args).to_host()
    assert r['counts'][0].tolist() == [256, 256, 256, 256] and r['match_det'][0].tolist() == list(reversed(range(256)))
    args, _, _ = _upload([([], [], [])], G=1, D=1025)
    with pytest.raises(RuntimeError, match="1025.*exceed"):
        quad_measure(*args)


@functools.lru_cache(maxsize=None)
def _parity():
    return R.parity_images()


def test_random_parity_with_the_restatement():
    images, redrawn, smallest = _parity()
    print("redrawn %d of %d images, smallest margin %.3e" % (redrawn, len(images), smallest))
    assert redrawn <= R.REDRAW_CAP * len(images) and smallest >= R.MARGIN
    assert sum(len(g) + len(d) for g, _, d, _ in images) >= 300
    args, G, D = _upload([im[:3] for im in images])
    r = quad_measure(*args).to_host()
    worst = max(_check_image(r, n, im[:3], im[3], G, D) for n, im in enumerate(images))
    print("largest |difference| of an area or IoU: %.3e (bar %.0e)" % (worst, AREA_TOL))
    got = _measure([im[:3] for im in images])
    for g, im in zip(got, images):
        for key in KEYS:
            assert g[key] == im[3][key], key
        assert np.allclose(np.array(g['iouMat']), np.array(im[3]['iouMat']), rtol=0, atol=AREA_TOL)


def test_more_than_100_detections_drop_the_iou_matrix():
    images = _padding_images()
    got = _measure(images)
    assert got[0]['iouMat'] == [] and len(got[0]['detPolPoints']) == 129              # 129 valid detections > 100
    assert np.array(got[1]['iouMat']).shape == (69, 3) and got[2]['iouMat'] == []
    assert got[1]['pairs'] == [{'gt': 63, 'det': 0}, {'gt': 68, 'det': 2}]


def test_end_to_end_representer_to_measurer():
    """Three filled rectangles -> SegDetectorRepresenter -> QuadMeasurer against two of them grown by the representer's
    unclip, and one ground truth where nothing was detected: 2 of 3 detections and 2 of 3 ground truths match."""
    rects = [(20, 20, 60, 40), (80, 70, 104, 82), (20, 90, 60, 110)]              # x0, y0, x1, y1, inclusive pixels
    prob = torch.zeros(1, 1, 128, 128)
    for x0, y0, x1, y1 in rects:
        prob[0, 0, y0:y1 + 1, x0:x1 + 1] = 1.0
    prob = prob.to(DEV)
    boxes, _ = SegDetectorRepresenter().represent({'image': prob, 'shape': [(128, 128)]}, {'binary': prob})
    assert len(boxes) == 1 and len(boxes[0]) == 3
    grown = [unclip([[x0, y0], [x1, y0], [x1, y1], [x0, y1]]) for x0, y0, x1, y1 in rects[:2]]
    gts = np.array(grown + [R.box(90.0, 5.0, 120.0, 25.0)], dtype=np.float64)
    got = QuadMeasurer().measure({'polygons': torch.from_numpy(gts)[None], 'ignore_tags': torch.zeros(1, 3)}, (boxes, None))
    assert got[0]['detMatched'] == 2 and got[0]['gtCare'] == 3 and got[0]['detCare'] == 3
    assert abs(got[0]['precision'] - 2.0 / 3.0) < 1e-15 and abs(got[0]['recall'] - 2.0 / 3.0) < 1e-15
    assert sorted(p['gt'] for p in got[0]['pairs']) == [0, 1]
    assert all(got[0]['iouMat'][p['gt']][p['det']] > 0.9 for p in got[0]['pairs'])
