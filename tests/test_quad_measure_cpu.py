"""The checker of the detection-metric kernels is checked first: tests/_quad_eval_ref.py (the float64 restatement that
tests/test_quad_measure_gpu.py compares the device results with) against answers derived by hand -- the known cases of
`evaluate_image`, intersection areas of convex and concave quads -- and against point counting on a grid, which shares
no code with the triangle clipping.  Plus the host-side wiring that needs no GPU: the drop-in table, the export, the
refusal of CPU tensors, `gather_measure`."""
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _quad_eval_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MEGREADER_REFERENCE", "/root/reference")


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_helper_known_answers(name):
    gts, ignores, dets, want = R.CASES[name]
    got = R.evaluate_image(gts, ignores, dets)
    for key, value in want.items():
        if key == 'iouMat':
            assert np.allclose(np.array(got[key]).reshape(-1), np.array(value).reshape(-1), rtol=0, atol=1e-12), key
        elif isinstance(value, float):
            assert abs(got[key] - value) <= 1e-15, (key, got[key])
        else:
            assert got[key] == value, (key, got[key])


def test_helper_self_test_areas():
    gts, _, dets, _ = R.CASES['selftest']
    got = R.evaluate_image(gts, [0, 0], dets)
    assert abs(got['inter'][0][0] - 0.9) < 1e-15 and abs(got['det_area'][0] - 0.9) < 1e-15
    assert got['gt_area'] == [1.0, 1.0] and got['inter'][1][0] == 0.0


CHEVRON = [(0, 0), (2, 1), (4, 0), (2, 3)]             # concave: the triangle (0,0) (4,0) (2,3) less (0,0) (4,0) (2,1)
HAND_AREAS = [
    # 2 x 2 square against the diamond |x - 1| + |y - 1| <= 1.5: the square less four corner triangles with legs 0.5
    (R.box(0, 0, 2, 2), [(1, -0.5), (2.5, 1), (1, 2.5), (-0.5, 1)], 3.5),
    # the chevron below y = 1: trapezoid of the big triangle (4 and 8/3 wide) less the small triangle (area 2)
    (CHEVRON, R.box(0, 0, 4, 1), 10.0 / 3.0 - 2.0),
    # the chevron against itself, and against itself turned clockwise and started at another vertex
    (CHEVRON, CHEVRON, 4.0),
    (CHEVRON, [CHEVRON[2], CHEVRON[1], CHEVRON[0], CHEVRON[3]], 4.0),
    # two chevrons, the second moved up by 1 (concave against concave).  The big triangles overlap in the part of the
    # first above y = 1: apex (2,3), base from 2/3 to 10/3, area 8/3.  The first dent lies below y = 1.  The moved dent
    # (0,1) (4,1) (2,2) is cut by the first triangle's sides at y = 1.5: widths 4 - 4y/3 on [1, 1.5] and 8 - 4y on
    # [1.5, 2] integrate to 7/6 + 1/2 = 5/3.  8/3 - 5/3 = 1
    (CHEVRON, [(x, y + 1) for x, y in CHEVRON], 1.0),
    # containment and disjointness
    (R.box(0, 0, 10, 10), R.box(2, 3, 5, 7), 12.0),
    (R.box(0, 0, 1, 1), R.box(2, 2, 3, 3), 0.0),
    # a shared edge only: zero area
    (R.box(0, 0, 1, 1), R.box(1, 0, 2, 1), 0.0),
]


@pytest.mark.parametrize("k", range(len(HAND_AREAS)))
def test_helper_hand_computed_intersections(k):
    p, q, want = HAND_AREAS[k]
    p, q = [(float(x), float(y)) for x, y in p], [(float(x), float(y)) for x, y in q]
    assert R.quad_valid(p) and R.quad_valid(q)
    for a, b in ((p, q), (q, p), (p[::-1], q), (p[1:] + p[:1], q[3:] + q[:3])):
        assert abs(R.quad_intersection(a, b) - want) <= 1e-12, (a, b, R.quad_intersection(a, b))


def _grid_estimate(p, q, n=1000):
    """Area of p and q's intersection by counting the centres of an n x n grid over the common bounding box, and the
    hard bound of its error: a cell is miscounted only if an edge of p or q passes through it, and an edge of length l
    passes through at most 2 l / cell + 3 cells."""
    xs, ys = [v[0] for v in p + q], [v[1] for v in p + q]
    x0, y0 = min(xs), min(ys)
    cell = max(max(xs) - x0, max(ys) - y0) / n
    cx, cy = np.meshgrid(x0 + (np.arange(n) + 0.5) * cell, y0 + (np.arange(n) + 0.5) * cell)

    def inside(quad):
        res = np.zeros(cx.shape, dtype=bool)
        for k in range(4):
            (ax, ay), (bx, by) = quad[k], quad[(k + 1) % 4]
            if ay == by:
                continue
            res ^= ((ay > cy) != (by > cy)) & (cx < ax + (cy - ay) * (bx - ax) / (by - ay))
        return res
    count = int((inside(p) & inside(q)).sum())
    cells = sum(2.0 * math.hypot(a[0] - b[0], a[1] - b[1]) / cell + 3.0
                for quad in (p, q) for a, b in zip(quad, quad[1:] + quad[:1]))
    return count * cell * cell, cells * cell * cell


def test_helper_intersections_against_point_counting():
    """Concave against concave, concave against convex, both orientations: quads drawn over each other."""
    import random
    rng = random.Random(7)
    checked = 0
    for trial in range(24):
        p = R.random_quad(rng, 1000.0, 1000.0, 100.0, concave=trial % 4 != 3)
        q = R.random_quad(rng, 1000.0 + rng.uniform(-60, 60), 1000.0 + rng.uniform(-60, 60), rng.uniform(60, 140),
                          concave=trial % 2 == 0)
        exact = R.quad_intersection(p, q)
        estimate, bound = _grid_estimate(p, q)
        assert abs(exact - estimate) <= bound, (trial, p, q, exact, estimate, bound)
        assert bound < 600.0         # px^2; a split along the wrong diagonal is off by the dent, thousands of px^2 here
        checked += exact > 0.0
    assert checked >= 18


def test_helper_validity_rule():
    assert R.quad_valid(R.box(0, 0, 2, 1)) and R.quad_valid(R.box(0, 0, 2, 1)[::-1])
    assert R.quad_valid([(float(x), float(y)) for x, y in CHEVRON])
    assert not R.quad_valid([(0, 0), (4, 4), (4, 0), (0, 2)])             # bow-tie with a non-zero shoelace sum
    assert not R.quad_valid([(0, 0), (1, 1), (1, 0), (0, 1)])             # symmetric bow-tie: zero shoelace sum
    assert not R.quad_valid([(0, 0), (1, 1), (2, 2), (3, 3)])             # zero area
    assert not R.quad_valid([(0, 0), (4, 0), (2, 0), (2, 3)])             # vertex 2 on the edge 0-1: edges touch
    assert not R.quad_valid([(0, 0), (4, 0), (4, 3), (float('nan'), 1)])


def test_parity_images_keep_their_margin_within_the_redraw_cap():
    """The seeds of the GPU parity test: every image keeps |iou - 0.5| and |inter / det_area - 0.5| >= MARGIN after at
    most REDRAW_CAP of them were redrawn, and the images are not trivial."""
    images, redrawn, smallest = R.parity_images()
    print("redrawn %d of %d, smallest margin %.3e" % (redrawn, len(images), smallest))
    assert redrawn <= R.REDRAW_CAP * len(images) and smallest >= R.MARGIN
    quads = [q for gts, _, dets, _ in images for q in gts + dets]
    assert 300 <= len(quads) and all(R.quad_valid(q) and R.quad_area(q) >= 16.0 for q in quads)
    assert all(0.0 <= c <= 2048.0 for q in quads for v in q for c in v)
    turns = [[R.orient2(q[k], q[(k + 1) % 4], q[(k + 2) % 4]) for k in range(4)] for q in quads]
    concave = sum(min(t) < 0.0 < max(t) for t in turns)
    assert 0.2 * len(quads) <= concave <= 0.8 * len(quads)
    assert sum(w['detMatched'] for *_, w in images) >= 30 and sum(len(w['detDontCare']) for *_, w in images) >= 10
    assert sum(w['detMatched'] < min(w['gtCare'], w['detCare']) for *_, w in images) >= 10


def test_dropin_installs_the_quad_measurer():
    ref = REF if os.path.isdir(os.path.join(REF, "structure", "measurers")) else None
    code = '''
        import megreader_amd.dropin as dropin
        installed = dropin.install(%r)
        assert "QuadMeasurer" in installed["structure.measurers"], installed
        import structure.measurers
        import megreader_amd.structure
        from megreader_amd.structure.quad_measurer import QuadMeasurer
        assert structure.measurers.QuadMeasurer is QuadMeasurer is megreader_amd.structure.QuadMeasurer
        assert structure.measurers.SequenceRecognitionMeasurer is megreader_amd.structure.SequenceRecognitionMeasurer
        print("INSTALLED")
    ''' % ref
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "INSTALLED" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-2000:]


def test_cpu_tensors_are_refused():
    from megreader_amd.ops.detection_measure import quad_measure
    from megreader_amd.structure import QuadMeasurer
    gt, det = torch.zeros(1, 1, 4, 2, dtype=torch.float64), torch.zeros(1, 1, 4, 2, dtype=torch.float64)
    one = torch.ones(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        quad_measure(gt, one, torch.zeros(1, 1, dtype=torch.int32), det, one)
    with pytest.raises(NotImplementedError):
        QuadMeasurer().measure({'polygons': [[R.box(0, 0, 1, 1)]], 'ignore_tags': [[0]]}, ([[R.box(0, 0, 1, 1)]],),
                               device="cpu")


def test_gather_measure_combines_global_sums():
    """`combine_results` + quad_measurer.py:43-64: global sums, n = number of images, fmeasure with the 1e-8."""
    from megreader_amd.structure import QuadMeasurer
    raw = [[dict(gtCare=2, detCare=1, detMatched=1), dict(gtCare=0, detCare=3, detMatched=0)],
           [dict(gtCare=4, detCare=4, detMatched=3)]]
    m = QuadMeasurer().gather_measure(raw)
    assert m['precision'].val == 4 / 8 and m['recall'].val == 4 / 6 and m['precision'].count == 3 == m['recall'].count
    assert m['precision'].avg == 0.5 and m['fmeasure'].count == 1
    assert m['fmeasure'].val == 2 * 0.5 * (4 / 6) / (0.5 + 4 / 6 + 1e-8)
    empty = QuadMeasurer().gather_measure([[dict(gtCare=0, detCare=0, detMatched=0)]])
    assert empty['precision'].val == 0 and empty['recall'].val == 0 and empty['fmeasure'].val == 0


def test_host_side_of_the_measurer_without_a_gpu():
    """The packing of the outputs into one buffer (`QuadOutputs`, here on the CPU device and filled from the restatement
    instead of by the kernels), its single-copy `to_host()`, and the per-image dicts `QuadMeasurer` builds from it."""
    from megreader_amd.ops.detection_measure import QuadOutputs
    from megreader_amd.structure import QuadMeasurer
    names = ('invalid', 'dontcare', 'empty_both', 'selftest')
    images = [R.CASES[name][:3] for name in names]
    wants = [R.evaluate_image(*im) for im in images]
    G, D = 3, 3
    out = QuadOutputs(len(images), G, D, torch.device("cpu"))
    assert set(out) == {'gt_valid', 'det_valid', 'gt_area', 'det_area', 'inter', 'iou', 'counts', 'scores', 'match_det',
                        'gt_dontcare', 'det_dontcare'}
    assert out['inter'].dtype == torch.float64 and out['match_det'].dtype == torch.int32
    assert tuple(out['iou'].shape) == (4, G, D) and tuple(out['counts'].shape) == (4, 4)
    out.packed.zero_()
    out['match_det'].fill_(-1)
    for n, ((gts, _, dets), w) in enumerate(zip(images, wants)):
        ng, nd = len(gts), len(dets)
        out['gt_valid'][n, :ng] = torch.tensor(w['gt_valid'], dtype=torch.int32)
        out['det_valid'][n, :nd] = torch.tensor(w['det_valid'], dtype=torch.int32)
        if ng and nd:
            out['iou'][n, :ng, :nd] = torch.tensor(w['iou'], dtype=torch.float64)
        out['counts'][n] = torch.tensor([w['gtCare'], w['detCare'], w['detMatched'], sum(w['gt_valid'])])
        out['scores'][n] = torch.tensor([w['precision'], w['recall'], w['hmean']], dtype=torch.float64)
        for pair in w['pairs']:
            out['match_det'][n, pair['gt']] = pair['det']
        out['gt_dontcare'][n, w['gtDontCare']] = 1
        out['det_dontcare'][n, w['detDontCare']] = 1
    host = out.to_host()
    for key in out:
        assert host[key].shape == tuple(out[key].shape) and (host[key] == out[key].numpy()).all(), key
    as_arrays = [[np.array(q, dtype=np.float64).reshape(-1, 4, 2) for q in (im[0], im[2])] for im in images]
    got = QuadMeasurer.per_image_results(host, [a[0] for a in as_arrays], [a[1] for a in as_arrays])
    for g, name in zip(got, names):
        for key, value in R.CASES[name][3].items():
            if key == 'iouMat':
                assert np.allclose(np.array(g[key]).reshape(-1), np.array(value).reshape(-1), rtol=0, atol=1e-12), (name, key)
            elif isinstance(value, float):
                assert abs(g[key] - value) <= 1e-15, (name, key)
            else:
                assert g[key] == value, (name, key, g[key])
    assert [len(g['gtPolPoints']) for g in got] == [2, 2, 0, 2] and [len(g['detPolPoints']) for g in got] == [2, 3, 0, 1]
