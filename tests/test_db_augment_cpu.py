"""The augmentation plan (megreader_amd/data/detection_augment.py) on the host: the stage algebra against hand values, the
`crop_area` restatement's properties, the window property (no tap inside the image lies outside the uploaded window) and
the consistency of the pixel map with the point map, through the numpy restatement of the kernel (tests/_db_augment_ref.py)."""
import ctypes
import math

import numpy as np
import pytest

import _db_augment_ref as R
from megreader_amd.data import AugmentPlan, DetectionAugmenter, WarpDesc
from megreader_amd.data.detection_augment import apply_points, crop_area, is_poly_outside_rect


def src_of(plan, u, v):
    a = plan.pixels_inv
    return a[0] * u + a[1] * v + a[2], a[3] * u + a[4] * v + a[5]


# ---- plan algebra ------------------------------------------------------------------------------------------------------------

def test_flip_sends_the_first_column_to_the_last():
    H, W = 48, 80
    plan = DetectionAugmenter(size=(W, H)).plan((H, W), flip=True)
    np.testing.assert_array_equal(apply_points(plan.points, [[0.0, 7.0], [W - 1.0, 7.0], [30.0, 0.0]]),
                                  [[W - 1.0, 7.0], [0.0, 7.0], [W - 31.0, 0.0]])
    assert src_of(plan, 0.0, 7.0) == (W - 1.0, 7.0) and src_of(plan, W - 1.0, 3.0) == (0.0, 3.0)    # pixels: the same map


def test_rotation_fixes_the_centre_and_plus_ten_degrees_moves_the_right_point_down():
    H, W = 48, 80
    cx, cy = (W - 1) / 2, (H - 1) / 2
    plan = DetectionAugmenter(size=(W, H)).plan((H, W), angle=10.0)
    np.testing.assert_allclose(apply_points(plan.points, [[cx, cy]]), [[cx, cy]], atol=1e-12)
    np.testing.assert_allclose(src_of(plan, cx, cy), (cx, cy), atol=1e-12)
    right = apply_points(plan.points, [[W - 1.0, cy]])[0]
    dx = W - 1 - cx
    np.testing.assert_allclose(right, [cx + math.cos(math.radians(10)) * dx, cy + math.sin(math.radians(10)) * dx], atol=1e-12)
    assert right[1] > cy + 6.8                            # sin(10 deg) * 39.5 = 6.86 rows DOWN
    np.testing.assert_allclose(src_of(plan, right[0], right[1]), (W - 1.0, cy), atol=1e-12)   # pixels follow the same map


def test_resize_and_crop_stages_on_a_worked_example():
    """Source 40 x 80 (rows x columns) at scale 2 -> 80 x 160; crop (x, y, w, h) = (40, 20, 80, 40) onto a 40 x 40 canvas:
    scale = min(40 / 80, 40 / 40) = 0.5, valid (w, h) = (40, 20).
    Points: (30, 20) -> x2 -> (60, 40) -> minus (40, 20), x0.5 -> (10, 10).
    Pixels: u = 10 -> x_c = 10.5 * 80 / 40 - 0.5 = 20.5 -> resized 60.5 -> source 61 * 80 / 160 - 0.5 = 30;
            v = 10 -> y_c = 10.5 * 40 / 20 - 0.5 = 20.5 -> resized 40.5 -> source 41 * 40 / 80 - 0.5 = 20.
    Clamp: x_c in [0, 79] <=> u in [0.5 * 40 / 80 - 0.5, 79.5 * 40 / 80 - 0.5] = [-0.25, 39.25]; y_c in [0, 39] <=> v in
    [0.5 * 20 / 40 - 0.5, 39.5 * 20 / 40 - 0.5] = [-0.25, 19.25]."""
    plan = DetectionAugmenter(size=(40, 40)).plan((40, 80), scale=2.0, crop=(40, 20, 80, 40))
    assert plan.resized == (80, 160) and plan.valid == (40, 20) and plan.canvas == (40, 40)
    np.testing.assert_array_equal(apply_points(plan.points, [[30.0, 20.0]]), [[10.0, 10.0]])
    np.testing.assert_array_equal(plan.points, [[1.0, 0.0, -20.0], [0.0, 1.0, -10.0], [0.0, 0.0, 1.0]])
    assert src_of(plan, 10.0, 10.0) == (30.0, 20.0)
    np.testing.assert_array_equal(plan.pixels_inv, [1.0, 0.0, 20.0, 0.0, 1.0, 10.0])
    assert plan.clamp == (-0.25, 39.25, -0.25, 19.25)
    # an enlarging crop: 20 x 20 at (5, 5) of a 40 x 40 source onto 40 x 40: x_c = (u + 0.5) / 2 - 0.5, clamp [0.5, 38.5]
    up = DetectionAugmenter(size=(40, 40)).plan((40, 40), crop=(5, 5, 20, 20))
    assert up.valid == (40, 40) and up.clamp == (0.5, 38.5, 0.5, 38.5)
    np.testing.assert_array_equal(up.pixels_inv, [0.5, 0.0, 4.75, 0.0, 0.5, 4.75])
    assert src_of(up, 0.5, 38.5) == (5.0, 24.0)           # the clamp bounds are the crop's first and last pixel


def test_resize_rounds_the_size_and_keeps_one_pixel():
    _, _, size = DetectionAugmenter.stages((48, 80), False, 0.0, 1.7)
    assert size == (82, 136)                              # round(81.6), round(136.0)
    assert DetectionAugmenter.stages((1, 1), False, 0.0, 0.5)[2] == (1, 1)


def test_identity_plan():
    H, W = 64, 96
    plan = DetectionAugmenter(size=(W, H)).plan((H, W))
    np.testing.assert_array_equal(plan.points, np.eye(3))
    np.testing.assert_array_equal(plan.pixels_inv, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    assert plan.valid == (W, H) and plan.window == (0, 0, W, H) and plan.clamp == (0.0, W - 1.0, 0.0, H - 1.0)


def test_resize_to_validation_plan():
    quad = [[[100.0, 50.0], [300.0, 50.0], [300.0, 90.0], [100.0, 90.0]]]
    plan = DetectionAugmenter.resize_to(1024, 576, (720, 1280), quad, [True])
    assert isinstance(plan, AugmentPlan)
    assert plan.canvas == (576, 1024) and plan.valid == (1024, 576) and plan.clamp == (0.0, 1023.0, 0.0, 575.0)
    np.testing.assert_array_equal(plan.pixels_inv, [1.25, 0.0, 0.125, 0.0, 1.25, 0.125])       # (u + 0.5) * 1.25 - 0.5
    np.testing.assert_array_equal(plan.polygons, np.array(quad) * 0.8)
    assert plan.ignore_tags.tolist() == [True] and plan.window == (0, 0, 1280, 720)


def test_descriptor_mirror():
    plan = DetectionAugmenter(size=(40, 40)).plan((40, 80), scale=2.0, crop=(40, 20, 80, 40))
    d = plan.fill(WarpDesc(), 4096)
    assert ctypes.sizeof(WarpDesc) == 128
    assert (d.offset, d.src_h, d.src_w, d.dst_h, d.dst_w) == (4096, 40, 80, 20, 40)
    assert (d.win_x, d.win_y, d.win_w, d.win_h) == plan.window and d.pitch == 3 * plan.window[2]
    assert list(d.a) == [1.0, 0.0, 20.0, 0.0, 1.0, 10.0] and (d.cu0, d.cu1, d.cv0, d.cv1) == plan.clamp


# ---- the window ------------------------------------------------------------------------------------------------------------

def _relative_quads(H, W):
    q = np.array([[[0.2, 0.2], [0.6, 0.25], [0.55, 0.5], [0.15, 0.45]], [[0.5, 0.6], [0.9, 0.6], [0.9, 0.9], [0.5, 0.9]]])
    return q * (W, H), [False, True]


@pytest.mark.parametrize("shape", [(37, 53), (48, 80), (1, 1), (2, 2)])
def test_no_tap_inside_the_image_lies_outside_the_window(shape):
    rng = np.random.RandomState(shape[0])
    src = rng.randint(0, 256, shape + (3,)).astype(np.uint8)
    quads, tags = _relative_quads(*shape)
    plans = []
    for size in ((96, 64), (7, 5)):
        aug = DetectionAugmenter(size=size, seed=100 + shape[1])
        plans += [aug.sample(shape, quads, tags) for _ in range(12)]
        plans += R.case_plans(shape, (size[1], size[0]), quads, tags)
        plans.append(DetectionAugmenter.resize_to(size[0], size[1], shape))
    for plan in plans:
        full = R.warp_normalize_ref(src, plan, window=(0, 0, shape[1], shape[0]))
        x, y, w, h = plan.window
        assert 0 <= x and 0 <= y and x + w <= shape[1] and y + h <= shape[0]
        t = full['taps']
        assert ((t[:, 0] >= x) & (t[:, 0] < x + w) & (t[:, 1] >= y) & (t[:, 1] < y + h)).all(), plan.__dict__
        np.testing.assert_array_equal(R.warp_normalize_ref(src, plan)['image'], full['image'])


def test_the_window_is_smaller_than_the_photo_for_a_crop():
    plan = DetectionAugmenter(size=(640, 640)).plan((720, 1280), angle=5.0, scale=3.0, crop=(1000, 700, 640, 640))
    x, y, w, h = plan.window
    assert w * h < 0.1 * 720 * 1280                      # 640 / 3 = 214 source pixels a side, plus the rotation's slant


# ---- the crop restatement ------------------------------------------------------------------------------------------------

def test_same_seed_same_plan():
    quads, tags = _relative_quads(480, 640)
    a = DetectionAugmenter(seed=7)
    b = DetectionAugmenter(seed=7)
    c = DetectionAugmenter(seed=8)
    seen = set()
    for _ in range(5):
        pa, pb, pc = (g.sample((480, 640, 3), quads, tags) for g in (a, b, c))
        assert (pa.flip, pa.angle, pa.scale, pa.crop, pa.window) == (pb.flip, pb.angle, pb.scale, pb.crop, pb.window)
        np.testing.assert_array_equal(pa.pixels_inv, pb.pixels_inv)
        np.testing.assert_array_equal(pa.polygons, pb.polygons)
        assert -10 <= pa.angle <= 10 and 0.5 <= pa.scale <= 3.0
        seen.add((pa.angle, pa.scale) == (pc.angle, pc.scale))
    assert seen == {False}


def _extents(polys):
    r = np.round(np.asarray(polys)).astype(np.int64)
    return r[..., 0].min(1), r[..., 0].max(1), r[..., 1].min(1), r[..., 1].max(1)


def test_crop_edges_do_not_cut_cared_for_polygons():
    """`crop_area` draws xmin and ymin from the columns and rows no cared-for polygon's rounded extent [min, max) covers, so
    the rectangle's left and top edge never cut one.  With a target size the right and bottom edge are xmin + width and
    ymin + width clipped to the image -- wherever that falls, as in the reference; without one (the fallback recursion) they
    are drawn from the free columns and rows as well, and then no edge cuts a polygon."""
    H, W = 200, 300
    polys = np.array([[[40, 30], [120, 34], [118, 60], [38, 56]], [[150, 100], [260, 100], [260, 140], [150, 140]],
                      [[20, 150], [90, 150], [90, 190], [20, 190]]], dtype=np.float64)
    minx, maxx, miny, maxy = _extents(polys)
    hits = sized = 0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        x, y, w, h = crop_area(rng, (H, W), polys, 64, 64)
        assert 0 <= x and 0 <= y and x + w <= W - 1 and y + h <= H - 1 and w >= 0.1 * W and h >= 0.1 * H
        assert not ((minx <= x) & (x < maxx)).any() and not ((miny <= y) & (y < maxy)).any()
        assert any(not is_poly_outside_rect(p, x, y, w, h) for p in polys)
        if (w, h) == (min(x + 64, W - 1) - x, min(y + 64, H - 1) - y):          # `width` sizes the height as well
            sized += 1
        else:                                                                     # every sized try failed: the fallback
            for e, lo, hi in ((x + w, minx, maxx), (y + h, miny, maxy)):
                assert not ((lo <= e) & (e < hi)).any()
        x, y, w, h = crop_area(rng, (H, W), polys)                               # no target size: both edges are free
        if (x, y, w, h) != (0, 0, W, H):
            hits += 1
            for e, lo, hi in ((x, minx, maxx), (x + w, minx, maxx), (y, miny, maxy), (y + h, miny, maxy)):
                assert not ((lo <= e) & (e < hi)).any()
    assert hits > 100 and sized > 100


def test_crop_falls_back_to_the_whole_image():
    H, W = 60, 90
    rng = np.random.default_rng(0)
    state = rng.bit_generator.state
    covered = [np.array([[0, 10], [W, 10], [W, 30], [0, 30]], dtype=np.float64)]     # every column is covered
    assert crop_area(rng, (H, W), covered, 64, 64) == (0, 0, W, H)
    assert rng.bit_generator.state == state                                           # decided before any draw
    assert crop_area(rng, (H, W), [], 64, 64) == (0, 0, W, H)                         # no polygon: every try fails
    # a negative coordinate slices from the end, as numpy does for the reference: [-3:20] of 90 columns is empty
    assert crop_area(np.random.default_rng(1), (H, W), [np.array([[-3, 5], [20, 5], [20, 50], [-3, 50]], dtype=np.float64)],
                     None, None, max_tries=50)[0] in range(0, W)


def test_polygons_outside_the_crop_are_dropped_and_tags_follow():
    quads = np.array([[[10, 10], [30, 10], [30, 20], [10, 20]],           # left of the crop: dropped
                      [[50, 12], [70, 12], [70, 22], [50, 22]],           # inside, ignored
                      [[75, 30], [95, 30], [95, 38], [75, 38]],           # straddles the right edge: kept
                      [[50, 45], [60, 45], [60, 47], [50, 47]]], dtype=np.float64)   # below: dropped
    plan = DetectionAugmenter(size=(80, 60)).plan((48, 100), quads, [False, True, False, True], crop=(40, 5, 40, 30))
    assert plan.valid == (80, 60) and plan.kept.tolist() == [1, 2]
    assert plan.ignore_tags.tolist() == [True, False]
    np.testing.assert_array_equal(plan.polygons, (quads[[1, 2]] - (40, 5)) * 2.0)
    with pytest.raises(ValueError):
        DetectionAugmenter().plan((48, 100), quads, [False])


# ---- image / label consistency -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(7))
def test_warped_image_agrees_with_the_transformed_quad(k):
    """A 48 x 80 source, white inside the quad (18,12) (62,15) (60,36) (16,33), onto a 64 x 96 canvas: `warped > 127.5` equals
    "inside the transformed quad" at every valid pixel farther than 2 px from the transformed boundary, and that band holds
    at most 25 % of the valid pixels (both are conditions: a float64 prototype of these plans disagreed no farther than
    1.11 px from the boundary, and a 2.5 px band held at most 19 % of the valid pixels)."""
    plan = R.case_plans()[k]
    out = R.warp_normalize_ref(R.quad_mask_image(), plan)
    Hd, Wd = R.CASE_CANVAS
    vv, uu = np.mgrid[0:Hd, 0:Wd].astype(np.float64)
    inside, dist = R.inside_and_distance(R.transformed_quad(plan), uu, vv)
    valid = out['valid']
    assert valid.sum() == plan.valid[0] * plan.valid[1] > 0
    far = valid & (dist > 2.0)
    band = int((valid & ~far).sum())
    white = out['value'][..., 0] > 127.5
    wrong = far & (white != inside)
    print("plan %d: valid %d, band %d (%.1f %%), farthest disagreement %.2f px" % (
        k, valid.sum(), band, 100.0 * band / valid.sum(), float(dist[valid & (white != inside)].max(initial=0.0))))
    assert not wrong.any()
    assert band <= 0.25 * valid.sum()
    assert inside[far].any() and (~inside[far]).any()      # both sides are tested
