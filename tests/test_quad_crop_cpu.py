"""The quad-crop planner (megreader_amd/data/quad_crop.py) and the numpy restatement of its kernel (tests/_quad_crop_ref.py) on
the host: the corner rule, the plan of an axis-aligned box, corner correspondence with and without `ensure_horizontal`'s
rotation, the 'pad' widths, and a closed form -- on a photo that is linear in (x, y) bilinear sampling is exact, so planner and
restatement are checked against the analytic value at the mapped point, which is neither of them."""
import math

import numpy as np
import pytest

import _quad_crop_ref as R
from megreader_amd.data.device_pipeline import target_width
from megreader_amd.data.quad_crop import crop_frame, plan_crop, rect_corners, top_edge_rule

ANGLES = (-80, -50, -44, -10, 0, 10, 44, 50, 80)


def rotated_box(a, b, angle, centre=(100.0, 80.0)):
    """The a x b rectangle (a along x before the rotation) turned by `angle` degrees about its centre: [4, 2]."""
    t = math.radians(angle)
    c, s = math.cos(t), math.sin(t)
    base = np.array([[-a / 2, -b / 2], [a / 2, -b / 2], [a / 2, b / 2], [-a / 2, b / 2]], dtype=np.float64)
    return base @ np.array([[c, s], [-s, c]]) + np.asarray(centre, dtype=np.float64)


def apply(h9, pts):
    m = np.asarray(h9, dtype=np.float64).reshape(3, 3)
    p = np.concatenate([np.asarray(pts, dtype=np.float64), np.ones((len(pts), 1))], axis=1) @ m.T
    return p[:, :2] / p[:, 2:]


def frame_corners(plan):
    """The (rotated) frame's points that are the crop frame's corners (0, 0), (w, 0), (w, h), (0, h)."""
    c = np.array([[0.0, 0.0], [plan.w, 0.0], [plan.w, plan.h], [0.0, plan.h]])
    if plan.rotated:                                    # (xc, yc) = (cw - 1 - yr, xr)  <=>  (xr, yr) = (yc, cw - 1 - xc)
        c = np.stack([c[:, 1], plan.cw - 1 - c[:, 0]], axis=1)
    return c


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("sides", [(40, 12), (12, 40)])
def test_corner_rule(sides, angle):
    box = rotated_box(sides[0], sides[1], angle)
    for pts in (box, box[::-1], np.roll(box, 2, axis=0)):                  # whatever order the points come in
        p = rect_corners(pts)
        e = np.roll(p, -1, axis=0) - p
        cross = e[:, 0] * np.roll(e[:, 1], -1) - e[:, 1] * np.roll(e[:, 0], -1)
        assert (cross > 0).all(), "corners do not run clockwise on screen"
        assert top_edge_rule(e[0])
        assert sum(top_edge_rule(d) for d in e) == 1
        assert sorted(map(tuple, np.round(p, 9))) == sorted(map(tuple, np.round(box, 9)))
        _, w, h = crop_frame(pts)
        # the side along edge 0 -> 1: the rectangle's side whose direction lies within [-45, 45) degrees of the x axis
        along = sides[0] if -45 <= angle < 45 else sides[1]
        assert abs(w - along) < 1e-9 and abs(h - (sides[0] + sides[1] - along)) < 1e-9


def test_axis_aligned_integer_box_is_a_translation():
    plan = plan_crop((60, 60), [[10, 5], [50, 5], [50, 20], [10, 20]], (15, 40))
    assert (plan.cw, plan.ch, plan.rotated, plan.dst_w) == (40, 15, False, 40)
    assert plan.h9.tolist() == [1.0, 0.0, 10.0, 0.0, 1.0, 5.0, 0.0, 0.0, 1.0]
    assert (plan.sx, plan.sy, plan.cu1, plan.cv1) == (1.0, 1.0, 39.0, 14.0)
    x, y, D, valid = R.source_points(plan)
    assert (D == 1.0).all() and valid.all()
    assert (x == np.arange(10, 50)[None, :]).all() and (y == np.arange(5, 20)[:, None]).all()


@pytest.mark.parametrize("rectify", ["min_area_rect", "quad"])
@pytest.mark.parametrize("sides,angle", [((40, 12), 0), ((40, 12), 30), ((40, 12), -44), ((12, 40), 10), ((40, 12), 80),
                                         ((12, 40), 0)])
def test_corner_correspondence(sides, angle, rectify):
    box = rotated_box(sides[0], sides[1], angle)
    plan = plan_crop((200, 200), box, (32, 128), rectify=rectify)
    assert plan.rotated == (plan.ch > 1.5 * plan.cw)
    assert np.abs(apply(plan.h9, frame_corners(plan)) - plan.corners).max() < 1e-9
    assert np.abs(apply(plan.crop_map, [[0, 0], [plan.w, 0], [plan.w, plan.h], [0, plan.h]]) - plan.corners).max() < 1e-9
    assert plan.frame == ((plan.cw, plan.ch) if plan.rotated else (plan.ch, plan.cw))
    assert (plan.cu1, plan.cv1) == (plan.frame[1] - 1, plan.frame[0] - 1)


def test_rotation_is_the_reference_flip():
    """R = np.flip(np.swapaxes(crop, 0, 1), 0): R[i][j] = crop[j][cw - 1 - i].  With a crop frame that is an integer slice of
    the photo, the rotated frame's pixel (xr, yr) = (j, i) must map onto the photo pixel of crop[j][cw - 1 - i]."""
    plan = plan_crop((80, 60), [[10, 5], [22, 5], [22, 45], [10, 45]], (12, 40))       # 12 wide, 40 high
    assert plan.rotated and (plan.cw, plan.ch) == (12, 40) and plan.frame == (12, 40)
    photo = np.arange(80 * 60 * 3, dtype=np.int64).reshape(80, 60, 3)
    rot = np.flip(np.swapaxes(photo[5:45, 10:22], 0, 1), 0)
    jj, ii = np.meshgrid(np.arange(40), np.arange(12))
    at = np.rint(apply(plan.h9, np.stack([jj.ravel(), ii.ravel()], axis=1).astype(np.float64))).astype(np.int64)
    assert (photo[at[:, 1], at[:, 0]].reshape(12, 40, 3) == rot).all()


def test_ensure_horizontal_threshold():
    for ch, rotated in ((59, False), (60, False), (61, True)):                   # cw = 40: 60 == 1.5 * 40 stays upright
        plan = plan_crop((100, 100), [[3, 2], [43, 2], [43, 2 + ch], [3, 2 + ch]], (32, 128))
        assert (plan.cw, plan.ch) == (40, ch) and plan.rotated == rotated
    assert plan_crop((100, 100), [[3, 2], [5, 2], [5, 5], [3, 5]], (32, 128)).rotated is False     # 3 == 1.5 * 2


@pytest.mark.parametrize("w,h", [(20, 12), (40, 12), (100, 20), (300, 20), (12, 40), (7, 33)])
def test_pad_widths_equal_target_width(w, h):
    plan = plan_crop((400, 400), [[5, 5], [5 + w, 5], [5 + w, 5 + h], [5, 5 + h]], (32, 128), mode='pad')
    frame = (w, h) if h > 1.5 * w else (h, w)
    assert plan.frame == frame
    assert plan.dst_w == target_width('pad', (32, 128), frame) <= 128
    assert plan.sx == 1.0 / (float(plan.dst_w) / float(frame[1])) and plan.sy == 1.0 / (32.0 / float(frame[0]))
    img = R.quad_crop_ref(np.full((400, 400, 3), 200, np.uint8), plan)
    assert (img[:, :, plan.dst_w:] == R.zero_pixel()[:, None, None]).all()
    assert (img[:, :, :plan.dst_w] != R.zero_pixel()[:, None, None]).all()


def test_other_modes_and_degenerate_quads_are_refused():
    box = [[5, 5], [25, 5], [25, 15], [5, 15]]
    for mode in ('keep_ratio', 'keep_size'):
        with pytest.raises(NotImplementedError):
            plan_crop((60, 60), box, (32, 128), mode=mode)
    with pytest.raises(ValueError):
        plan_crop((60, 60), box, (32, 128), rectify='hull')
    for flat in ([[5, 5], [25, 5], [25, 5], [5, 5]], [[7, 7]] * 4):
        for rectify in ('min_area_rect', 'quad'):
            with pytest.raises(ValueError):
                plan_crop((60, 60), flat, (32, 128), rectify=rectify)


@pytest.mark.parametrize("canvas", [(8, 24), (32, 128)])
@pytest.mark.parametrize("sides,angle", [((30, 10), 0), ((30, 10), 30), ((30, 10), -44), ((10, 30), 10), ((30, 10), 80),
                                         ((24, 16), 50)])
def test_closed_form_on_a_linear_photo(sides, angle, canvas):
    """I(x, y) = x + 2 y on 60 x 60 (values <= 177): the bilinear blend of a linear function is the function itself, so the
    restatement must give ((x + 2 y) - mean) / 255 at the point the PLAN maps each canvas pixel to -- computed here from the
    corners alone: the frame point (cx, cy) lies at p0 + cx / w (p1 - p0) + cy / h (p3 - p0), after undoing the rotation."""
    box = rotated_box(sides[0], sides[1], angle, centre=(30.0, 29.0))
    assert box.min() >= 1 and box.max() <= 58                              # fully inside: no zero border
    yy, xx = np.mgrid[0:60, 0:60]
    photo = np.repeat((xx + 2 * yy).astype(np.uint8)[..., None], 3, axis=2)
    for mode in ('resize', 'pad'):
        plan = plan_crop(photo.shape, box, canvas, mode=mode)
        H, W = canvas
        cx = np.clip((np.arange(W) + 0.5) * plan.frame[1] / plan.dst_w - 0.5, 0, plan.frame[1] - 1)[None, :]
        cy = np.clip((np.arange(H) + 0.5) * plan.frame[0] / H - 0.5, 0, plan.frame[0] - 1)[:, None]
        xc, yc = (plan.cw - 1 - cy, cx) if plan.rotated else (cx, cy)
        p = plan.corners
        px = p[0][0] + xc / plan.w * (p[1][0] - p[0][0]) + yc / plan.h * (p[3][0] - p[0][0])
        py = p[0][1] + xc / plan.w * (p[1][1] - p[0][1]) + yc / plan.h * (p[3][1] - p[0][1])
        want = ((px + 2 * py)[None] - np.array(R.RGB_MEAN)[:, None, None]) / 255.0
        want = np.where((np.arange(W) < plan.dst_w)[None, None, :], want, R.zero_pixel()[:, None, None])
        got = R.quad_crop_ref(photo, plan)
        assert got.dtype == np.float32 and got.shape == (3, H, W)
        assert np.abs(got - want).max() < 1e-5


def test_quad_mode_maps_a_trapezoid_onto_the_canvas_corners():
    trap = np.array([[12.0, 5.0], [48.0, 8.0], [50.0, 22.0], [10.0, 20.0]])
    for pts in (trap, trap[::-1], np.roll(trap, 1, axis=0)):
        assert (crop_frame(pts, 'quad')[0] == trap).all()
        plan = plan_crop((60, 60), pts, (32, 128), rectify='quad')
        assert plan.w == max(np.linalg.norm(trap[1] - trap[0]), np.linalg.norm(trap[2] - trap[3]))
        assert plan.h == max(np.linalg.norm(trap[2] - trap[1]), np.linalg.norm(trap[3] - trap[0]))
        assert np.abs(apply(plan.h9, frame_corners(plan)) - trap).max() < 1e-9
        assert abs(plan.h9[6]) > 1e-4 and abs(plan.h9[7]) > 1e-4               # a true projective map
        x, y, D, _ = R.source_points(plan)
        assert (D > 0).all()


def test_two_pass_restatement_is_close_to_the_fused_pass():
    """Reported, not gated beyond sanity: on a smooth photo both chains sample the same place."""
    yy, xx = np.mgrid[0:60, 0:60]
    photo = np.repeat((xx + 2 * yy).astype(np.uint8)[..., None], 3, axis=2)
    for box in (rotated_box(30, 10, 30, (30, 29)), rotated_box(10, 30, 10, (30, 29))):
        plan = plan_crop(photo.shape, box, (8, 24))
        one, two = R.quad_crop_ref(photo, plan), R.two_pass_ref(photo, plan, 'resize')
        # both chains evaluate the linear photo at the same frame points; the two-pass one rounds the intermediate crop to
        # uint8 (at most half a grey level per pixel) and the resize blends those rounded values convexly
        assert np.abs(one - two).max() <= 0.5 / 255 + 1e-5
