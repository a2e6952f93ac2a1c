"""`Ribbon` (structure/ribbon.py) and `plan_strip` / `StripPlan` (data/strip_crop.py) without a GPU: the strip map of a box is the
quad crop's map, outlines round-trip, and what is refused."""
import numpy as np
import pytest

from megreader_amd.data.quad_crop import DegenerateQuad, plan_crop
from megreader_amd.data.strip_crop import StripDesc, plan_strip
from megreader_amd.structure.ribbon import Ribbon

QUADS = {
    'upright': [[20.0, 30.0], [140.0, 30.0], [140.0, 62.0], [20.0, 62.0]],
    'tilted': [[30.0, 40.0], [133.9, 100.0], [117.9, 127.7], [14.0, 67.7]],                 # 120 x 32 at 30 degrees
    'tilted back': [[20.0, 90.0], [122.1, 52.8], [132.4, 81.0], [30.3, 118.2]],             # about -20 degrees
    'vertical': [[50.0, 10.0], [74.0, 10.0], [74.0, 130.0], [50.0, 130.0]],
    'vertical tilted': [[60.0, 12.0], [83.6, 16.2], [62.8, 134.4], [39.2, 130.2]],          # 24 x 120, 10 degrees off the vertical
}


@pytest.mark.parametrize("mode", ['resize', 'pad'])
@pytest.mark.parametrize("name", sorted(QUADS))
def test_the_strip_map_of_a_box_is_the_quad_crops_map(name, mode):
    quad = QUADS[name]
    crop = plan_crop((200, 220), quad, (32, 128), mode)
    strip = plan_strip((200, 220), Ribbon.from_box(quad), (32, 128), mode)
    assert crop.rotated == name.startswith('vertical')
    assert (strip.dst_w, strip.frame, strip.canvas) == (crop.dst_w, tuple(crop.frame), tuple(crop.canvas))
    assert (strip.sx, strip.sy, strip.cu1, strip.cv1) == (crop.sx, crop.sy, crop.cu1, crop.cv1)
    vv, uu = np.mgrid[-4:37:0.5, -8:137:0.5]
    grid = np.stack([uu, vv], axis=-1)
    worst = float(np.abs(strip.canvas_to_photo(grid) - crop.canvas_to_photo(grid)).max())
    print("%s, %s: strip map and quad map differ by %.3g px" % (name, mode, worst))
    assert worst <= 1e-9


def test_outlines_round_trip_and_from_box_is_two_rulings():
    g = np.random.default_rng(5)
    r = Ribbon(g.uniform(0, 100, (7, 2)), g.uniform(0, 100, (7, 2)))
    assert r.polygon().shape == (14, 2) and np.array_equal(r.polygon()[:7], r.top) and np.array_equal(r.polygon()[7:], r.bottom[::-1])
    assert Ribbon.from_polygon(r.polygon()) == r and Ribbon.from_polygon(r.polygon().tolist()) == r
    assert Ribbon.from_polygon(r.polygon()[::-1]) != r
    box = Ribbon.from_box(QUADS['upright'])
    assert box.knots == 2 and box.polygon().tolist() == QUADS['upright']


def test_a_plan_fills_its_descriptor():
    top = [[10.0, 20.0], [40.0, 12.0], [70.0, 20.0]]
    bot = [[12.0, 40.0], [40.0, 30.0], [68.0, 40.0]]
    plan = plan_strip((100, 100), Ribbon(top, bot), (32, 128), 'pad')
    c = (np.array(top) + np.array(bot)) / 2.0
    seg = np.sqrt(((c[1:] - c[:-1]) ** 2).sum(axis=1))
    assert plan.s.tolist() == [0.0, seg[0], seg[0] + seg[1]] and plan.w == plan.s[-1]
    assert plan.hgt == max(np.hypot(2.0, 20.0), 18.0) and (plan.cw, plan.ch) == (int(plan.w), int(plan.hgt))
    d = plan.fill(StripDesc(), 3)
    assert (d.image, d.dst_w, d.knots, d.reserved) == (3, plan.dst_w, 3, 0) and plan.dst_w < 128
    assert [d.s[i] for i in range(3)] == plan.s.tolist() and d.s[3] == 0.0
    assert [[d.top[i][0], d.top[i][1]] for i in range(3)] == top and [[d.bot[i][0], d.bot[i][1]] for i in range(3)] == bot
    # a canvas point on a ruling comes back on the ruling
    mid = plan.canvas_to_photo([[(plan.s[1] + 0.5) / plan.sx, 0.5 / plan.sy]])
    assert np.abs(mid - np.array(top[1])).max() <= 1e-9


def test_refusals():
    with pytest.raises(ValueError):
        Ribbon.from_polygon([[0, 0], [1, 0], [2, 0], [2, 1], [0, 1]])                      # an odd number of points
    with pytest.raises(ValueError):
        Ribbon([[0, 0]], [[0, 1]])                                                          # one ruling
    with pytest.raises(ValueError):
        Ribbon(np.zeros((19, 2)), np.ones((19, 2)))                                         # more than 18
    with pytest.raises(ValueError):
        Ribbon(np.zeros((3, 2)), np.ones((4, 2)))
    with pytest.raises(DegenerateQuad):
        plan_strip((50, 50), Ribbon([[5, 5], [5, 5]], [[5, 9], [5, 9]]), (32, 128), 'resize')      # no length
    with pytest.raises(DegenerateQuad):
        plan_strip((50, 50), Ribbon([[5, 5], [30, 5]], [[5, 5], [30, 5]]), (32, 128), 'resize')    # no height
    with pytest.raises(DegenerateQuad):
        plan_strip((50, 50), Ribbon([[5, 5], [30, 5], [30, 5]], [[5, 9], [30, 9], [30, 9]]), (32, 128), 'resize')
    with pytest.raises(DegenerateQuad):
        Ribbon.from_box([[5, 5], [30, 5], [30, 5], [5, 5]])
    with pytest.raises(NotImplementedError):
        plan_strip((50, 50), Ribbon.from_box(QUADS['upright']), (32, 128), 'keep_ratio')
    with pytest.raises(TypeError):
        plan_strip((50, 50), QUADS['upright'], (32, 128), 'resize')
