"""The ribbon rule of `mr_db_ribbons` (include/megreader_hip.h), checked on its restatement tests/_db_ribbon_ref.py without a
GPU: properties of the rule on painted 240 x 320 masks.  The kernel is held to the restatement bit for bit in
tests/test_db_ribbons_gpu.py."""
import functools
import math

import numpy as np
import pytest

import _db_boxes_ref as B
import _db_ribbon_ref as R
from megreader_amd.data.strip_crop import plan_strip
from megreader_amd.structure.ribbon import Ribbon

H, W = 240, 320
CENTRE = (160.0, 120.0)


@functools.lru_cache(maxsize=None)
def _ribbon(kind, args, S):
    mask = {'bar': R.paint_bar, 'sector': R.paint_sector, 'sine': R.paint_sine}[kind](H, W, *args)
    xs, ys, box = R.candidate(mask)
    return R.ribbon_of(xs, ys, box, S), box


def _line_distance(p, a, b):
    (px, py), (ax, ay), (bx, by) = p, a, b
    return abs((bx - ax) * (py - ay) - (by - ay) * (px - ax)) / math.hypot(bx - ax, by - ay)


@pytest.mark.parametrize("degrees", [0.0, 20.0, 90.0, -35.0])
def test_bars_give_straight_ribbons_that_cover_the_unclipped_bar(degrees):
    got, _ = _ribbon('bar', (CENTRE, 121, 17, degrees), 8)
    assert got['why'] == R.RIBBON and got['knots'] == 9
    for side in (got['top'], got['bot']):
        worst = max(_line_distance(p, side[0], side[-1]) for p in side)
        print("bar %g: knots off the chord by %.3f px" % (degrees, worst))
        assert worst <= 1.0
    # the four end corners against the painted bar (point extents 120 x 16) grown by the ribbon's own d
    d = got['d']
    print("bar %g: d = %.3f" % (degrees, d))
    assert abs(d - 120.0 * 16.0 * 1.5 / (2.0 * (120.0 + 16.0))) <= 1.0
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    if degrees == 90.0:                 # a vertical word reads downwards, its top on the photo's right: the frame turned
        c, s = 0.0, 1.0
    want = {}
    for name, (u, v) in {'T0': (-60.0 - d, -8.0 - d), 'T1': (60.0 + d, -8.0 - d), 'B0': (-60.0 - d, 8.0 + d),
                         'B1': (60.0 + d, 8.0 + d)}.items():
        want[name] = (CENTRE[0] + u * c - v * s, CENTRE[1] + u * s + v * c)
    ends = {'T0': got['top'][0], 'T1': got['top'][-1], 'B0': got['bot'][0], 'B1': got['bot'][-1]}
    worst = max(math.hypot(ends[k][0] - want[k][0], ends[k][1] - want[k][1]) for k in ends)
    print("bar %g: end corners off by %.3f px" % (degrees, worst))
    assert worst <= 3.0


def test_a_word_of_aspect_below_three_keeps_its_box():
    got, _ = _ribbon('bar', (CENTRE, 61, 21, 0.0), 8)
    assert got['why'] == R.SHORT and got['knots'] == 0 and got['top'] == []


SECTORS = [(80, 14, 100.0), (60, 10, 120.0), (30, 8, 140.0)]
ARC_CENTRE = (160.0, 150.0)


def _polar_measures(plan):
    """The three distortion measures of a plan's map onto its canvas, about ARC_CENTRE: (departure of the column-mean angle from a
    line in u, greatest spread of angle within a column, greatest spread of radius within a row), degrees and pixels."""
    Hc, Wc = plan.canvas
    vv, uu = np.mgrid[0:Hc, 0:Wc].astype(np.float64)
    p = plan.canvas_to_photo(np.stack([uu + 0.5, vv + 0.5], axis=-1))
    dx, dy = p[..., 0] - ARC_CENTRE[0], p[..., 1] - ARC_CENTRE[1]
    ang = np.degrees(np.arctan2(dx, -dy))                  # 0 at the top of the arch, growing along the reading direction
    rad = np.sqrt(dx * dx + dy * dy)
    mean = ang.mean(axis=0)
    u = np.arange(Wc, dtype=np.float64)
    fit = np.polyval(np.polyfit(u, mean, 1), u)
    return float(np.abs(mean - fit).max()), float((ang.max(axis=0) - ang.min(axis=0)).max()), \
        float((rad.max(axis=1) - rad.min(axis=1)).max())


@pytest.mark.parametrize("sector", SECTORS)
def test_sectors_follow_the_circle(sector):
    radius, thick, span = sector
    got, box = _ribbon('sector', (ARC_CENTRE, radius, thick, span), 16)
    assert got['why'] == R.RIBBON and 5 <= got['knots'] <= 18
    top, bot, d = np.array(got['top']), np.array(got['bot']), got['d']
    centres = (top + bot) / 2.0
    off = np.abs(np.sqrt(((centres - ARC_CENTRE) ** 2).sum(axis=1)) - radius)
    print("sector %s: %d knots, interior centres off the circle by %.3f px, end centres by %.3f" %
          (sector, got['knots'], off[1:-1].max(), max(off[0], off[-1])))
    assert off[1:-1].max() <= 2.0
    lengths = np.sqrt(((top - bot) ** 2).sum(axis=1))
    print("sector %s: ruling lengths off thickness + 2 d by %.3f px" % (sector, np.abs(lengths - (thick + 2.0 * d)).max()))
    assert np.abs(lengths - (thick + 2.0 * d)).max() <= 1.5
    # the strip map against the unclipped rectangle's, both onto 32 x 128
    rect, _ = B.mini_box(B.hull_of_points(B.unclip(box)))
    curved = _polar_measures(plan_strip((H, W), Ribbon(top, bot), (32, 128), 'resize'))
    straight = _polar_measures(plan_strip((H, W), Ribbon.from_box(rect), (32, 128), 'resize'))
    for name, a, b in zip(("column-mean angle off a line", "angle spread in a column", "radius spread in a row"), curved, straight):
        print("sector %s: %s %.3f against the rectangle's %.3f: ratio %.3f" % (sector, name, a, b, a / b))
        assert a <= 0.25 * b


SINES = [(12.0, 160.0), (20.0, 200.0), (25.0, 120.0)]


@pytest.mark.parametrize("sine", SINES)
def test_sine_bands_follow_the_sine(sine):
    amplitude, period = sine
    got, _ = _ribbon('sine', (120.0, amplitude, period), 16)
    assert got['why'] == R.RIBBON
    centres = (np.array(got['top']) + np.array(got['bot'])) / 2.0
    x = np.linspace(40.0, 280.0, 24001)
    curve = np.stack([x, 120.0 + amplitude * np.sin(2.0 * math.pi * x / period)], axis=1)
    off = [float(np.sqrt(((curve - c) ** 2).sum(axis=1)).min()) for c in centres[1:-1]]
    print("sine %s: %d knots, interior centres off the sine by %.3f px" % (sine, got['knots'], max(off)))
    assert max(off) <= 1.5


def test_fold_is_flagged_and_emitted_ribbons_have_convex_cells():
    # knots on a circle of radius 10 with half thickness 9: the unclip distance takes h + d beyond the radius
    angles = np.radians(np.linspace(-60.0, 60.0, 7))
    c = [(100.0 + 10.0 * math.sin(a), 100.0 - 10.0 * math.cos(a)) for a in angles]
    t = [(math.cos(a), math.sin(a)) for a in angles]
    why, top, bot, d = R.finish(c, t, [9.0] * 7, 1.5)
    assert 9.0 + d > 10.0 and why == R.FOLDED and not R.cells_convex(top, bot)
    why, top, bot, d = R.finish(c, t, [2.0] * 7, 1.5)
    assert 2.0 + d < 10.0 and why == R.RIBBON and R.cells_convex(top, bot)
    emitted = 0
    for kind, shapes, S in (('bar', [(CENTRE, 121, 17, a) for a in (0.0, 20.0, 90.0, -35.0)], 8),
                            ('sector', [(ARC_CENTRE,) + s for s in SECTORS], 16),
                            ('sine', [(120.0,) + s for s in SINES], 16)):
        for args in shapes:
            got, _ = _ribbon(kind, args, S)
            if got['knots']:
                emitted += 1
                assert R.cells_convex(got['top'], got['bot']), (kind, args)
    assert emitted == 10


def test_slab_sums_are_the_moments_of_the_component():
    mask = R.paint_sector(H, W, ARC_CENTRE, 80, 14, 100.0)
    xs, ys, box = R.candidate(mask)
    got = R.ribbon_of(xs, ys, box, 16)
    total = np.array(got['sums']).sum(axis=0)
    assert total.tolist() == [len(xs), int(xs.sum()), int(ys.sum()), int((xs * xs).sum()), int((xs * ys).sum()),
                              int((ys * ys).sum())]
