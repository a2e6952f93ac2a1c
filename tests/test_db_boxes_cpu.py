"""The device algorithm of `mr_db_boxes`, restated in tests/_db_boxes_ref.py, against the oracle of the host path
(oracle/db_post.py) and against db_geometry.convex_hull -- no GPU.  tests/test_db_boxes_gpu.py then holds the kernels equal to
the restatement bit for bit."""
import functools

import numpy as np
import pytest

import _db_boxes_ref as R
from megreader_amd.structure import db_geometry as G
from oracle import db_post as O

SEEDS = [3, 4, 5, 6, 11, 12]


@functools.lru_cache(maxsize=None)
def _maps(seed):
    maps = O.synthetic_maps(seed, N=3, H=96, W=128, regions=7)
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def _restated(seed, resize):
    maps = _maps(seed)
    dest = [(384, 192)] * 3 if resize else [(128, 96)] * 3
    return R.db_boxes(maps, maps > 0.3, dest)


@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_equals_oracle(seed, resize):
    maps = _maps(seed)
    got = R.box_lists(_restated(seed, resize))
    total = 0
    for n in range(3):
        want = (O.boxes_from_bitmap(maps[n], maps[n] > 0.3, 384, 192, resize=True) if resize
                else O.boxes_from_bitmap(maps[n], maps[n] > 0.3, 128, 96))
        assert got[n] == want, (n, got[n], want)
        total += len(want)
    assert total >= 3, "the synthetic maps must produce boxes"


@pytest.mark.parametrize("seed", SEEDS)
def test_restated_slots(seed):
    """Ranks, statuses and the candidate rectangles against the oracle's own stages."""
    maps, out = _maps(seed), _restated(seed, False)
    for n in range(3):
        comps = O.components(maps[n] > 0.3)
        assert out['components'][n] == len(comps)
        kept = 0
        for k, comp in enumerate(comps[:100]):
            box, sside = O.mini_box(comp)
            assert out['cand'][n, k].tolist() == box
            if sside < 3:
                want = R.SHORT
            elif 0.7 > O.box_score(maps[n], box):
                want = R.WEAK
            else:
                want = R.SMALL if O.mini_box(O.unclip(box))[1] < 5 else R.KEPT
            assert out['status'][n, k] == want, (n, k)
            if want >= R.WEAK:
                s, c = out['cand_sums'][n, k]
                assert c > 0 and abs(float(s) / float(c) - O.box_score(maps[n], box)) < 1e-5    # f32 sums of < 2000 pixels
            kept += want == R.KEPT
        assert (out['status'][n, len(comps):] == R.NONE).all() and out['count'][n] == kept


def _mask(H, W, pixels):
    m = np.zeros((H, W), bool)
    for x, y in pixels:
        m[y, x] = True
    return m


def _ring(H=40, W=48, cx=23, cy=19, r0=9, r1=14):
    yy, xx = np.mgrid[0:H, 0:W]
    d = (xx - cx) ** 2 + (yy - cy) ** 2
    return (d >= r0 * r0) & (d <= r1 * r1)


def _c_shape(H=40, W=48):
    m = _ring(H, W)
    m[14:25, 30:] = False         # open the ring to the right
    return m


SHAPES = {
    'ring': _ring(),
    'c': _c_shape(),
    'one pixel': _mask(8, 8, [(3, 5)]),
    'two pixels': _mask(8, 8, [(3, 5), (4, 4)]),
    'two pixels in a row': _mask(8, 8, [(3, 5), (4, 5)]),
    'line': _mask(8, 32, [(x, 3) for x in range(5, 25)]),
    'column': _mask(32, 8, [(3, y) for y in range(5, 25)]),
    'full': np.ones((64, 64), bool),
    'lens outline': R.lens_outline(),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hull_from_row_extremes_equals_convex_hull_of_all_pixels(name):
    mask = SHAPES[name]
    root, roots = R.label_components(mask)
    assert len(roots) == 1
    ys, xs = np.nonzero(mask)
    want = G.convex_hull(zip(xs.tolist(), ys.tolist()))
    got = R.hull_from_extremes(R.row_extremes(root, roots[0]))
    assert [(float(x), float(y)) for x, y in got] == want
    assert R.mini_box(got) == G.mini_box(list(zip(xs.tolist(), ys.tolist())))
    if name == 'lens outline':
        assert len(got) == 264                  # every row end is a vertex: more edges than one round of the kernel's calipers


@pytest.mark.parametrize("seed", [3, 4])
def test_hulls_of_synthetic_components(seed):
    maps = _maps(seed)
    for n in range(3):
        root, roots = R.label_components(maps[n] > 0.3)
        comps = O.components(maps[n] > 0.3)
        assert len(roots) == len(comps)
        for r, comp in zip(roots, comps):
            assert min(comp, key=lambda p: (p[1], p[0])) == (r % 128, r // 128)
            got = R.hull_from_extremes(R.row_extremes(root, r))
            assert [(float(x), float(y)) for x, y in got] == G.convex_hull(comp)


def test_sequential_choice_is_not_an_arg_min():
    def tolerant_arg_min(areas):
        return min(i for i, a in enumerate(areas) if a <= min(areas) + 1e-12)
    # a run of areas each 0.8e-12 below the one before: the scan moves its base when the gap to the BASE passes 1e-12
    # (index 2, 1.6e-12 below index 0) and then stays (index 3 is only 0.4e-12 below index 2)
    areas = [10.0, 10.0 - 0.8e-12, 10.0 - 1.6e-12, 10.0 - 2.0e-12]
    assert R.sequential_choice(areas) == 2
    assert int(np.argmin(areas)) == 3                              # the plain arg-min takes the last
    assert tolerant_arg_min(areas[:3]) == 1                        # the first within 1e-12 of the minimum is another one too
    assert R.sequential_choice(areas[:3]) == 2
    # ... and an area below best - 1e-12 becomes the new base
    areas = [10.0, 10.0 - 6e-13, 9.0, 9.0 - 6e-13, 8.0]
    assert R.sequential_choice(areas) == 4
    assert R.sequential_choice([5.0, 5.0, 4.0, 4.0]) == 2          # ties keep the first edge
    # the same rule inside db_geometry.min_area_rect: the restatement picks the host's rectangle on a square (4 equal areas)
    square = [(0, 0), (4, 0), (4, 4), (0, 4)]
    assert R.min_area_rect(G.convex_hull(square)) == G.min_area_rect(square)


def test_box_sums_order_is_a_sum():
    g = np.random.default_rng(0)
    pred = g.uniform(0, 1, (40, 50)).astype(np.float32)
    box = [[5.5, 3.2], [30.9, 8.1], [28.0, 25.7], [2.6, 20.8]]
    s, c = R.box_sums(pred, box)
    assert abs(float(s) / float(c) - O.box_score(pred, box)) < 1e-6 and c == int(c) > 300
    assert s.dtype == np.float32
