"""The planner of tiled multi-scale detection (megreader_amd/data/detection_tiles.py) and the numpy restatements of its two
kernels (tests/_det_tiles_ref.py), without a GPU: the 1-D cover, the canvases, the refusals, and that tiles cut from a whole map
stitch back to it."""
import math

import numpy as np
import pytest

import _det_tiles_ref as R
from megreader_amd.data.detection_tiles import DetectionTiler, canvas_size, cover_1d, cover_owner


@pytest.mark.parametrize("t,h,align", [(16, 4, 4), (24, 8, 8), (32, 0, 1)])
def test_cover_partitions_every_side(t, h, align):
    s = t - 2 * h
    for L in range(1, 201):
        origins, cores = cover_1d(L, t, h, align)
        K = len(origins)
        assert K == (1 if L <= t else math.ceil((L - t) / s) + 1), L
        assert all(o % align == 0 for o in origins) and origins == [k * s for k in range(K)], L
        assert cores[0][0] == 0 and cores[-1][1] == L, L
        assert all(cores[k][1] == cores[k + 1][0] for k in range(K - 1)), L          # no gap, no overlap
        for k, (lo, hi) in enumerate(cores):
            assert lo < hi and origins[k] <= lo and hi <= origins[k] + t, (L, k)     # not empty, inside its tile
            if K > 1:                                                               # at least h from the tile's inner borders
                assert (k == 0 or lo - origins[k] >= h) and (k == K - 1 or origins[k] + t - hi >= h), (L, k)
        held = [k for p in range(L) for k, (lo, hi) in enumerate(cores) if lo <= p < hi]
        assert held == [cover_owner(p, t, h, K) for p in range(L)], L
        assert origins[-1] + t >= L                                                  # the last tile reaches the end


def test_canvas_rounding_fit_and_base_level():
    assert canvas_size((48, 80), 1.0, (64, 96), 32) == (64, 96)         # 1.5 and 2.5 round up at .5
    assert canvas_size((47, 79), 1.0, (64, 96), 32) == (32, 64)
    assert canvas_size((5, 5), 1.0, (64, 96), 32) == (32, 32)           # never below align
    assert canvas_size((2160, 3840), 0.5, (576, 1024), 32) == (1088, 1920)
    assert canvas_size((2160, 3840), 'fit', (576, 1024), 32) == (576, 1024)
    tiler = DetectionTiler(tile=(64, 96), halo=(8, 8), scales=('fit', 1.0, 2.0, 2.0), align=8)
    plan = tiler.plan([(40, 50, 3), (64, 96, 3)])
    fit = plan.levels[0][0]
    assert fit.canvas == (64, 96) and (len(fit.ys), len(fit.xs)) == (1, 1)
    assert fit.scale_x == 1.0 / (96.0 / 50.0) and fit.scale_y == 1.0 / (64.0 / 40.0)
    assert plan.base == [2, 2] and plan.sizes == [(80, 104), (128, 192)]      # the first of the two equal largest levels
    assert DetectionTiler(tile=(64, 96), halo=(8, 8), scales=('fit', 1.0), align=8).plan([(64, 96)]).base == [0]     # a tie
    levels, photos, max_pixels = plan.stitch_tables()
    assert max_pixels == 128 * 192 and [(e.hc, e.wc, e.ratio_x, e.ratio_y) for e in levels][:2] == [
        (64, 96, 96.0 / 104.0, 64.0 / 80.0), (40, 48, 48.0 / 104.0, 40.0 / 80.0)]          # (double)wc / wb, (double)hc / hb
    assert [(p.hb, p.wb, p.levels, p.first_level, p.base) for p in photos] == [(80, 104, 4, 0, 2), (128, 192, 4, 4, 2)]
    assert plan.offsets == [0, 80 * 104] and plan.total == 80 * 104 + 128 * 192
    assert plan.T == len(plan.tiles) == sum(len(lv.ys) * len(lv.xs) for levels in plan.levels for lv in levels)
    for levels in plan.levels:                                                   # tile (ky, kx) is first + ky * Kx + kx
        for l, lv in enumerate(levels):
            for ky, y0 in enumerate(lv.ys):
                for kx, x0 in enumerate(lv.xs):
                    assert plan.tiles[lv.first + ky * len(lv.xs) + kx][1:] == (l, ky, kx, x0, y0)


def test_refusals_name_the_value():
    ok = dict(tile=(64, 96), halo=(8, 8), align=8)
    for kw, word in ((dict(scales=()), "()"), (dict(scales=(0.0,)), "0.0"), (dict(scales=(-1.5,)), "-1.5"),
                     (dict(scales=(float('nan'),)), "nan"), (dict(scales=(float('inf'),)), "inf"), (dict(scales=('big',)), "big"),
                     (dict(fuse='sum'), "sum"), (dict(halo=(32, 8)), "32"), (dict(halo=(8, 48)), "48"),
                     (dict(tile=(60, 96)), "60"), (dict(halo=(8, 4)), "4"), (dict(align=0), "0")):
        with pytest.raises(ValueError) as e:
            DetectionTiler(**dict(ok, **kw))
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError) as e:
        DetectionTiler().plan([(2160, 3840)])
    assert "(2176, 3840)" in str(e.value) and "2048" in str(e.value) and "mr_db_boxes" in str(e.value)
    assert DetectionTiler(max_canvas=(2176, 3840)).plan([(2160, 3840)]).sizes == [(2176, 3840)]
    assert DetectionTiler(scales=('fit', 0.5)).plan([(2160, 3840)]).sizes == [(1088, 1920)]


def cut(whole, plan, level_of):
    """The maps of the plan's tiles cut from whole maps (`level_of(photo, level)` -> [Hc, Wc]), zeros beyond the canvas."""
    th, tw = plan.tile
    maps = np.zeros((plan.T, th, tw), dtype=np.float32)
    for t, (i, l, _, _, x0, y0) in enumerate(plan.tiles):
        win = level_of(i, l)[y0:y0 + th, x0:x0 + tw]
        maps[t, :win.shape[0], :win.shape[1]] = win
    return maps


@pytest.mark.parametrize("scales,fuse", [((1.0,), 'max'), ((1.0,), 'mean'), ((1.0, 1.0), 'mean'), ((1.0, 1.0), 'max')])
def test_tiles_cut_from_a_whole_map_stitch_back_to_it(scales, fuse):
    rng = np.random.RandomState(3)
    tiler = DetectionTiler(tile=(16, 24), halo=(4, 4), scales=scales, fuse=fuse, align=4)
    plan = tiler.plan([(37, 53), (64, 41)])
    assert plan.sizes == [(36, 52), (64, 40)] and plan.T > 2 * len(scales)
    whole = [rng.uniform(0.0, 1.0, size).astype(np.float32) for size in plan.sizes]
    maps = cut(whole, plan, lambda i, l: whole[i])
    levels, photos, _ = plan.stitch_tables()
    out = np.full(plan.total, np.nan, dtype=np.float32)
    R.tile_stitch_ref(maps, 16, 24, (4, 4), R.entries(levels), R.entries(photos, 2), fuse, out)
    for o, size, want in zip(plan.offsets, plan.sizes, whole):
        got = out[o:o + size[0] * size[1]].reshape(size)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_sample_restatement_is_the_window_of_the_whole_canvas():
    rng = np.random.RandomState(5)
    photos = [rng.randint(0, 256, (37, 53, 3)).astype(np.uint8), rng.randint(0, 256, (64, 41, 3)).astype(np.uint8)]
    tiler = DetectionTiler(tile=(16, 24), halo=(4, 4), scales=(1.0, 0.5, 1.7, 'fit'), align=1)
    plan = tiler.plan([p.shape for p in photos])
    assert plan.levels[0][0].canvas == (37, 53)                                  # the copy shortcut
    tiles = R.entries(plan.tile_descs(), plan.T)
    got = R.tile_sample_ref(photos, tiles, 16, 24)
    outside = 0
    for t, (i, l, _, _, x0, y0) in enumerate(plan.tiles):
        hc, wc = plan.levels[i][l].canvas
        want = np.zeros((3, 16, 24), dtype=np.float32)
        win = R.whole_canvas(photos[i], hc, wc)[:, y0:y0 + 16, x0:x0 + 24]
        want[:, :win.shape[1], :win.shape[2]] = win
        outside += want[0].size - win[0].size
        assert np.array_equal(got[t].view(np.uint32), want.view(np.uint32)), t       # 0.0 (all bits zero) outside
    assert outside > 0
