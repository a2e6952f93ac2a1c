"""`TextReader(det_scales=...)`: the detector on tiles of the photo at its own scale, fused per photo (data/detection_tiles.py).
Stub models in the manner of tests/test_text_reader_gpu.py (copied, not imported): the detector marks every bright pixel, the
recogniser spells one word.  A painted a x b rectangle is expected back grown by the representer's unclip distance
d = 1.5 a b / (2 (a + b)) on every side, within 3 px, corners in the order top-left, top-right, bottom-right, bottom-left."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _jpeg_ref as jpeg_ref  # noqa: E402
from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.structure.db_geometry import mini_box  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, DET_SIZE = (240, 400), (64, 96)
SMALL, LARGE = (14.0, 5.0), (60.0, 20.0)
SMALL_AT = [(200.0, 30.0), (330.0, 100.0), (60.0, 180.0), (250.0, 200.0)]
LARGE_AT = (88.0, 56.0)             # on the corner of four cores: tiles of 64 x 96 with halo 8 own rows [0, 56) and columns [0, 88) first
TILED = dict(det_size=DET_SIZE, det_scales=(1.0,), det_halo=(8, 8), det_align=8)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_split")


def grow(a, b):
    return 1.5 * a * b / (2.0 * (a + b))


def paint(rects, shape=SHAPE):
    """rects: [((a, b), (cx, cy))], axis-parallel, grey level 255 on black."""
    photo = np.zeros(shape + (3,), dtype=np.uint8)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    for (a, b), (cx, cy) in rects:
        photo[(np.abs(xx - cx) <= a / 2) & (np.abs(yy - cy) <= b / 2)] = 255
    return photo


def detector(x):
    return {'binary': (x[:, :1] > 0).float()}


class SpellOneWord(torch.nn.Module):
    """[M, C, 1, T] scores that spell "X9" for every crop."""

    def __init__(self, charset, T=8):
        super().__init__()
        self.charset, self.T = charset, T

    def forward(self, crops):
        out = torch.zeros((crops.shape[0], len(self.charset), 1, self.T), dtype=torch.float32)
        ids = [0] * self.T
        ids[1:4:2] = [self.charset.index(ch) for ch in "X9"]
        out[:, ids, 0, torch.arange(self.T)] = 1.0
        return out.to(crops.device)


def reader(**kw):
    charset = EnglishCharset()
    return TextReader(detector, SpellOneWord(charset), charset, **kw)


def ordered(quad):
    return np.array(mini_box([tuple(p) for p in quad])[0], dtype=np.float64)


def expected(size, centre):
    (a, b), (cx, cy), d = size, centre, grow(*size)
    return np.array([[cx - a / 2 - d, cy - b / 2 - d], [cx + a / 2 + d, cy - b / 2 - d], [cx + a / 2 + d, cy + b / 2 + d],
                     [cx - a / 2 - d, cy + b / 2 + d]], dtype=np.float64)


def check(found, rects):
    """One box per painted rectangle, each within 3 px of its rectangle grown by the unclip distance."""
    assert len(found) == len(rects)
    left = list(rects)
    for item in found:
        got = ordered(item['quad'])
        dist = [np.abs(got - expected(size, centre)).max() for size, centre in left]
        k = int(np.argmin(dist))
        print("box at %s: %.2f px from the painted rectangle grown by %.2f" % (left[k][1], dist[k], grow(*left[k][0])))
        assert dist[k] < 3.0
        assert item['text'] == "X9"
        del left[k]


def test_small_words_are_lost_on_one_canvas_and_found_on_tiles():
    rects = [(SMALL, at) for at in SMALL_AT]
    photo = paint(rects)
    assert reader(det_size=DET_SIZE).read([photo]) == [[]]              # 14 x 5 squeezed by 4.2 x 3.75: under min_size
    tiled = reader(**TILED)
    assert tiled.det_tiler.plan([photo.shape]).T == 5 * 5
    found = tiled.read([photo])
    check(found[0], rects)
    assert tiled.read([]) == []
    assert tiled.read([paint([]), photo]) == [[], found[0]]             # per photo, in order


def test_a_word_across_a_core_border_is_one_box_the_box_of_one_tile():
    rects = [(LARGE, LARGE_AT)]
    photo = paint(rects)
    tiled = reader(**TILED)
    plan = tiled.det_tiler.plan([photo.shape])
    assert plan.levels[0][0].cores_y[0] == (0, 56) and plan.levels[0][0].cores_x[0] == (0, 88)
    found = tiled.read([photo])
    check(found[0], rects)
    one_tile = reader(det_size=SHAPE, det_scales=(1.0,), det_halo=(8, 8), det_align=8)
    assert one_tile.det_tiler.plan([photo.shape]).T == 1
    assert found == one_tile.read([photo])


def test_fit_and_full_scale_together_find_large_and_small_words():
    """The coarse level is resampled onto the fine one before the maximum, so a region is as wide as the wider of the two: the
    extent of a box is no longer the unclip formula's.  Found means: one box per rectangle, its centre within 3 px of the
    rectangle's."""
    rects = [(LARGE, LARGE_AT)] + [(SMALL, at) for at in SMALL_AT]
    photo = paint(rects)
    found = reader(det_size=DET_SIZE, det_scales=('fit', 1.0), det_halo=(8, 8), det_align=8).read([photo])[0]
    assert len(found) == len(rects)
    left = [centre for _, centre in rects]
    for item in found:
        centre = ordered(item['quad']).mean(axis=0)
        dist = [np.abs(centre - np.asarray(c)).max() for c in left]
        k = int(np.argmin(dist))
        print("box centre %.2f px from the rectangle at %s" % (dist[k], left[k]))
        assert dist[k] < 3.0
        del left[k]


def test_scores_and_encoded_photos():
    rects = [(LARGE, LARGE_AT)] + [(SMALL, at) for at in SMALL_AT]
    photo = paint(rects)
    plain = reader(**TILED).read([photo])
    scored = reader(scores=True, **TILED).read([photo])
    assert [dict(item, score=None) for item in scored[0]] == [dict(item, score=None) for item in plain[0]]
    assert all(isinstance(item['score'], float) and 0.7 <= item['score'] <= 1.0 for item in scored[0])
    with open(os.path.join(GOLDEN, "reader_scene0.jpg"), "rb") as f:
        blob = f.read()
    pixels = np.ascontiguousarray(jpeg_ref.decode(blob))
    want = reader(**TILED).read([pixels])
    assert len(want[0]) == 2                                            # the two 60 x 20 rectangles of the scene
    assert reader(encoded=True, **TILED).read([blob]) == want


def test_without_det_scales_nothing_changes():
    rects = [(LARGE, (200.0, 120.0))]
    photo = paint(rects)
    size = (120, 200)                                                   # half the photo: the rectangle arrives as 30 x 10
    want = reader(det_size=size).read([photo])
    assert len(want[0]) == 1
    explicit = reader(det_size=size, det_scales=None, det_halo=(64, 64), det_fuse='max', det_batch=8)
    assert explicit.det_tiler is None and explicit.read([photo]) == want


def test_bad_arguments_are_refused_in_the_constructor():
    for kw, word in ((dict(det_scales=()), "()"), (dict(det_scales=(0.0,)), "0.0"), (dict(det_scales=(1.0,), det_fuse='sum'), "sum"),
                     (dict(det_scales=(1.0,), det_halo=(32, 8)), "32"), (dict(det_scales=(1.0,), det_batch=0), "0"),
                     (dict(det_scales=(1.0,), det_halo=(8, 8), det_align=32), "8"),
                     (dict(det_scales=(1.0,), det_size=(60, 96)), "60")):
        with pytest.raises(ValueError) as e:
            reader(**dict(dict(det_size=DET_SIZE, det_halo=(8, 8), det_align=8), **kw))
        assert word in str(e.value), (kw, str(e.value))
