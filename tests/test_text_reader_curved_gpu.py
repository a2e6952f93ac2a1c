"""`TextReader(curved=True)` end to end with stub models: the detector marks every bright pixel, the recogniser spells a string
chosen by the crop's brightest grey level.  One photo holds a painted annular sector (R = 80, 14 px thick, 100 degrees: a word on
an arch) and a painted 60 x 20 bar.  The sector comes back as a ribbon on its circle and its characters follow the circle; the
bar is too short for a ribbon and keeps its box; with curved=False the same characters lie on the rectangle's midline, up to the
arc's sagitta away from the glyphs.

The representer's box score is the mean of the map over the RECTANGLE, of which the sector fills about a third, so the readers
here take `box_thresh=0.2`."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _db_ribbon_ref as R  # noqa: E402
from megreader_amd import Ribbon, StripCropper, TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.structure import SegDetectorRepresenter  # noqa: E402

SHAPE = (240, 320)                      # 3 : 4 like the detector's input below: the resize is the identity
CENTRE, RADIUS, THICK, SPAN = (160.0, 150.0), 80, 14, 100.0
LEVELS = {135: "AB12", 255: "HELLO"}


def photo():
    p = np.zeros(SHAPE + (3,), dtype=np.uint8)
    p[R.paint_sector(SHAPE[0], SHAPE[1], CENTRE, RADIUS, THICK, SPAN)] = 255
    p[R.paint_bar(SHAPE[0], SHAPE[1], (70.0, 200.0), 61, 21, 0.0)] = 135
    return p


def detector(x):
    return {'binary': (x[:, :1] > 0).float()}


class SpellByBrightest(torch.nn.Module):
    """[M, C, 1, T] scores that spell LEVELS[g], g the grey level nearest to the brightest pixel of the crop's channel 0, with a
    blank between the symbols (symbol k in column 2 k + 1).  Counts its calls."""

    def __init__(self, charset, T=16):
        super().__init__()
        self.charset, self.T, self.batches = charset, T, []

    def forward(self, crops):
        self.batches.append(crops.shape[0])
        grey = (crops[:, 0] * 255.0 + RGB_MEAN[0]).amax(dim=(1, 2)).cpu().numpy()
        out = torch.zeros((crops.shape[0], len(self.charset), 1, self.T), dtype=torch.float32)
        for m, g in enumerate(grey):
            text = LEVELS[min(LEVELS, key=lambda level: abs(level - g))]
            ids = [0] * self.T
            ids[1:2 * len(text):2] = [self.charset.index(ch) for ch in text]
            out[m, ids, 0, torch.arange(self.T)] = 1.0
        return out.to(crops.device)


def reader(curved, **kw):
    charset = EnglishCharset()
    rec = SpellByBrightest(charset)
    return TextReader(detector, rec, charset, representer=SegDetectorRepresenter(resize=True, box_thresh=0.2, device_geometry=True),
                      det_size=SHAPE, rec_size=(32, 128), curved=curved, **kw), rec


@functools.lru_cache(maxsize=None)
def _read(curved, chars):
    return reader(curved, chars=chars)[0].read([photo()])[0]


def off_circle(points):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return np.abs(np.sqrt(((p - CENTRE) ** 2).sum(axis=1)) - RADIUS)


def test_the_sector_is_read_along_its_ribbon_and_the_bar_keeps_its_box():
    found = _read(True, False)
    assert [item['text'] for item in found] == ["HELLO", "AB12"]                  # raster order: the arch starts higher up
    assert all(set(item) == {'quad', 'text', 'polygon'} for item in found)
    sector, bar = found
    outline = np.array(sector['polygon'])
    assert len(outline) % 2 == 0 and 10 <= len(outline) <= 36
    ribbon = Ribbon.from_polygon(outline)
    off = off_circle(ribbon.centres())
    print("sector: %d knots, interior centres %.2f px off the circle, end centres %.2f" % (ribbon.knots, off[1:-1].max(),
                                                                                           max(off[0], off[-1])))
    assert off[1:-1].max() <= 2.0
    assert bar['polygon'] == bar['quad'] and len(bar['quad']) == 4
    # the ribbon is the restatement's for the painted sector (the detector's map is the paint)
    xs, ys, box = R.candidate(R.paint_sector(SHAPE[0], SHAPE[1], CENTRE, RADIUS, THICK, SPAN))
    want = R.ribbon_of(xs, ys, box, 8)
    to_photo = [[(x / 320.0 * 320.0, y / 240.0 * 240.0) for x, y in side] for side in (want['top'], want['bot'])]    # step 9
    assert ribbon == Ribbon(*to_photo)


def test_character_boxes_follow_the_curve():
    curved, straight = _read(True, True)[0], _read(False, True)[0]
    assert curved['text'] == straight['text'] == "HELLO" and curved['quad'] == straight['quad']
    assert [c['char'] for c in curved['chars']] == list("HELLO") == [c['char'] for c in straight['chars']]
    on = off_circle([np.mean(c['quad'], axis=0) for c in curved['chars']])
    print("curved: character centres off the circle by", np.round(on, 2).tolist())
    assert on.max() <= 4.0
    # without the ribbon the same characters sit on the rectangle's midline, up to the arc's sagitta away from the glyphs
    q = np.array(straight['quad'])
    a, b = (q[0] + q[3]) / 2.0, (q[1] + q[2]) / 2.0
    centres = np.array([np.mean(c['quad'], axis=0) for c in straight['chars']])
    from_midline = np.abs((b[0] - a[0]) * (centres[:, 1] - a[1]) - (b[1] - a[1]) * (centres[:, 0] - a[0])) / np.hypot(*(b - a))
    away = off_circle(centres)
    print("straight: character centres off the circle by", np.round(away, 2).tolist())
    assert from_midline.max() <= 1.0 and away.max() >= 10.0
    assert all(0.99 <= c['score'] <= 1.0 for c in curved['chars'])


def test_chunks_the_straight_reader_and_a_representer_without_ribbons():
    whole, rec = reader(True)
    results = whole.read([photo(), photo()[:, ::-1].copy()])
    assert rec.batches == [4] and [len(f) for f in results] == [2, 2]
    chunked, rec1 = reader(True, max_crops=1)
    assert chunked.read([photo(), photo()[:, ::-1].copy()]) == results and rec1.batches == [1, 1, 1, 1]
    assert results[0] == _read(True, False)
    # curved=False (the default) is the reader as it was: no 'polygon', the boxes the representer gives
    plain = reader(False)[0].read([photo()])[0]
    default = TextReader(detector, SpellByBrightest(EnglishCharset()), EnglishCharset(), det_size=SHAPE, rec_size=(32, 128),
                         representer=SegDetectorRepresenter(resize=True, box_thresh=0.2, device_geometry=True)).read([photo()])[0]
    assert plain == default and all(set(item) == {'quad', 'text'} for item in plain)
    assert [item['quad'] for item in plain] == [item['quad'] for item in results[0]]
    assert [item['text'] for item in plain] == ["HELLO", "AB12"]
    scored = reader(True, scores=True)[0].read([photo()])[0]
    assert [item['polygon'] for item in scored] == [item['polygon'] for item in results[0]]
    assert 0.2 <= scored[0]['score'] < 0.7 and scored[1]['score'] > 0.9

    class BoxesOnly(object):
        def represent(self, batch, pred):
            return [[] for _ in batch['shape']], pred

    with pytest.raises(ValueError):
        TextReader(detector, rec, EnglishCharset(), representer=BoxesOnly(), curved=True)
    with pytest.raises(ValueError):
        TextReader(detector, rec, EnglishCharset(), curved=True, ribbon_slabs=2)
    TextReader(detector, rec, EnglishCharset(), representer=BoxesOnly())                # not asked for ribbons: fine


def test_the_tiled_path_reads_ribbons_off_the_fused_map():
    """`det_scales`: the detector on 128 x 160 tiles of the photo at its own scale; the fused map is the paint again, so the
    representer finds the ribbon it finds on the one-canvas map."""
    charset = EnglishCharset()
    tiled = TextReader(detector, SpellByBrightest(charset), charset, det_size=(128, 160), det_scales=(1.0,), det_halo=(8, 8),
                       det_align=8, rec_size=(32, 128), curved=True, scores=True,
                       representer=SegDetectorRepresenter(resize=True, box_thresh=0.2, device_geometry=True))
    found = tiled.read([photo()])[0]
    whole = _read(True, False)
    assert [item['text'] for item in found] == ["HELLO", "AB12"]
    assert [item['polygon'] for item in found] == [item['polygon'] for item in whole]
    assert [item['quad'] for item in found] == [item['quad'] for item in whole] and 0.2 <= found[0]['score'] < 0.7


def test_strip_cropper_crops_annotated_outlines():
    """`Ribbon.from_polygon` of an annotation, as CTW1500 and Total-Text give it, through `StripCropper`: the crop of the painted
    sector along its own outline is bright from end to end."""
    angles = np.radians(np.linspace(-SPAN / 2.0, SPAN / 2.0, 7))
    outer = [(CENTRE[0] + (RADIUS + 7.0) * math.sin(a), CENTRE[1] - (RADIUS + 7.0) * math.cos(a)) for a in angles]
    inner = [(CENTRE[0] + (RADIUS - 7.0) * math.sin(a), CENTRE[1] - (RADIUS - 7.0) * math.cos(a)) for a in angles]
    ribbon = Ribbon.from_polygon(outer + inner[::-1])
    batch = StripCropper(image_size=(32, 128)).crop([photo()], [[ribbon]])
    grey = (batch['image'][0, 0] * 255.0 + RGB_MEAN[0]).cpu().numpy()
    assert batch['index'].tolist() == [0] and grey[4:28, 2:126].min() > 200.0
