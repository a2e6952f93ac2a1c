"""TextReader(scores=True): every item carries the detector's confidence in its box, from
`SegDetectorRepresenter.represent_scored` (one chain of launches, one copy).  Stub models with known answers: dark photos with
bright rectangles (one of them turned), a detector that turns brightness into a probability, a recogniser that spells the crop's
brightness.  The scored reader on the device-geometry representer must read what the default reader reads; the scores must be
those of `represent_scored`, also behind a box that the cropper drops."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.structure import SegDetectorRepresenter  # noqa: E402

A, B = 60.0, 20.0
DET_SIZE = (240, 320)
# (photo shape, [(centre, angle in degrees, grey level)])
SCENES = [((120, 160), [((50.0, 30.0), 0.0, 135), ((100.0, 85.0), 20.0, 255)]),
          ((150, 200), [((60.0, 110.0), 0.0, 215), ((140.0, 40.0), 0.0, 175)]),
          ((90, 120), []),                                  # a photo without boxes
          ((8, 200), [])]                                   # a dark strip: the detector below invents two regions in it
STRIP = 3
# regions (rows, columns, probability) of the detector's 240 x 320 map of the strip.  The first is 4 px high: unclipped it
# spans rows 115.3 .. 124.7, which the strip's 8 rows scale to 3.84 .. 4.16 -- both round to 4, a box without height, which the
# cropper drops.  The second keeps a height.
INVENTED = [((118, 123), (100, 141), 0.9), ((150, 201), (200, 261), 0.8)]


def paint(shape, rects):
    photo = np.zeros(shape + (3,), dtype=np.uint8)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    for (cx, cy), angle, level in rects:
        t = math.radians(angle)
        along = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
        across = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
        photo[(np.abs(along) <= A / 2) & (np.abs(across) <= B / 2)] = level
    return photo


def photos():
    return [paint(shape, rects) for shape, rects in SCENES]


def detector(x):
    """Pixels brighter than the mean are text, the surer the brighter (0.86 .. 1): boxes get different scores."""
    v = x[:, :1]
    prob = torch.where(v > 0, (0.85 + 0.3 * v).clamp(max=1.0), torch.zeros_like(v))
    if x.shape[0] > STRIP:
        for (r0, r1), (c0, c1), p in INVENTED:
            prob[STRIP, 0, r0:r1, c0:c1] = p
    return {'binary': prob}


class SpellBrightness(torch.nn.Module):
    """ids that spell the mean grey level of the crop in hex ('ids' decoding: no head, no CTC)."""

    def __init__(self, charset):
        super().__init__()
        self.charset = charset

    def forward(self, crops):
        grey = (crops[:, 0] * 255.0 + RGB_MEAN[0]).mean(dim=(1, 2)).cpu().numpy()
        ids = [[self.charset.index(ch) for ch in "%02X" % int(round(float(g)))] for g in grey]
        return torch.tensor(ids, dtype=torch.int64, device=crops.device)


def flat(quad):
    return len({p[0] for p in quad}) == 1 or len({p[1] for p in quad}) == 1


def test_scores_ride_along_and_stay_with_their_boxes():
    charset = EnglishCharset()
    rep = SegDetectorRepresenter(resize=True, device_geometry=True)
    reader = TextReader(detector, SpellBrightness(charset), charset, representer=rep, det_size=DET_SIZE, decode='ids',
                        scores=True)
    results = reader.read(photos())
    plain = TextReader(detector, SpellBrightness(charset), charset, det_size=DET_SIZE, decode='ids').read(photos())
    assert [len(found) for found in plain] == [2, 2, 0, 1]
    assert all(set(item) == {'quad', 'text'} for found in plain for item in found)            # the default reader is unchanged
    assert [[{'quad': item['quad'], 'text': item['text']} for item in found] for found in results] == plain
    assert len({item['text'] for found in plain for item in found}) >= 4                      # the crops differ, so do the strings

    # what represent_scored says about the same maps
    batch, _ = reader._upload(photos())
    pred = detector(batch['image'])
    boxes, scores, _ = rep.represent_scored({'image': batch['image'], 'shape': [p.shape[:2] for p in photos()]}, pred)
    assert [len(b) for b in boxes] == [2, 2, 0, 2]
    assert flat(boxes[STRIP][0]) and not flat(boxes[STRIP][1])          # the dropped box comes BEFORE the one that stays
    for found, bs, ss in zip(results, boxes, scores):
        assert [(item['quad'], item['score']) for item in found] == [(b, s) for b, s in zip(bs, ss) if not flat(b)]
    got = [item['score'] for found in results for item in found]
    assert all(0.7 <= s <= 1.0 for s in got) and len(set(got)) == len(got) == 5
    assert abs(results[STRIP][0]['score'] - 0.8) < 1e-5                 # the f32 mean of 51 x 61 pixels that all hold 0.8
    # a host-geometry representer serves scores too
    host = TextReader(detector, SpellBrightness(charset), charset, det_size=DET_SIZE, decode='ids', scores=True).read(photos())
    assert host == results
    assert TextReader(detector, SpellBrightness(charset), charset, det_size=DET_SIZE, decode='ids', scores=True).read(
        [photos()[2]]) == [[]]
