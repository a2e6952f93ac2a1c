"""TextReader (megreader_amd/reader.py) end to end: photos -> detector -> SegDetectorRepresenter -> QuadCropper -> recogniser ->
strings.  The plumbing is checked with stub models whose answers are known -- the detector marks every bright pixel, the recogniser
spells a string chosen by the crop's mean brightness -- and then with a real (randomly initialised) CRNN against the same steps
done by hand.

What the boxes must be.  `SegDetectorRepresenter` treats a region as DB's SHRUNK text kernel and unclips it: an a x b rectangle
comes back grown by d = 1.5 a b / (2 (a + b)) on every side (structure/db_geometry.py `unclip`; 11.25 px for 60 x 20).  So a
painted rectangle is expected back as that rectangle grown by d, within 3 px, after both are put in the order top-left,
top-right, bottom-right, bottom-left."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd import QuadCropper, TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.ops.decode import ctc_greedy_decode  # noqa: E402
from megreader_amd.structure.db_geometry import mini_box  # noqa: E402

A, B = 60.0, 20.0                                   # every painted rectangle: the crops then hold the same share of bright pixels
GROW = 1.5 * A * B / (2.0 * (A + B))                # the representer's unclip distance
SHARE = A * B / ((A + 2 * GROW) * (B + 2 * GROW))   # bright share of an unclipped box
LEVELS = {135: "AB12", 175: "HELLO", 215: "X9", 255: "TEXT"}
# (photo shape, [(centre, angle in degrees, grey level)]); both photos are 3 : 4 like the detector's input, so the detector's
# resize is isotropic and the unclip distance is the same in photo pixels
SCENES = [((120, 160), [((50.0, 30.0), 0.0, 135), ((100.0, 85.0), 20.0, 255)]),
          ((150, 200), [((60.0, 110.0), 0.0, 215), ((140.0, 40.0), 0.0, 175)]),
          ((90, 120), [])]
DET_SIZE = (240, 320)


def rectangle(a, b, centre, angle):
    t = math.radians(angle)
    c, s = math.cos(t), math.sin(t)
    base = np.array([[-a / 2, -b / 2], [a / 2, -b / 2], [a / 2, b / 2], [-a / 2, b / 2]], dtype=np.float64)
    return base @ np.array([[c, s], [-s, c]]) + np.asarray(centre, dtype=np.float64)


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
    return {'binary': (x[:, :1] > 0).float()}


class SpellByBrightness(torch.nn.Module):
    """[M, C, 1, T] scores that spell LEVELS[g], g the grey level nearest to (mean of channel 0 in grey levels) / SHARE, with a
    blank between the symbols.  Counts its calls."""

    def __init__(self, charset, T=16):
        super().__init__()
        self.charset, self.T, self.batches = charset, T, []

    def forward(self, crops):
        self.batches.append(crops.shape[0])
        grey = (crops[:, 0] * 255.0 + RGB_MEAN[0]).mean(dim=(1, 2)).cpu().numpy() / SHARE
        out = torch.zeros((crops.shape[0], len(self.charset), 1, self.T), dtype=torch.float32)
        for m, g in enumerate(grey):
            text = LEVELS[min(LEVELS, key=lambda level: abs(level - g))]
            ids = [0] * self.T
            ids[1:2 * len(text):2] = [self.charset.index(ch) for ch in text]
            out[m, ids, 0, torch.arange(self.T)] = 1.0
        return out.to(crops.device)


def ordered(quad):
    return np.array(mini_box([tuple(p) for p in quad])[0], dtype=np.float64)


def check(results):
    assert len(results) == len(SCENES)
    for found, (shape, rects) in zip(results, SCENES):
        assert len(found) == len(rects)
        left = list(rects)
        for item in found:
            got = ordered(item['quad'])
            dist = [np.abs(got - ordered(rectangle(A + 2 * GROW, B + 2 * GROW, centre, angle))).max() for centre, angle, _ in left]
            k = int(np.argmin(dist))
            print("box at %s: %.2f px from the painted rectangle grown by %.2f" % (left[k][0], dist[k], GROW))
            assert dist[k] < 3.0
            assert item['text'] == LEVELS[left[k][2]]               # the text of ITS box
            del left[k]
    assert results[2] == []


def test_plumbing_with_stubs():
    charset = EnglishCharset()
    recognizer = SpellByBrightness(charset)
    reader = TextReader(detector, recognizer, charset, det_size=DET_SIZE)
    results = reader.read(photos())
    check(results)
    assert recognizer.batches == [4]
    chunked = SpellByBrightness(charset)
    again = TextReader(detector, chunked, charset, det_size=DET_SIZE, max_crops=2).read(photos())
    assert chunked.batches == [2, 2]
    assert again == results
    assert TextReader(detector, recognizer, charset, det_size=DET_SIZE).read([photos()[2]]) == [[]]
    assert reader.read([]) == []


def test_real_recogniser_reads_what_the_steps_by_hand_read():
    from megreader_amd.backbones import crnn_backbone
    from megreader_amd.decoders import CRNNDecoder

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = crnn_backbone()
            self.decoder = CRNNDecoder(in_channels=512)

        def forward(self, x):
            return self.decoder(self.backbone(x))

    torch.manual_seed(0)
    model = Model().cuda().eval()
    charset = EnglishCharset()
    results = TextReader(detector, model, charset, det_size=DET_SIZE, rec_size=(32, 128)).read(photos())
    assert [len(found) for found in results] == [2, 2, 0]
    quads = [[item['quad'] for item in found] for found in results]
    crops = QuadCropper(image_size=(32, 128)).crop(photos(), quads)
    assert crops['index'].cpu().tolist() == [0, 0, 1, 1]
    with torch.no_grad():
        pred = model(crops['image'])
    assert pred.shape[:3] == (4, len(charset), 1)
    ids, lengths = ctc_greedy_decode(pred)
    by_hand = [charset.label_to_string(row[:int(k)]) for row, k in zip(ids.cpu().numpy(), lengths.cpu().numpy())]
    assert [item['text'] for found in results for item in found] == by_hand
