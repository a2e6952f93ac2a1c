"""TextReader with a lexicon (megreader_amd/reader.py): the recognised ids go through `Lexicon.nearest` on the device and an item's
'text' becomes the nearest lexicon word.  Stub models as in tests/test_text_reader_gpu.py: the detector marks every bright pixel,
the recogniser answers the ids of a string chosen by the crop's mean brightness (`decode='ids'`)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.ops.lexicon import Lexicon  # noqa: E402

A, B = 60.0, 20.0                                   # every painted rectangle: the crops then hold the same share of bright pixels
GROW = 1.5 * A * B / (2.0 * (A + B))                # the representer's unclip distance
SHARE = A * B / ((A + 2 * GROW) * (B + 2 * GROW))   # bright share of an unclipped box
LEVELS = {135: "AB12", 175: "HELO", 215: "X9", 255: "TEXT"}          # what the recogniser spells: two of them misspelt
WORDS = ["TEXT", "HELLO", "AB13", "AB72", "WORLD"]
NEAREST = {"AB12": ("AB13", 1), "HELO": ("HELLO", 1), "X9": ("TEXT", 3), "TEXT": ("TEXT", 0)}   # lowest index on the AB13 / AB72 tie
SCENES = [((120, 160), [((50.0, 30.0), 0.0, 135), ((100.0, 85.0), 20.0, 255)]),
          ((150, 200), [((60.0, 110.0), 0.0, 215), ((140.0, 40.0), 0.0, 175)]),
          ((90, 120), [])]
DET_SIZE = (240, 320)


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


class IdsByBrightness(torch.nn.Module):
    """i32 [M, T] ids that spell LEVELS[g], g the grey level nearest to (mean of channel 0 in grey levels) / SHARE, with a blank
    between the symbols."""

    def __init__(self, charset, T=16):
        super().__init__()
        self.charset, self.T = charset, T

    def forward(self, crops):
        grey = (crops[:, 0] * 255.0 + RGB_MEAN[0]).mean(dim=(1, 2)).cpu().numpy() / SHARE
        out = torch.zeros((crops.shape[0], self.T), dtype=torch.int32)
        for m, g in enumerate(grey):
            text = LEVELS[min(LEVELS, key=lambda level: abs(level - g))]
            out[m, 1:2 * len(text):2] = torch.tensor([self.charset.index(ch) for ch in text], dtype=torch.int32)
        return out.to(crops.device)


def raw_texts():
    """The strings the recogniser spells, per photo, as a sorted list (the representer's box order is its own)."""
    return [sorted(LEVELS[level] for _, _, level in rects) for _, rects in SCENES]


def reader(**kw):
    charset = EnglishCharset()
    return TextReader(detector, IdsByBrightness(charset), charset, det_size=DET_SIZE, decode='ids', **kw)


def test_without_a_lexicon_items_keep_their_keys():
    results = reader().read(photos())
    assert [sorted(item['text'] for item in found) for found in results] == raw_texts()
    assert all(set(item) == {'quad', 'text'} for found in results for item in found)


@pytest.mark.parametrize("lexicon", ["words", "object"])
def test_text_becomes_the_nearest_word(lexicon):
    given = WORDS if lexicon == "words" else Lexicon(WORDS, EnglishCharset())
    for kw in (dict(), dict(max_crops=3)):                         # one chunk, and two chunks of crops
        results = reader(lexicon=given, **kw).read(photos())
        assert [sorted(item['raw_text'] for item in found) for found in results] == raw_texts()
        assert results[2] == []
        for item in (item for found in results for item in found):
            assert set(item) == {'quad', 'text', 'raw_text', 'lexicon_distance'}
            assert (item['text'], item['lexicon_distance']) == NEAREST[item['raw_text']]


def test_max_distance_keeps_misspelt_predictions_raw():
    results = reader(lexicon=WORDS, lexicon_max_distance=0).read(photos())
    items = [item for found in results for item in found]
    assert sorted(item['raw_text'] for item in items) == sorted(LEVELS.values())
    for item in items:
        assert item['text'] == item['raw_text']                    # the one exact word is itself, the others stay as read
        assert item['lexicon_distance'] == NEAREST[item['raw_text']][1]
    within_one = [item for found in reader(lexicon=WORDS, lexicon_max_distance=1).read(photos()) for item in found]
    assert sorted(item['text'] for item in within_one) == sorted(["AB13", "HELLO", "X9", "TEXT"])


def test_scores_and_the_other_decoders_keep_working():
    charset = EnglishCharset()

    class Scores(IdsByBrightness):                                 # [M, C, 1, T] scores for decode='ctc'
        def forward(self, crops):
            ids = super().forward(crops).long()
            return torch.nn.functional.one_hot(ids, len(self.charset)).permute(0, 2, 1).unsqueeze(2).float()

    ctc = TextReader(detector, Scores(charset), charset, det_size=DET_SIZE, decode='ctc', lexicon=WORDS, scores=True)
    by_call = TextReader(detector, IdsByBrightness(charset), charset, det_size=DET_SIZE, lexicon=WORDS,
                         decode=lambda ids: (ids, torch.full((ids.shape[0],), 5, dtype=torch.int32, device=ids.device)))
    for item in (item for found in ctc.read(photos()) for item in found):
        assert set(item) == {'quad', 'text', 'raw_text', 'lexicon_distance', 'score'}
        assert (item['text'], item['lexicon_distance']) == NEAREST[item['raw_text']]
    # a callable that reports 5 valid ids per row: the reader, and the lexicon with it, sees only the first 2 symbols (5 ids)
    cut = {"AB": ("AB13", 2), "HE": ("TEXT", 3), "X9": ("TEXT", 3), "TE": ("TEXT", 2)}
    for item in (item for found in by_call.read(photos()) for item in found):
        assert (item['text'], item['lexicon_distance']) == cut[item['raw_text']]
