"""TextReader with `lexicon_rule='likelihood'` (megreader_amd/reader.py): the recogniser's CTC posterior goes through
`Lexicon.transcribe` on the device and an item's 'text' becomes the most probable lexicon word.  The scenes, the stub detector and
the brightness rule are those of tests/test_text_reader_lexicon_gpu.py; the stub recogniser here answers [M, C, 1, T] posteriors
whose arg-max path spells HELO, with the rest of the mass on a second L (HELLO) or on P in O's column (HELP)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_text_reader_lexicon_gpu as base  # noqa: E402
from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.ops.lexicon import Lexicon  # noqa: E402

WORDS = ["HELP", "HELLO"]                             # both one edit from HELO: `nearest` takes the first listed
T = 12
# grey level of the painted rectangle -> the columns after H, E, L: {character or '' (blank): probability}
LEVELS = {135: [{'': 0.9}, {'': 0.55, 'L': 0.4}, {'O': 0.9}],            # a second L in the gap: HELLO
          175: [{'': 0.9}, {'': 0.97}, {'O': 0.5, 'P': 0.45}],           # P beside O: HELP
          215: [{'': 0.9}, {'': 0.55, 'L': 0.4}, {'O': 0.9}],
          255: [{'': 0.9}, {'': 0.97}, {'O': 0.5, 'P': 0.45}]}
LIKELY = {135: "HELLO", 175: "HELP", 215: "HELLO", 255: "HELP"}


def posterior(charset, tail):
    C = len(charset)
    y = np.full((T, C), 1e-4)
    for t, column in enumerate([{'H': 0.9}, {'E': 0.9}, {'L': 0.9}] + tail + [{'': 1.0}] * (T - 3 - len(tail))):
        for ch, p in column.items():
            y[t, getattr(charset, 'blank', 0) if ch == '' else charset.index(ch)] += p
    y /= y.sum(axis=1, keepdims=True)
    return torch.from_numpy(y.T.astype(np.float32)).reshape(C, 1, T)


class PosteriorByBrightness(torch.nn.Module):
    def __init__(self, charset):
        super().__init__()
        self.table = {level: posterior(charset, tail) for level, tail in LEVELS.items()}

    def forward(self, crops):
        grey = (crops[:, 0] * 255.0 + RGB_MEAN[0]).mean(dim=(1, 2)).cpu().numpy() / base.SHARE
        return torch.stack([self.table[min(LEVELS, key=lambda level: abs(level - g))] for g in grey]).to(crops.device)


def reader(**kw):
    charset = EnglishCharset()
    return TextReader(base.detector, PosteriorByBrightness(charset), charset, det_size=base.DET_SIZE, decode='ctc', **kw)


def wanted():
    """The likely words per photo, sorted (the representer's box order is its own)."""
    return [sorted(LIKELY[level] for _, _, level in rects) for _, rects in base.SCENES]


def test_nearest_is_the_default_and_unchanged():
    for kw in (dict(), dict(lexicon_rule='nearest')):
        results = reader(lexicon=WORDS, **kw).read(base.photos())
        items = [item for found in results for item in found]
        assert len(items) == 4 and results[2] == []
        for item in items:
            assert set(item) == {'quad', 'text', 'raw_text', 'lexicon_distance'}
            assert (item['text'], item['raw_text'], item['lexicon_distance']) == ("HELP", "HELO", 1)


@pytest.mark.parametrize("lexicon", ["words", "object"])
def test_likelihood_returns_the_more_probable_word_with_its_score(lexicon):
    given = WORDS if lexicon == "words" else Lexicon(WORDS, EnglishCharset())
    for kw in (dict(), dict(max_crops=3), dict(lexicon_max_distance=1), dict(scores=True)):
        results = reader(lexicon=given, lexicon_rule='likelihood', **kw).read(base.photos())
        assert [sorted(item['text'] for item in found) for found in results] == wanted()
        for item in (item for found in results for item in found):
            assert set(item) == {'quad', 'text', 'raw_text', 'lexicon_distance', 'lexicon_score'} | ({'score'} if 'scores' in kw else set())
            assert item['raw_text'] == "HELO" and item['lexicon_distance'] == 1
            # the word's probability is below 1 and not below its best single path: 0.9^4 * 0.4 * 0.9 resp. 0.9^4 * 0.97 * 0.45,
            # less the floor's share of each column (under 1 % each over 12 columns)
            best_path = 0.9 ** 4 * (0.4 * 0.9 if item['text'] == "HELLO" else 0.97 * 0.45)
            assert isinstance(item['lexicon_score'], float) and math.log(best_path * 0.99 ** 12) < item['lexicon_score'] < 0.0


def test_likelihood_needs_the_ctc_posterior():
    charset = EnglishCharset()
    for decode in ('ids', lambda pred: (pred, None)):
        with pytest.raises(ValueError, match="likelihood"):
            TextReader(base.detector, PosteriorByBrightness(charset), charset, decode=decode, lexicon=WORDS,
                       lexicon_rule='likelihood')
    with pytest.raises(ValueError, match="lexicon_rule"):
        TextReader(base.detector, PosteriorByBrightness(charset), charset, lexicon=WORDS, lexicon_rule='posterior')
    TextReader(base.detector, PosteriorByBrightness(charset), charset, decode='ids', lexicon=WORDS)      # 'nearest' takes ids


def test_no_possible_word_keeps_the_raw_text():
    for kw in (dict(lexicon=WORDS, lexicon_max_distance=0),       # HELO is no member
               dict(lexicon=[]),                                   # an empty lexicon
               dict(lexicon=["A" * 13, "HELO?"])):                 # 13 symbols do not fit 12 columns; '?' is outside the alphabet
        results = reader(lexicon_rule='likelihood', **kw).read(base.photos())
        items = [item for found in results for item in found]
        assert len(items) == 4
        for item in items:
            assert (item['text'], item['raw_text'], item['lexicon_distance']) == ("HELO", "HELO", -1)
            assert item['lexicon_score'] == -math.inf
    assert reader(lexicon=WORDS, lexicon_rule='likelihood').read([]) == []            # an empty call
    blank_photo = [np.zeros((60, 80, 3), dtype=np.uint8)]
    assert reader(lexicon=WORDS, lexicon_rule='likelihood').read(blank_photo) == [[]]  # a photo without boxes
