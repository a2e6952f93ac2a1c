"""TextReader with `decode='beam'` (megreader_amd/reader.py): the recogniser's CTC posterior goes through
`ctc_beam_search_decode` and an item's 'text' becomes the most probable STRING, with its log-probability in 'text_score' and the
other readings in 'alternatives'.  The scenes, the stub detector and the brightness-keyed stub recogniser are those of
tests/test_text_reader_lexicon_ctc_gpu.py; here every crop gets the posterior whose best path spells HELO while the most probable
string is HELLO: after H, E, L and a confident blank come two columns `blank 0.55 / L 0.40`, then O -- no second L (0.55^2) is
less likely than at least one."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_text_reader_lexicon_ctc_gpu as ctc  # noqa: E402
import test_text_reader_lexicon_gpu as base  # noqa: E402
from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402

TAIL = [{'': 0.9}, {'': 0.55, 'L': 0.4}, {'': 0.55, 'L': 0.4}, {'O': 0.9}]
BEST_ALIGNMENT = 0.9 ** 5 * 0.4 * 0.55            # H E L - L - O: the likeliest single path that spells HELLO (before the floor)


class Hello(ctc.PosteriorByBrightness):
    def __init__(self, charset):
        torch.nn.Module.__init__(self)
        self.table = {level: ctc.posterior(charset, TAIL) for level in ctc.LEVELS}


def reader(**kw):
    charset = EnglishCharset()
    return TextReader(base.detector, Hello(charset), charset, det_size=base.DET_SIZE, **kw)


def items_of(results):
    assert len(results) == len(base.SCENES) and results[2] == []
    items = [item for found in results for item in found]
    assert len(items) == 4
    return items


def test_greedy_is_unchanged():
    for item in items_of(reader(decode='ctc').read(base.photos())):
        assert set(item) == {'quad', 'text'} and item['text'] == "HELO"
    for item in items_of(reader(decode='ctc', scores=True, lexicon=ctc.WORDS).read(base.photos())):
        assert set(item) == {'quad', 'text', 'raw_text', 'lexicon_distance', 'score'} and item['raw_text'] == "HELO"


def test_beam_returns_the_most_probable_string_with_its_score():
    for kw in (dict(), dict(max_crops=3), dict(max_crops=1), dict(beam_width=4, beam_top_classes=3)):
        for item in items_of(reader(decode='beam', **kw).read(base.photos())):
            assert set(item) == {'quad', 'text', 'text_score'}
            assert item['text'] == "HELLO"
            assert isinstance(item['text_score'], float) and math.log(BEST_ALIGNMENT) < item['text_score'] < 0.0


def test_alternatives():
    greedy = [item['quad'] for item in items_of(reader(decode='ctc').read(base.photos()))]
    for kw in (dict(), dict(max_crops=3)):
        found = items_of(reader(decode='beam', nbest=3, **kw).read(base.photos()))
        assert [item['quad'] for item in found] == greedy
        for item in found:
            assert set(item) == {'quad', 'text', 'text_score', 'alternatives'}
            alt = item['alternatives']
            assert len(alt) == 3 and alt[0] == (item['text'], item['text_score']) and alt[0][0] == "HELLO"
            assert all(isinstance(t, str) and isinstance(s, float) for t, s in alt)
            assert alt[0][1] > alt[1][1] > alt[2][1]
            assert "HELO" in [t for t, _ in alt] and len({t for t, _ in alt}) == 3


def test_scores_compose():
    plain = items_of(reader(decode='beam', scores=True).read(base.photos()))
    want = items_of(reader(decode='ctc', scores=True).read(base.photos()))
    for item, other in zip(plain, want):
        assert set(item) == {'quad', 'text', 'text_score', 'score'}
        assert item['score'] == other['score'] and item['quad'] == other['quad'] and item['text'] == "HELLO"


def test_nearest_lexicon_word_of_the_beam_string():
    for item in items_of(reader(decode='beam', lexicon=ctc.WORDS).read(base.photos())):           # ["HELP", "HELLO"]
        assert set(item) == {'quad', 'text', 'raw_text', 'lexicon_distance', 'text_score'}
        assert (item['text'], item['raw_text'], item['lexicon_distance']) == ("HELLO", "HELLO", 0)
    for item in items_of(reader(decode='beam', lexicon=["HELP", "JELLO"], nbest=2).read(base.photos())):
        assert (item['text'], item['raw_text'], item['lexicon_distance']) == ("JELLO", "HELLO", 1)
        assert item['alternatives'][0][0] == "HELLO"


def test_likelihood_keeps_requiring_greedy_decoding():
    charset = EnglishCharset()
    with pytest.raises(ValueError, match="needs decode='ctc'"):
        TextReader(base.detector, Hello(charset), charset, decode='beam', lexicon=ctc.WORDS, lexicon_rule='likelihood')
    with pytest.raises(ValueError, match="beam_width"):
        reader(decode='beam', beam_width=2, nbest=3)


def test_a_dead_beam_gives_an_empty_reading():
    class Dead(Hello):
        def forward(self, crops):
            y = super().forward(crops).clone()
            y[:, :, :, 5] = 0.0
            y[:, 1, :, 5] = 1.0                          # one column with all its mass on `unknown`
            return y
    charset = EnglishCharset()
    found = TextReader(base.detector, Dead(charset), charset, det_size=base.DET_SIZE, decode='beam', nbest=2).read(base.photos())
    for item in items_of(found):
        assert (item['text'], item['text_score'], item['alternatives']) == ('', -math.inf, [])
