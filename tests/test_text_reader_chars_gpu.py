"""TextReader with `chars=True` (megreader_amd/reader.py): the final text of every crop -- greedy, beam or lexicon word -- is aligned
to the recogniser's CTC posterior by `ctc_forced_align` and every item carries 'chars', one {'char', 'quad', 'score'} per
character.  The scenes, the stub detector and the brightness-keyed stub recogniser are those of
tests/test_text_reader_lexicon_ctc_gpu.py: 12 columns, H E L in the first three, O (or P) in column 5."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_text_reader_lexicon_ctc_gpu as ctc  # noqa: E402
import test_text_reader_lexicon_gpu as base  # noqa: E402
from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset, EnglishPrintableCharset  # noqa: E402
from megreader_amd.data.quad_crop import plan_crop  # noqa: E402
from megreader_amd.ops.decode import ctc_forced_align  # noqa: E402

REC_SIZE = (32, 128)
T = ctc.T


class ByLevel(ctc.PosteriorByBrightness):
    """The posterior of a crop is table[its grey level]: {level: [C, 1, T]}."""

    def __init__(self, table):
        torch.nn.Module.__init__(self)
        self.table = table


def reader(charset=None, table=None, **kw):
    charset = charset if charset is not None else EnglishCharset()
    table = table if table is not None else {level: ctc.posterior(charset, tail) for level, tail in ctc.LEVELS.items()}
    kw.setdefault('decode', 'ctc')
    return TextReader(base.detector, ByLevel(table), charset, det_size=base.DET_SIZE, **kw), table


def flat(results, photos):
    """[(item, shape of its photo)]"""
    return [(item, photo.shape) for found, photo in zip(results, photos) for item in found]


def direct(post, ids):
    """`ctc_forced_align` of one id string on one posterior [C, 1, T]: (begin, end, exp(sym_lp / n)) as lists."""
    tg = torch.tensor([ids], dtype=torch.int32, device="cuda")
    out = ctc_forced_align(post.unsqueeze(0).to("cuda"), tg, torch.tensor([len(ids)], dtype=torch.int32, device="cuda"))
    assert math.isfinite(float(out['score'][0]))
    begin, end, lp = (out[k][0].cpu().tolist() for k in ('begin', 'end', 'sym_lp'))
    return begin, end, [math.exp(v / (e - b)) for v, b, e in zip(lp, begin, end)]


def check_boxes(item, shape, begin, end, stride=REC_SIZE[1] / float(T), offset=0.0):
    """The quads of item['chars'] are the canvas rectangles [offset + begin * stride, offset + end * stride] x [0, H] of the
    crop, carried to the photo: corners on the top and bottom edge of the crop's outline at those abscissae, in reading order,
    neighbours not overlapping, none outside the outline."""
    plan = plan_crop(shape, np.asarray(item['quad'], dtype=np.float64), REC_SIZE, 'resize', 'min_area_rect')
    H, W = REC_SIZE
    tl, tr, br, bl = plan.canvas_to_photo([[0, 0], [W, 0], [W, H], [0, H]])
    along = (tr - tl) / np.linalg.norm(tr - tl)
    length = float(np.linalg.norm(tr - tl))
    assert np.allclose(br - bl, tr - tl, atol=1e-9)                            # (min_area_rect: the outline is a rectangle)
    last = 0.0
    for ch, b, e in zip(item['chars'], begin, end):
        quad = np.asarray(ch['quad'], dtype=np.float64)
        assert quad.shape == (4, 2)
        u0 = min(max(offset + b * stride, 0.0), W) / W * length
        u1 = min(max(offset + e * stride, 0.0), W) / W * length
        for corner, origin, want in ((0, tl, u0), (1, tl, u1), (2, bl, u1), (3, bl, u0)):
            rel = quad[corner] - origin
            assert abs(rel @ along - want) <= 1e-6, (ch['char'], corner)
            assert abs(rel[0] * along[1] - rel[1] * along[0]) <= 1e-6, (ch['char'], corner)     # on that edge
        assert -1e-9 <= last <= u0 + 1e-9 and u0 < u1 <= length + 1e-9
        last = u1
    return plan


def test_greedy_text():
    charset = EnglishCharset()
    photos = base.photos()
    rd, table = reader(charset, chars=True)
    results = rd.read(photos)
    items = flat(results, photos)
    assert len(items) == 4 and results[2] == []
    ids = [charset.index(ch) for ch in "HELO"]
    known = {level: direct(table[level], ids) for level in ctc.LEVELS}
    for item, shape in items:
        assert set(item) == {'quad', 'text', 'chars'} and item['text'] == "HELO"
        assert [ch['char'] for ch in item['chars']] == list(item['text'])
        assert all(set(ch) == {'char', 'quad', 'score'} for ch in item['chars'])
        scores = [ch['score'] for ch in item['chars']]
        match = [level for level, (_, _, want) in known.items() if want == scores]
        assert match, (scores, known)
        begin, end, _ = known[match[0]]
        assert (begin, end) == ([0, 1, 2, 5], [1, 2, 3, 6])
        assert all(0.0 < s <= 1.0 for s in scores) and abs(scores[0] - float(table[match[0]][charset.index('H'), 0, 0])) < 1e-6
        check_boxes(item, shape, begin, end)


def test_chars_false_is_today():
    photos = base.photos()
    plain = reader()[0].read(photos)
    assert plain == reader(chars=False)[0].read(photos)
    assert all('chars' not in item for found in plain for item in found)
    with_chars = reader(chars=True, scores=True)[0].read(photos)
    without = reader(scores=True)[0].read(photos)
    assert [[{k: v for k, v in item.items() if k != 'chars'} for item in found] for found in with_chars] == without


@pytest.mark.parametrize("max_crops", [256, 3, 1])
def test_lexicon_words_are_what_is_aligned(max_crops):
    charset = EnglishCharset()
    photos = base.photos()
    # nearest: HELP for every crop (the first listed of the two at distance 1), although O is what the posterior shows
    rd, table = reader(charset, chars=True, lexicon=ctc.WORDS, max_crops=max_crops)
    for item, shape in flat(rd.read(photos), photos):
        assert (item['text'], item['raw_text']) == ("HELP", "HELO")
        assert [ch['char'] for ch in item['chars']] == list("HELP")
        known = [direct(table[level], [charset.index(ch) for ch in "HELP"]) for level in ctc.LEVELS]
        match = [k for k in known if k[2] == [ch['score'] for ch in item['chars']]]
        assert match
        check_boxes(item, shape, match[0][0], match[0][1])
    # likelihood: HELLO or HELP by the crop's posterior
    rd, table = reader(charset, chars=True, lexicon=ctc.WORDS, lexicon_rule='likelihood', max_crops=max_crops)
    results = rd.read(photos)
    assert [sorted(item['text'] for item in found) for found in results] == ctc.wanted()
    for item, shape in flat(results, photos):
        assert item['raw_text'] == "HELO" and [ch['char'] for ch in item['chars']] == list(item['text'])
        level = [lv for lv, word in ctc.LIKELY.items() if word == item['text']][0]
        begin, end, scores = direct(table[level], [charset.index(ch) for ch in item['text']])
        assert scores == [ch['score'] for ch in item['chars']]
        assert (begin, end) == (([0, 1, 2, 4, 5], [1, 2, 3, 5, 6]) if item['text'] == "HELLO" else ([0, 1, 2, 5], [1, 2, 3, 6]))
        check_boxes(item, shape, begin, end)


def test_folded_lexicon_word_beside_raw_strings():
    """A case-sensitive charset: the lexicon word "helo" is compared and aligned over the folded alphabet, where O and o are one
    class (0.5 + 0.4); the crops that keep their raw string "HELP" are aligned to the posterior as it is.  Both kinds share a
    chunk."""
    charset = EnglishPrintableCharset(case_sensitive=True)
    helo = [{'': 0.9}, {'': 0.97}, {'O': 0.5, 'o': 0.4}]
    help_ = [{'': 0.9}, {'': 0.97}, {'P': 0.9}]
    table = {135: ctc.posterior(charset, helo), 175: ctc.posterior(charset, help_),
             215: ctc.posterior(charset, helo), 255: ctc.posterior(charset, help_)}
    photos = base.photos()
    rd, _ = reader(charset, table, chars=True, lexicon=["helo"], lexicon_max_distance=0)
    items = flat(rd.read(photos), photos)
    assert sorted(item['text'] for item, _ in items) == ["HELP", "HELP", "helo", "helo"]
    for item, shape in items:
        assert [ch['char'] for ch in item['chars']] == list(item['text'])
        last = item['chars'][-1]['score']
        if item['text'] == "helo":
            assert item['raw_text'] == "HELO" and 0.98 < last < 1.0            # O + o: (0.5 + 0.4) / 0.91
            fold = rd.lexicon._tensors(torch.device("cuda", 0))[2]
            folded = rd.lexicon._folded(table[135].unsqueeze(0).to("cuda").select(2, 0), fold, False)
            ids, lengths = rd.lexicon.ids(torch.tensor([0], device="cuda"))
            assert lengths.tolist() == [4] and ids.dtype == torch.int32 and ids.shape == (1, 4)
            begin, end, scores = direct(folded[0].unsqueeze(1), ids[0].tolist())
        else:
            assert 0.98 < last < 1.0
            begin, end, scores = direct(table[175], [charset.index(ch) for ch in "HELP"])
        assert scores == [ch['score'] for ch in item['chars']]
        check_boxes(item, shape, begin, end)
    # ... and the raw O alone is 0.5 / 0.91 where no word is taken
    rd, _ = reader(charset, table, chars=True)
    lows = [item['chars'][-1]['score'] for item, _ in flat(rd.read(photos), photos) if item['text'] == "HELO"]
    assert len(lows) == 2 and all(0.53 < s < 0.57 for s in lows)


def test_lexicon_ids():
    lexicon = reader(lexicon=["TEXT", "A", "", "HELLO"])[0].lexicon
    ids, lengths = lexicon.ids(torch.tensor([3, -1, 0, 2, 1], device="cuda"))
    assert ids.is_cuda and lengths.is_cuda and ids.dtype == lengths.dtype == torch.int32
    assert lengths.tolist() == [5, 0, 4, 0, 1] and ids.shape == (5, 5)
    charset = lexicon.charset
    assert ids.tolist() == [[charset.index(ch) for ch in word] + [lexicon.blank] * (5 - len(word))
                            for word in ("HELLO", "", "TEXT", "", "A")]


def test_beam_text():
    import test_text_reader_beam_gpu as beam
    charset = EnglishCharset()
    photos = base.photos()
    rd = TextReader(base.detector, beam.Hello(charset), charset, det_size=base.DET_SIZE, decode='beam', chars=True)
    begin, end, scores = direct(ctc.posterior(charset, beam.TAIL), [charset.index(ch) for ch in "HELLO"])
    assert len(begin) == 5
    for item, shape in flat(rd.read(photos), photos):
        assert set(item) == {'quad', 'text', 'text_score', 'chars'} and item['text'] == "HELLO"
        assert [ch['char'] for ch in item['chars']] == list("HELLO") and [ch['score'] for ch in item['chars']] == scores
        check_boxes(item, shape, begin, end)


def test_column_geometry():
    photos = base.photos()
    rd, table = reader(chars=True, column_geometry=(4.0, -2.0))                # the CRNN's: a column every 4 pixels
    charset = rd.charset
    for item, shape in flat(rd.read(photos), photos):
        begin, end, _ = direct(table[135], [charset.index(ch) for ch in "HELO"])
        check_boxes(item, shape, begin, end, stride=4.0, offset=-2.0)


def test_vertical_crop_gives_stacked_boxes():
    photo = np.zeros((150, 200, 3), dtype=np.uint8)
    photo[40:101, 90:111] = 175                                                # the rectangle of the scenes on end: 21 wide, 61 tall
    rd, table = reader(chars=True)
    results = rd.read([photo])
    assert len(results) == 1 and len(results[0]) == 1
    item = results[0][0]
    assert item['text'] == "HELO" and len(item['chars']) == 4
    begin, end, _ = direct(table[175], [rd.charset.index(ch) for ch in "HELO"])
    plan = check_boxes(item, photo.shape, begin, end)
    assert plan.rotated
    centres = [np.asarray(ch['quad']).mean(axis=0) for ch in item['chars']]
    for a, b in zip(centres, centres[1:]):
        assert b[1] > a[1] and abs(b[0] - a[0]) <= 0.1 * (b[1] - a[1])         # down the photo, not across


def test_a_word_longer_than_the_posterior_has_no_chars():
    photos = base.photos()
    rd, _ = reader(chars=True, lexicon=["A" * 13])
    items = flat(rd.read(photos), photos)
    assert len(items) == 4
    for item, _ in items:
        assert item['text'] == "A" * 13 and item['raw_text'] == "HELO" and item['chars'] is None
