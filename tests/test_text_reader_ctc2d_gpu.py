"""TextReader on a 2D-CTC recogniser (megreader_amd/reader.py): one whose eval output is (classify [M, C, H, W], mask [M, 1, H, W])
with H > 1.  Its posterior is `ctc2d_marginal(classify, mask)`; greedy decoding is `ctc2d_greedy_decode`; the beam, the lexicon by
likelihood and the alignment read the marginal as they read a 1-D head, and with `chars=True` every character's quad spans the band
of heights `ctc2d_char_rows` finds for it.

The scenes and the stub detector are those of tests/test_text_reader_lexicon_gpu.py, the 1-D posteriors those of
tests/test_text_reader_lexicon_ctc_gpu.py (12 columns, H E L in the first three, O or P in column 5, keyed by brightness).  The
2-D stub has H = 4: classify repeats the 1-D posterior on every height, the mask has most of each column's mass on ONE height,
HEIGHTS[w] -- so H, E, L and O lie on the heights 0, 1, 2 and 3."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_text_reader_chars_gpu as chars1d  # noqa: E402
import test_text_reader_lexicon_ctc_gpu as ctc  # noqa: E402
import test_text_reader_lexicon_gpu as base  # noqa: E402
from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.data.quad_crop import plan_crop  # noqa: E402
from megreader_amd.ops.decode import (ctc2d_greedy_decode, ctc2d_marginal, ctc_beam_search_decode,  # noqa: E402
                                      ctc_forced_align)
from megreader_amd.ops.lexicon import Lexicon  # noqa: E402

REC_SIZE = (32, 128)
T, H = ctc.T, 4
HEIGHTS = [0, 1, 2, 2, 2, 3] + [3] * (T - 6)        # the height of every column: H E L (gap) (second L) O, then blanks


def head(y, heights=HEIGHTS):
    """(classify [C, H, T], mask [1, H, T]) from a 1-D posterior y [C, 1, T]."""
    classify = y.expand(y.shape[0], H, T).contiguous()
    mask = torch.full((1, H, T), 0.1)
    for w, h in enumerate(heights):
        mask[0, h, w] = 0.7
    return classify, mask


class Head2DByBrightness(torch.nn.Module):
    """The 2-D head of a crop is table[its grey level]: {level: (classify [C, H, T], mask [1, H, T])}."""

    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, crops):
        grey = (crops[:, 0] * 255.0 + RGB_MEAN[0]).mean(dim=(1, 2)).cpu().numpy() / base.SHARE
        picked = [self.table[min(self.table, key=lambda level: abs(level - g))] for g in grey]
        return (torch.stack([p[0] for p in picked]).to(crops.device), torch.stack([p[1] for p in picked]).to(crops.device))


def reader(charset=None, table=None, **kw):
    charset = charset if charset is not None else EnglishCharset()
    table = table if table is not None else {level: head(ctc.posterior(charset, tail)) for level, tail in ctc.LEVELS.items()}
    kw.setdefault('decode', 'ctc')
    return TextReader(base.detector, Head2DByBrightness(table), charset, det_size=base.DET_SIZE, **kw), table


def marginal(entry):
    """`ctc2d_marginal` of one table entry: [1, C, T] on the device."""
    return ctc2d_marginal(entry[0].unsqueeze(0).to("cuda"), entry[1].unsqueeze(0).to("cuda"))


def direct(entry, ids):
    """One id string aligned to the marginal of one table entry: (begin, end, exp(sym_lp / n)) as lists."""
    tg = torch.tensor([ids], dtype=torch.int32, device="cuda")
    out = ctc_forced_align(marginal(entry), tg, torch.tensor([len(ids)], dtype=torch.int32, device="cuda"))
    assert math.isfinite(float(out['score'][0]))
    begin, end, lp = (out[k][0].cpu().tolist() for k in ('begin', 'end', 'sym_lp'))
    return begin, end, [math.exp(v / (e - b)) for v, b, e in zip(lp, begin, end)]


def check_boxes(item, shape, begin, end, heights=HEIGHTS, row_stride=REC_SIZE[0] / float(H), row_offset=0.0):
    """The quads of item['chars'] are the canvas rectangles [begin * stride, end * stride] x [row_offset + lo * row_stride,
    row_offset + (hi + 1) * row_stride] of the crop carried to the photo, lo and hi the least and greatest height of the
    character's columns: the columns exactly as `check_boxes` of tests/test_text_reader_chars_gpu.py has them, the rows as exactly
    down the crop's other edge; in reading order, neighbours not overlapping, none outside the outline."""
    plan = plan_crop(shape, np.asarray(item['quad'], dtype=np.float64), REC_SIZE, 'resize', 'min_area_rect')
    Hc, Wc = REC_SIZE
    tl, tr, br, bl = plan.canvas_to_photo([[0, 0], [Wc, 0], [Wc, Hc], [0, Hc]])
    along, down = (tr - tl) / np.linalg.norm(tr - tl), (bl - tl) / np.linalg.norm(bl - tl)
    length, depth = float(np.linalg.norm(tr - tl)), float(np.linalg.norm(bl - tl))
    assert np.allclose(br - bl, tr - tl, atol=1e-9) and abs(along @ down) <= 1e-9
    stride = Wc / float(T)
    last = 0.0
    for ch, b, e in zip(item['chars'], begin, end):
        quad = np.asarray(ch['quad'], dtype=np.float64)
        assert quad.shape == (4, 2)
        lo, hi = min(heights[b:e]), max(heights[b:e])
        u0, u1 = b * stride / Wc * length, e * stride / Wc * length
        v0 = min(max(row_offset + lo * row_stride, 0.0), Hc) / Hc * depth
        v1 = min(max(row_offset + (hi + 1) * row_stride, 0.0), Hc) / Hc * depth
        for corner, (u, v) in enumerate(((u0, v0), (u1, v0), (u1, v1), (u0, v1))):
            rel = quad[corner] - tl
            assert abs(rel @ along - u) <= 1e-6 and abs(rel @ down - v) <= 1e-6, (ch['char'], corner, rel @ along, u, rel @ down, v)
        assert -1e-9 <= last <= u0 + 1e-9 and u0 < u1 <= length + 1e-9 and 0.0 <= v0 < v1 <= depth + 1e-9
        last = u1
    return plan


def flat(results, photos):
    return chars1d.flat(results, photos)


def test_greedy_text_is_the_2d_greedy_decode():
    charset = EnglishCharset()
    photos = base.photos()
    rd, table = reader(charset)
    results = rd.read(photos)
    items = flat(results, photos)
    assert len(items) == 4 and results[2] == []
    for item, _ in items:
        assert set(item) == {'quad', 'text'} and item['text'] == "HELO"
    for entry in table.values():                                               # ... which is what ctc2d_greedy_decode says of the head
        ids, lengths = ctc2d_greedy_decode(entry[0].unsqueeze(0).to("cuda"), entry[1].unsqueeze(0).to("cuda"),
                                           blank=charset.blank, unknown=charset.unknown)
        assert charset.label_to_string(ids[0, :int(lengths[0])].cpu().numpy()) == "HELO"
    assert rd.recognize(torch.zeros((0, 3) + REC_SIZE, device="cuda")) == []


@pytest.mark.parametrize("nbest", [1, 3])
def test_beam_text_score_is_the_beam_on_the_marginal(nbest):
    charset = EnglishCharset()
    photos = base.photos()
    rd, table = reader(charset, decode='beam', nbest=nbest)
    known = {}
    for level, entry in table.items():
        out = ctc_beam_search_decode(marginal(entry), beam=8, nbest=nbest, blank=charset.blank, unknown=charset.unknown)
        ids, lengths = out['ids'][0].cpu().numpy(), out['lengths'][0].cpu().numpy()
        known[level] = [(charset.label_to_string(ids[j][:int(lengths[j])]), float(out['scores'][0, j]))
                        for j in range(int(out['count'][0]))]
    items = flat(rd.read(photos), photos)
    assert len(items) == 4
    for item, _ in items:
        match = [level for level, hyps in known.items() if hyps[0] == (item['text'], item['text_score'])]
        assert match, (item, known)
        assert -5.0 < item['text_score'] < 0.0
        if nbest > 1:
            assert item['alternatives'] == known[match[0]]
    assert sorted(item['text'] for item, _ in items) == sorted(hyps[0][0] for hyps in known.values())


def test_lexicon_by_likelihood_reads_the_marginal():
    charset = EnglishCharset()
    photos = base.photos()
    rd, table = reader(charset, lexicon=ctc.WORDS, lexicon_rule='likelihood')
    results = rd.read(photos)
    assert [sorted(item['text'] for item in found) for found in results] == ctc.wanted()
    lex = Lexicon(ctc.WORDS, charset)
    known = {}
    for level, entry in table.items():
        found = lex.transcribe(marginal(entry))
        known[ctc.WORDS[int(found['index'][0])]] = float(found['score'][0])
    for item, _ in flat(results, photos):
        assert set(item) == {'quad', 'text', 'raw_text', 'lexicon_distance', 'lexicon_score'}
        assert item['raw_text'] == "HELO" and item['lexicon_distance'] == 1 and item['lexicon_score'] == known[item['text']]
    nearest = reader(charset, lexicon=ctc.WORDS)[0].read(photos)               # the nearest rule reads the 2-D greedy string
    assert all((item['text'], item['raw_text']) == ("HELP", "HELO") for found in nearest for item in found)


@pytest.mark.parametrize("max_crops", [256, 3])
def test_chars_span_their_band_of_heights(max_crops):
    charset = EnglishCharset()
    photos = base.photos()
    rd, table = reader(charset, chars=True, max_crops=max_crops)
    items = flat(rd.read(photos), photos)
    assert len(items) == 4
    ids = [charset.index(ch) for ch in "HELO"]
    known = {level: direct(table[level], ids) for level in table}
    for item, shape in items:
        assert set(item) == {'quad', 'text', 'chars'} and item['text'] == "HELO"
        assert [ch['char'] for ch in item['chars']] == list("HELO")
        scores = [ch['score'] for ch in item['chars']]
        match = [level for level, (_, _, want) in known.items() if want == scores]   # exp(sym_lp / (end - begin)) on the marginal
        assert match, (scores, known)
        begin, end, _ = known[match[0]]
        assert (begin, end) == ([0, 1, 2, 5], [1, 2, 3, 6])
        check_boxes(item, shape, begin, end)
        # H, E, L, O on the heights 0, 1, 2, 3: four bands of a quarter of the crop, each below the one before
        tops = [np.asarray(ch['quad'])[0] for ch in item['chars']]
        plan = plan_crop(shape, np.asarray(item['quad'], dtype=np.float64), REC_SIZE, 'resize', 'min_area_rect')
        tl, _, _, bl = plan.canvas_to_photo([[0, 0], [REC_SIZE[1], 0], [REC_SIZE[1], REC_SIZE[0]], [0, REC_SIZE[0]]])
        down = (bl - tl) / np.linalg.norm(bl - tl)
        depth = float(np.linalg.norm(bl - tl))
        assert np.allclose([(top - tl) @ down for top in tops], [k * depth / 4 for k in range(4)], atol=1e-6)


def test_chars_of_a_beam_string_a_lexicon_word_and_a_band_of_two_heights():
    charset = EnglishCharset()
    photos = base.photos()
    # likelihood: HELLO (the second L in column 4, height 2) or HELP
    rd, table = reader(charset, chars=True, lexicon=ctc.WORDS, lexicon_rule='likelihood')
    for item, shape in flat(rd.read(photos), photos):
        level = [lv for lv, word in ctc.LIKELY.items() if word == item['text']][0]
        begin, end, scores = direct(table[level], [charset.index(ch) for ch in item['text']])
        assert scores == [ch['score'] for ch in item['chars']]
        assert (begin, end) == (([0, 1, 2, 4, 5], [1, 2, 3, 5, 6]) if item['text'] == "HELLO" else ([0, 1, 2, 5], [1, 2, 3, 6]))
        check_boxes(item, shape, begin, end)
    # the beam's string
    rd, table = reader(charset, chars=True, decode='beam')
    for item, shape in flat(rd.read(photos), photos):
        known = [direct(entry, [charset.index(ch) for ch in item['text']]) for entry in table.values()]
        match = [k for k in known if k[2] == [ch['score'] for ch in item['chars']]]
        assert match and set(item) == {'quad', 'text', 'text_score', 'chars'}
        check_boxes(item, shape, match[0][0], match[0][1])
    # an L of two columns on the heights 2 and 1: its band is both, [1, 3) of 4; and another row geometry
    heights = [0, 1, 2, 1, 3, 3] + [0] * (T - 6)
    y = ctc.posterior(charset, [{'L': 0.9}, {'': 0.9}, {'O': 0.9}])
    table = {level: head(y, heights) for level in ctc.LEVELS}
    for kw, geometry in ((dict(), dict()), (dict(row_geometry=(6.0, 5.0)), dict(row_stride=6.0, row_offset=5.0))):
        rd, _ = reader(charset, table, chars=True, **kw)
        for item, shape in flat(rd.read(photos), photos):
            assert item['text'] == "HELO"
            begin, end, scores = direct(table[135], [charset.index(ch) for ch in "HELO"])
            assert (begin, end) == ([0, 1, 2, 5], [1, 2, 4, 6]) and scores == [ch['score'] for ch in item['chars']]
            check_boxes(item, shape, begin, end, heights, **geometry)
    for bad in ((0.0, 0.0), (-1.0, 0.0), (float('inf'), 0.0), (8.0, float('nan'))):
        with pytest.raises(ValueError, match="row_geometry"):
            reader(charset, table, chars=True, row_geometry=bad)


def test_a_1d_recogniser_reads_as_before():
    charset = EnglishCharset()
    photos = base.photos()
    one_d, table = chars1d.reader(charset, chars=True, row_geometry=(3.0, 1.0))   # (a row geometry means nothing to a 1-D head)
    assert type(one_d) is type(reader(charset)[0])
    results = one_d.read(photos)
    assert results == chars1d.reader(charset, chars=True)[0].read(photos)
    ids = [charset.index(ch) for ch in "HELO"]
    for item, shape in flat(results, photos):
        assert set(item) == {'quad', 'text', 'chars'} and item['text'] == "HELO"
        known = [chars1d.direct(table[level], ids) for level in ctc.LEVELS]
        match = [k for k in known if k[2] == [ch['score'] for ch in item['chars']]]
        assert match
        chars1d.check_boxes(item, shape, match[0][0], match[0][1])             # the whole height of the crop
    # a pair whose first member has one height is a 1-D head still
    class Pair(ctc.PosteriorByBrightness):
        def forward(self, crops):
            post = super().forward(crops)
            return post, torch.ones_like(post[:, :1])

    paired = TextReader(base.detector, Pair(charset), charset, det_size=base.DET_SIZE, decode='ctc', chars=True).read(photos)
    assert paired == results
