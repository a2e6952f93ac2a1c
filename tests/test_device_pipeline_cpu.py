"""CPU: the host half of megreader_amd.data.device_pipeline.  `charset_table` (what mr_encode_labels searches) against
`charset.index(chr(cp))` for EVERY codepoint outside the surrogates -- case folding included: a case-insensitive charset maps
a codepoint to the class of its upper case, never to a lower-case class of its own -- and `target_width` against the
expression of oracle/pipeline.py (resize_image.py:40-48)."""
import string

import numpy as np
import pytest

from megreader_amd import charsets
from megreader_amd.data.device_pipeline import charset_table, target_width

CODEPOINTS = [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF]


def mixed_charset(**kwargs):
    """5 360 classes: the 5 348 ideographs from U+4E00 on (as tests/test_crnn_wide_gpu.py builds its alphabet) plus Latin and
    Greek letters of both cases and the micro sign, whose upper case is the Greek capital MU (not a class here)."""
    cs = charsets.Charset([chr(0x4E00 + i) for i in range(5348)] + list("abcXYZΑΒΣµ"), **kwargs)
    assert len(cs) == 5360
    return cs


def _chinese(tmp_path, monkeypatch, **kwargs):
    (tmp_path / "assets").mkdir(exist_ok=True)
    (tmp_path / "assets" / "chinese_charset.dic").write_text("文a中A文zßσΣǆ0-\n", encoding="utf-8")
    monkeypatch.chdir(tmp_path)
    return charsets.ChineseCharset(**kwargs)


CHARSETS = {
    "english": lambda tmp_path, monkeypatch: charsets.EnglishCharset(),
    "printable": lambda tmp_path, monkeypatch: charsets.EnglishPrintableCharset(),
    "printable_case_sensitive": lambda tmp_path, monkeypatch: charsets.EnglishPrintableCharset(case_sensitive=True),
    "mixed_5360": lambda tmp_path, monkeypatch: mixed_charset(),
    "mixed_5360_case_sensitive": lambda tmp_path, monkeypatch: mixed_charset(case_sensitive=True),
    "greek_latin": lambda tmp_path, monkeypatch: charsets.Charset("ΑΒΓΜΣ0123KS"),
    "chinese": lambda tmp_path, monkeypatch: _chinese(tmp_path, monkeypatch),
    "chinese_case_sensitive": lambda tmp_path, monkeypatch: _chinese(tmp_path, monkeypatch, case_sensitive=True),
}


@pytest.mark.parametrize("name", sorted(CHARSETS))
def test_charset_table_equals_index_on_every_codepoint(name, tmp_path, monkeypatch):
    cs = CHARSETS[name](tmp_path, monkeypatch)
    cps, ids = charset_table(cs)
    assert cps.dtype == np.int32 and ids.dtype == np.int32 and cps.shape == ids.shape
    assert np.all(np.diff(cps) > 0)                      # strictly increasing: the kernel searches it by bisection
    assert not np.any(ids == cs.unknown)                 # a missing entry IS `unknown`; none is stored
    lut = dict(zip(cps.tolist(), ids.tolist()))
    index, unknown = cs.index, cs.unknown
    wrong = [cp for cp in CODEPOINTS if lut.get(cp, unknown) != index(chr(cp))]
    assert not wrong, "%d mismatches, e.g. %s" % (
        len(wrong), ["%r: want %d, got %d" % (chr(cp), index(chr(cp)), lut.get(cp, unknown)) for cp in wrong[:8]])


def test_charset_table_folding_examples():
    """the rows of the table that differ between `index` and a table seeded with every class: lower-case classes are never
    targets, and the upper-casing of Unicode is not the inverse of its lower-casing (dotless i, long s, micro sign, final sigma)"""
    p = charsets.EnglishPrintableCharset()
    lut = dict(zip(*(a.tolist() for a in charset_table(p))))
    for lo, up in zip(string.ascii_lowercase, string.ascii_uppercase):
        assert lut[ord(lo)] == lut[ord(up)] == p.index(up) == p.index(lo)
    assert lut[ord("ı")] == p.index("I") and lut[ord("ſ")] == p.index("S")
    assert sorted(set(lut.values())) == [i for i in range(2, len(p)) if p[i].upper() == p[i]]
    s = charsets.EnglishPrintableCharset(case_sensitive=True)
    lut = dict(zip(*(a.tolist() for a in charset_table(s))))
    assert lut == {ord(s[i]): i for i in range(2, len(s))}
    g = charsets.Charset("ΑΒΓΜΣ0123KS")
    lut = dict(zip(*(a.tolist() for a in charset_table(g))))
    assert lut[ord("µ")] == lut[ord("μ")] == g.index("Μ") and lut[ord("ς")] == lut[ord("σ")] == g.index("Σ")
    assert lut[ord("ϐ")] == g.index("Β") and lut[ord("ſ")] == g.index("S") and lut[ord("K")] == g.index("K")
    assert ord("ß") not in lut                           # 'ß'.upper() is two characters: never a class


class _Duck(object):
    """what charset_table may rely on: len, __getitem__, `case_sensitive` (absent = insensitive)"""

    def __init__(self, entries, **attrs):
        self.entries = entries
        self.__dict__.update(attrs)

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, i):
        return self.entries[i]


def test_charset_table_duck_typing():
    entries = [None, None, "<eos>", "A", "b", "é", "É", ""]
    cps, ids = charset_table(_Duck(entries))
    assert dict(zip(cps.tolist(), ids.tolist())) == {ord("A"): 3, ord("a"): 3, ord("É"): 6, ord("é"): 6}
    cps, ids = charset_table(_Duck(entries, case_sensitive=True))
    assert dict(zip(cps.tolist(), ids.tolist())) == {ord("A"): 3, ord("b"): 4, ord("é"): 5, ord("É"): 6}
    cps, ids = charset_table(_Duck([None, None]))
    assert cps.shape == ids.shape == (0,) and cps.dtype == ids.dtype == np.int32


def _oracle_width(mode, image_size, shape):
    """the width expression of oracle/pipeline.py process_sample (mode 'pad') / the canvas width (mode 'resize')"""
    height, width = image_size
    if mode == 'pad':
        return min(width, max(int(height / shape[0] * shape[1] / 32 + 0.5) * 32, 32))
    return width


@pytest.mark.parametrize("image_size", [(32, 128), (48, 160), (64, 256)])
def test_target_width_equals_the_oracle(image_size):
    height, width = image_size
    shapes = [(1, 1), (1, 50), (50, 1), (2, 2), (32, 77), (100, 5), (3, 400), (255, 1000), (1000, 3), (height, width),
              (height, width - 1), (height, 16), (height, 15), (height, 47), (height, 48), (height, 49), (height, 10 * width),
              (2 * height, 2 * width - 33), (31, 100), (17, 300), (7, 7)]
    for shape in shapes:
        assert target_width('resize', image_size, shape) == width
        assert target_width('pad', image_size, shape) == _oracle_width('pad', image_size, shape), shape
    # the 32 floor (tall), the canvas-width cap (very wide), and a value strictly between them (a multiple of 32)
    assert target_width('pad', image_size, (1000, 3)) == 32
    assert target_width('pad', image_size, (3, 400)) == width
    assert target_width('pad', image_size, (height, 48)) == 64 and target_width('pad', image_size, (height, 47)) == 32
    assert target_width('pad', image_size, (height, 15)) == 32      # rounds to 0 columns: the floor, not the rounding


def test_target_width_agrees_with_process_sample():
    """the width the kernel is told to fill is the width oracle.pipeline.process_sample pastes: columns beyond it keep the value
    of a zero pixel, columns inside it do not (a white source)"""
    from oracle.pipeline import process_sample
    zero = process_sample(np.zeros((4, 4, 3), np.uint8), "", (32, 128), 'resize', None)[0][:, 0, 0]
    for shape in [(50, 1), (32, 77), (100, 5), (3, 400), (33, 33)]:
        chw, _, _ = process_sample(np.full(shape + (3,), 255, np.uint8), "", (32, 128), 'pad', None)
        w = target_width('pad', (32, 128), shape)
        assert np.all(chw[:, :, :w] != zero[:, None, None]) and np.all(chw[:, :, w:] == zero[:, None, None]), shape
