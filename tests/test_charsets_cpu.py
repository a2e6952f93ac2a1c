"""CPU: megreader_amd.charsets (Charset, EnglishCharset, EnglishPrintableCharset, ChineseCharset) against the reference's
concern/charsets.py objects where the reference tree exists, the construction rules on their own everywhere, the label table of
the device pipeline on a 5 360-class alphabet, and the host-only path query mr_ctc_wide."""
import os
import string

import numpy as np
import pytest

from megreader_amd import _lib, charsets
from megreader_amd.data.device_pipeline import charset_table

MIXED = "aZ9 ~q中文Kk_0é!"     # letters of both cases, digits, punctuation, CJK, a character no charset holds


def wide_charset():
    """5 360 classes without the reference's dictionary: 5 358 CJK ideographs from U+4E00 on."""
    return charsets.Charset([chr(0x4E00 + i) for i in range(5358)])


def _same(ours, theirs, probes):
    assert len(ours) == len(theirs)
    assert [ours[i] for i in range(len(ours))] == [theirs[i] for i in range(len(theirs))]
    assert ours.blank == theirs.blank and ours.unknown == theirs.unknown
    for ch in probes:
        assert ours.index(ch) == theirs.index(ch), ch
    assert all(ours.is_empty(i) == theirs.is_empty(i) for i in range(4))
    for text in (MIXED, MIXED * 4):               # the second is longer than max_size
        a, b = ours.string_to_label(text), theirs.string_to_label(text)
        assert a.dtype == b.dtype and np.array_equal(a, b)
        assert ours.label_to_string(a) == theirs.label_to_string(b)


@pytest.fixture()
def reference_charsets(tmp_path, monkeypatch):
    from oracle import refimport
    if not refimport.available():
        pytest.skip("reference tree not present (GPU box)")
    refimport.import_reference()
    import concern.charsets as ref
    # ./assets/chinese_charset.dic is read relative to the working directory (concern/charsets.py:68)
    os.symlink(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(ref.__file__))), "assets"), tmp_path / "assets")
    monkeypatch.chdir(tmp_path)
    return ref


def test_english_charsets_equal_the_reference(reference_charsets):
    ref = reference_charsets
    ours, theirs = charsets.EnglishCharset(), ref.EnglishCharset()
    assert len(ours) == 38
    _same(ours, theirs, list(string.printable) + ["中"])
    ours, theirs = charsets.EnglishPrintableCharset(), ref.EnglishPrintableCharset()
    assert len(ours) == 96
    _same(ours, theirs, list(string.printable) + ["中"])


def test_general_charset_equals_the_reference(reference_charsets):
    ref = reference_charsets
    corpus = "hello, World 0123 中文中"
    for cs in (False, True):
        ours = charsets.Charset(corpus, case_sensitive=cs)
        theirs = ref.Charset(corpus, case_sensitive=cs)
        _same(ours, theirs, list(corpus) + ["H", "w", "#"])


def test_chinese_charset_equals_the_reference(reference_charsets):
    ref = reference_charsets
    ours, theirs = charsets.ChineseCharset(), ref.ChineseCharset()
    assert len(ours) == 5360
    probes = [theirs[i] for i in range(2, len(theirs))] + list("abcXYZ09") + ["é", "￿"]
    _same(ours, theirs, probes)
    ours, theirs = charsets.ChineseCharset(case_sensitive=True), ref.ChineseCharset(case_sensitive=True)
    _same(ours, theirs, list("abcXYZ09") + [theirs[i] for i in range(2, len(theirs), 97)])


def test_construction_rules():
    cs = charsets.Charset("banana Bread")
    assert [cs[i] for i in range(len(cs))] == [None, None, " ", "B", "a", "b", "d", "e", "n", "r"]
    assert cs.index("b") == cs.index("B") == 3          # queries fold to upper case; the class of "b" is never a target
    assert cs.index("a") == cs.unknown == 1 and cs.index("?") == 1
    assert charsets.Charset("banana Bread", case_sensitive=True).index("a") == 4
    assert cs.is_empty(0) and cs.is_empty(1) and not cs.is_empty(2)
    lab = cs.string_to_label("B B")
    assert lab.dtype == np.int32 and lab.shape == (32,) and lab[:4].tolist() == [3, 2, 3, 0]
    assert cs.string_to_label("B" * 40).shape == (40,)
    assert cs.label_to_string([3, 0, 1, 2, 3]) == "B B"
    assert len(charsets.EnglishCharset()) == 38 and len(charsets.EnglishPrintableCharset()) == 96
    assert charsets.DefaultCharset is charsets.EnglishCharset
    e = charsets.EnglishCharset()
    assert e.index("a") == e.index("A") == 12 and e[2] == "0" and e[37] == "Z" and e.label_to_string([12, 0, 1, 2]) == "A0"


def test_chinese_charset_reads_the_dictionary_of_the_working_directory(tmp_path, monkeypatch):
    (tmp_path / "assets").mkdir()
    (tmp_path / "assets" / "chinese_charset.dic").write_text("文a中A文z\n", encoding="utf-8")
    monkeypatch.chdir(tmp_path)
    cs = charsets.ChineseCharset()
    assert [cs[i] for i in range(len(cs))] == [None, None, "A", "Z", "中", "文"]
    assert cs.index("a") == 2 and cs.index("文") == 5
    cs = charsets.ChineseCharset(case_sensitive=True)
    assert [cs[i] for i in range(len(cs))] == [None, None, "A", "a", "z", "中", "文"]


def test_charset_table_of_a_wide_charset_round_trips_every_id():
    cs = wide_charset()
    assert len(cs) == 5360
    cps, ids = charset_table(cs)
    assert cps.dtype == np.int32 and ids.dtype == np.int32
    assert np.all(np.diff(cps) > 0)                                  # strictly sorted: the kernel searches it by bisection
    lut = dict(zip(cps.tolist(), ids.tolist()))
    for i in range(2, len(cs)):
        assert lut[ord(cs[i])] == i == cs.index(cs[i])
    assert sorted(ids.tolist()) == list(range(2, 5360))


def test_ctc_wide_path_query():
    lib = _lib.load()
    assert lib.mr_ctc_wide(38, 32) == 0 and lib.mr_ctc_wide(3932, 32) == 0
    assert lib.mr_ctc_wide(3933, 32) == 1 and lib.mr_ctc_wide(5360, 32) == 1
    assert lib.mr_ctc_wide(96, 32) == 0 and lib.mr_ctc_wide(4099, 32) == 1 and lib.mr_ctc_wide(5360, 25) == 1
