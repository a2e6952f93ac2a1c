"""The host half of lexicon-constrained reading (megreader_amd/ops/lexicon.py `Lexicon.encode` / `from_file` / `grouped`, the
shared fold table, the measurer's six-meter gather) and the bit-parallel recurrence of csrc/lexicon.hip restated in numpy
(tests/_lexicon_ref.py) against a plain DP.  No GPU."""
import math
import random
import string

import numpy as np
import pytest

import _lexicon_ref as R
from megreader_amd.charsets import Charset, ChineseCharset, EnglishCharset, EnglishPrintableCharset, upper_fold_table
from megreader_amd.ops.lexicon import Lexicon
from megreader_amd.structure.measurers import SequenceRecognitionMeasurer


def words_of(sym, off):
    return [sym[off[l]:off[l + 1]].tolist() for l in range(len(off) - 1)]


def test_english_charset_folds_case_in_index():
    cs = EnglishCharset()
    sym, off = Lexicon.encode(['hello', 'HELLO'], cs)
    a, b = words_of(sym, off)
    assert a == b == [cs.index(ch) for ch in 'HELLO']
    assert sym.dtype == np.int32 and off.dtype == np.int32 and off.tolist() == [0, 5, 10]


def test_printable_charset_joins_case_only_through_the_fold_table():
    cs = EnglishPrintableCharset(case_sensitive=True)
    assert len(cs) == 96
    lower = [cs.index(ch) for ch in 'hello']
    upper = [cs.index(ch) for ch in 'HELLO']
    assert lower != upper                                  # 52 letters are 52 classes
    fold = upper_fold_table(cs)
    assert [fold[i] for i in lower] == [fold[i] for i in upper]
    a, b = words_of(*Lexicon.encode(['hello', 'HELLO'], cs))
    assert a == b == [fold[i] for i in upper]


def test_character_outside_the_alphabet_stays_unknown():
    cs = EnglishCharset()
    (word,) = words_of(*Lexicon.encode(['A-B'], cs))
    assert word == [cs.index('A'), cs.unknown, cs.index('B')]


def test_word_length_limits():
    cs = EnglishCharset()
    sym, off = Lexicon.encode(['A' * 64, ''], cs)
    assert off.tolist() == [0, 64, 64]                     # 64 symbols are accepted, the empty word is allowed
    with pytest.raises(ValueError, match='B' * 65):
        Lexicon.encode(['A', 'B' * 65], cs)
    lex = Lexicon(['ab', '', 'Ab'], cs)
    assert lex.words == ['ab', '', 'Ab'] and len(lex) == 3
    assert lex.strings([2, -1, 0]) == ['Ab', None, 'ab']


def test_from_file_is_the_sorted_set_of_split(tmp_path):
    path = tmp_path / "lexicon.txt"
    text = "zebra apple\nApple  apple\tmango\n\nzebra 42\n"
    path.write_text(text)
    lex = Lexicon.from_file(str(path), EnglishCharset())
    assert lex.words == sorted(set(text.split()))


def test_grouped_spans_tile_the_lexicon():
    groups = [['a', 'bb'], [], ['ccc'], ['d', 'e', 'f']]
    lex, spans = Lexicon.grouped(groups, EnglishCharset())
    spans = spans.tolist()
    assert lex.words == [w for g in groups for w in g]
    assert spans[0][0] == 0 and spans[-1][1] == len(lex)
    assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
    assert [lex.words[lo:hi] for lo, hi in spans] == groups
    empty, none = Lexicon.grouped([], EnglishCharset())
    assert len(empty) == 0 and tuple(none.shape) == (0, 2)


@pytest.mark.parametrize("alphabet", [2, 36])
def test_bit_parallel_restatement_equals_the_dp(alphabet):
    rng = random.Random(alphabet)
    for m in (0, 1, 31, 32, 33, 63, 64):
        for n in (0, 1, 7, 64):
            for _ in range(6):
                a = [rng.randrange(2, 2 + alphabet) for _ in range(m)]
                b = [rng.randrange(2, 2 + alphabet) for _ in range(n)]
                assert R.bit_parallel(a, b) == R.levenshtein(a, b), (m, n)
            near = list(a[:n]) + [2] * max(0, n - m)     # the word a prefix of the pattern (or the pattern itself, padded)
            assert R.bit_parallel(a, near) == R.levenshtein(a, near)
            if n:
                last = near[:-1] + [near[-1] + 1]        # ... and differing from it only in the last symbol
                assert R.bit_parallel(a, last) == R.levenshtein(a, last)
    # an `unknown` in the word matches nothing, on both sides of the comparison
    assert R.bit_parallel([5, 1, 6], [5, 1, 6], unknown=1) == R.levenshtein([5, 1, 6], [5, 1, 6], unknown=1) == 1


def _batches():
    # (edit_distance, accuracy, in_lexicon): no in-lexicon row first, then only in-lexicon rows, then mixed
    return [dict(edit_distance=[0.5, 0.25, 1.0], accuracy=[False, False, True], in_lexicon=[False, False, False]),
            dict(edit_distance=[1.0, 0.75], accuracy=[True, False], in_lexicon=[True, True]),
            dict(edit_distance=[0.0, 1.0, 0.6, 0.2], accuracy=[False, True, False, False], in_lexicon=[True, False, True, False])]


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_gather_measure_with_a_lexicon_is_the_reference_arithmetic():
    measurer = SequenceRecognitionMeasurer(charset=EnglishCharset(), lexicon=['HELLO', 'WORLD'])
    for upto in (1, 2, 3):                                  # after the first batch the in-lexicon meters average to nan
        raw = _batches()[:upto]
        got = measurer.gather_measure(raw)
        want = R.gather(raw)
        assert sorted(got) == sorted(want) == sorted(
            p + k for p in ('total_', 'in_lexicon_', 'out_lexicon_') for k in ('edit_distance', 'accuracy'))
        for key in want:
            for field in ('val', 'avg', 'sum', 'count'):
                assert _same(float(getattr(got[key], field)), float(getattr(want[key], field))), (upto, key, field)
    first = measurer.gather_measure(_batches()[:1])
    assert math.isnan(first['in_lexicon_accuracy'].avg) and first['in_lexicon_accuracy'].count == 0
    assert first['out_lexicon_edit_distance'].avg == np.array([0.5, 0.25, 1.0]).sum() / 3
    # hand-checked on the mixed batch alone
    mixed = measurer.gather_measure(_batches()[2:])
    assert mixed['in_lexicon_edit_distance'].avg == (0.0 + 0.6) / 2 and mixed['in_lexicon_edit_distance'].count == 2
    assert mixed['out_lexicon_accuracy'].avg == 0.5 and mixed['total_accuracy'].avg == 0.25


def test_gather_measure_without_a_lexicon_keeps_its_two_keys(tmp_path):
    raw = [dict(edit_distance=m['edit_distance'], accuracy=m['accuracy']) for m in _batches()]
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    for measurer in (SequenceRecognitionMeasurer(charset=EnglishCharset()),
                     SequenceRecognitionMeasurer(charset=EnglishCharset(), nori_lexicon_path=None, lexicon=None, correct=False),
                     SequenceRecognitionMeasurer(charset=EnglishCharset(), nori_lexicon_path=str(empty))):
        got = measurer.gather_measure(raw)
        assert sorted(got) == ['accuracy', 'edit_distance']
        assert got['accuracy'].count == 9 and got['accuracy'].avg == (1 + 1 + 1) / 9
        assert got['edit_distance'].sum == sum(np.array(m['edit_distance']).sum() / len(m['edit_distance']) * len(m['edit_distance'])
                                               for m in raw)


def test_measurer_reads_the_lexicon_file_and_sets_members_first(tmp_path):
    path = tmp_path / "lexicon.txt"
    path.write_text("WORLD hello HELLO\nA1\n")
    measurer = SequenceRecognitionMeasurer(charset=EnglishCharset(), nori_lexicon_path=str(path))
    assert measurer.lexicon.words == ['A1', 'HELLO', 'WORLD', 'hello'] and measurer.members == 3


def _fold_as_the_measurer_built_it(charset):
    canon, fold = {}, []
    for i, ch in enumerate(charset._charset):
        key = ch.upper() if isinstance(ch, str) else ("#", i)
        fold.append(canon.setdefault(key, i))
    return fold if any(f != i for i, f in enumerate(fold)) else None


def test_shared_fold_table_is_the_table_the_measurer_built(tmp_path, monkeypatch):
    (tmp_path / "assets").mkdir()
    (tmp_path / "assets" / "chinese_charset.dic").write_text("文a中A文zßσΣǆ0-\n", encoding="utf-8")
    monkeypatch.chdir(tmp_path)                            # ChineseCharset reads ./assets/chinese_charset.dic
    for cs in (EnglishCharset(), EnglishPrintableCharset(), EnglishPrintableCharset(case_sensitive=True), ChineseCharset(),
               ChineseCharset(case_sensitive=True), Charset(string.ascii_letters, case_sensitive=True)):
        want = _fold_as_the_measurer_built_it(cs)
        assert upper_fold_table(cs) == want
        fold = SequenceRecognitionMeasurer(charset=cs).fold
        assert (fold is None) == (want is None)
        if want is not None:
            assert fold.tolist() == want
    assert upper_fold_table(EnglishCharset()) is None and upper_fold_table(None) is None
    assert upper_fold_table(EnglishPrintableCharset()) is not None


def test_the_row_wise_restatement_equals_the_scalar_one():
    rng = np.random.RandomState(5)
    words = [rng.randint(1, 6, size=k).tolist() for k in rng.randint(0, 9, size=40)]      # 1 = unknown inside words
    preds = rng.randint(0, 6, size=(9, 12))
    fold = [0, 1, 2, 2, 4, 5]
    spans = [[0, 40], [3, 3], [5, 6], [10, 40], [0, 1], [39, 40], [7, 30], [20, 10], [0, 40]]
    for kw in (dict(), dict(spans=spans), dict(fold=fold), dict(blank=5, unknown=3)):
        for got, want in zip(R.nearest_rows(preds, words, **kw), R.nearest(preds, words, **kw)):
            assert got.tolist() == want.tolist(), kw
