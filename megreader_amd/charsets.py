"""Charset objects: the alphabet of a recognition head and the mapping between characters and class ids.

Same construction rules as reference concern/charsets.py:17-29,65-78,101-110: the corpus is reduced to its sorted unique
characters, then blank (id 0) and unknown (id 1) are inserted in front.  Only ChineseCharset upper-cases its corpus first (unless
it is case sensitive); the general Charset keeps the corpus as given, so the 52 letters of EnglishPrintableCharset are 52 classes
although `index` of a case-insensitive charset folds every query to upper case (the lower-case classes are never targets).

EnglishCharset = 36 alphanumerics => 38 classes; EnglishPrintableCharset = digits, letters and punctuation => 96 classes;
ChineseCharset = the characters of ./assets/chinese_charset.dic => 5 360 classes with the reference's dictionary.  The reference's
own Charset objects (constructed from YAML) are accepted unchanged by the decoders; EnglishCharset is the default when none is
passed.
"""
import string

import numpy as np


class Charset(object):
    """Alphabet built from the characters of `corpus` (any iterable of characters)."""

    def __init__(self, corpus, blank=0, unknown=1, case_sensitive=False, blank_char=None, unknown_char=None):
        self.blank = blank
        self.unknown = unknown
        self.case_sensitive = case_sensitive
        # reference quirk Q6: a charset built from YAML carries None for both placeholder characters
        self.blank_char = blank_char
        self.unknown_char = unknown_char
        chars = set(self._filter_corpus(corpus))
        chars.discard(blank_char)
        chars.discard(unknown_char)
        self._charset = sorted(chars)
        self._charset.insert(blank, blank_char)
        self._charset.insert(unknown, unknown_char)
        self._lut = {ch: i for i, ch in enumerate(self._charset)}

    def _filter_corpus(self, corpus):
        return corpus

    def __len__(self):
        return len(self._charset)

    def __getitem__(self, index):
        return self._charset[index]

    def is_empty(self, index):
        return index == self.blank or index == self.unknown

    def is_empty_char(self, x):
        return x == self.blank_char or x == self.unknown_char

    def index(self, x):
        """Class id of one character; `unknown` if the alphabet does not hold it (concern/charsets.py:37-41)."""
        return self._lut.get(x if self.case_sensitive else x.upper(), self.unknown)

    def string_to_label(self, string_input, max_size=32):
        """int32 ids of a string, zero padded to at least `max_size` entries."""
        label = np.zeros((max(max_size, len(string_input)),), dtype=np.int32)
        for i, ch in enumerate(string_input):
            label[i] = self.index(ch)
        return label

    def label_to_string(self, label):
        ignore = (self.unknown, self.blank)
        return "".join(self._charset[int(i)] for i in label if int(i) not in ignore)


class EnglishCharset(Charset):
    def __init__(self, **kwargs):
        super().__init__(string.digits + string.ascii_uppercase, **kwargs)


class EnglishPrintableCharset(Charset):
    def __init__(self, **kwargs):
        super().__init__(string.digits + string.ascii_letters + string.punctuation, **kwargs)


class ChineseCharset(Charset):
    """The characters of ./assets/chinese_charset.dic, a path relative to the working directory as in the reference."""
    DICTIONARY = "./assets/chinese_charset.dic"

    def __init__(self, **kwargs):
        with open(self.DICTIONARY, encoding="utf-8") as reader:
            corpus = reader.read().strip()
        super().__init__(corpus, **kwargs)

    def _filter_corpus(self, corpus):
        return corpus if self.case_sensitive else [ch.upper() for ch in corpus]


DefaultCharset = EnglishCharset


def upper_fold_table(charset):
    """id -> canonical id under `.upper()` of the characters: ids whose characters upper-case to the same character get the id of
    the first of them, so that comparing folded id sequences is comparing the upper-cased strings (what
    SequenceRecognitionMeasurer and Lexicon do).  A list of len(charset) ints, or None when the table would be the identity or the
    object has no `_charset` list to read."""
    if charset is None or not hasattr(charset, "_charset"):
        return None
    canon, fold = {}, []
    for i, ch in enumerate(charset._charset):
        key = ch.upper() if isinstance(ch, str) else ("#", i)
        fold.append(canon.setdefault(key, i))
    return fold if any(f != i for i, f in enumerate(fold)) else None
