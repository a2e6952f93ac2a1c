"""Lexicon-constrained reading on the GPU (mr_lexicon_nearest, csrc/lexicon.hip): the nearest lexicon word, by Levenshtein distance,
of every predicted id sequence.  The recognition benchmarks the reference's YAML files name (IIIT5K, SVT, IC03 / IC13) are reported
with lexicons -- 50 words per image, 1 k words per set, the "full" lexicon of ~90 k words -- and the rule is the same in all of
them: replace the prediction by the lexicon word with the smallest edit distance.  The reference itself only tests membership
(structure/measurers/sequence_recognition_measurer.py:59-64), on the host; `Lexicon.contains` is that test on id sequences.

    lexicon = Lexicon(words, charset)                       # or Lexicon.from_file(path, charset)
    found = lexicon.nearest(ids)                            # ids: i32 [N, S] on the device (greedy-decode output, blank padded)
    lexicon.strings(found['index']), found['distance']

Words and predictions are compared as the measurer compares strings: case folded like `Charset.index`, then through the `.upper()`
canonical-id table (charsets.upper_fold_table).  There is no CPU fallback; the host half (`encode`) needs no GPU."""
import numpy as np
import torch

from .._lib import _DEFINES, call, ptr, require_cuda
from ..charsets import DefaultCharset, upper_fold_table

MAX_WORD = _DEFINES["MR_LEXICON_MAX_WORD"]


class Lexicon(object):
    def __init__(self, words, charset=None, device=None):
        self.charset = charset if charset is not None else DefaultCharset()
        self.words = list(words)                    # the original strings, in index order
        self.blank = getattr(self.charset, 'blank', 0)
        self.unknown = getattr(self.charset, 'unknown', 1)
        self.classes = len(self.charset)
        self.sym, self.off = self.encode(self.words, self.charset)
        self.fold = upper_fold_table(self.charset)
        self.device = None if device is None else torch.device(device)
        self._resident = {}                         # device -> (sym, off, fold) tensors, uploaded on first use

    def __len__(self):
        return len(self.words)

    @staticmethod
    def encode(words, charset):
        """(sym i32 [total], off i32 [L + 1]) as numpy: word l is sym[off[l]:off[l + 1]], every character through `charset.index`
        (characters outside the alphabet become `unknown` and are kept: they match nothing) and then the `.upper()` fold table."""
        fold = upper_fold_table(charset)
        off = np.zeros(len(words) + 1, dtype=np.int64)
        sym = []
        for l, word in enumerate(words):
            if len(word) > MAX_WORD:
                raise ValueError("lexicon word %r has %d symbols; mr_lexicon_nearest takes at most %d" % (word, len(word), MAX_WORD))
            ids = [charset.index(ch) for ch in word]
            sym.extend(ids if fold is None else [fold[i] for i in ids])
            off[l + 1] = len(sym)
        if off[-1] > np.iinfo(np.int32).max:
            raise ValueError("lexicon of %d symbols does not fit int32 offsets" % off[-1])
        return np.asarray(sym, dtype=np.int32), off.astype(np.int32)

    @classmethod
    def from_file(cls, path, charset=None, device=None):
        """The words of a whitespace-separated file: `set(f.read().split())` as the reference reads `nori_lexicon_path`, sorted so
        that word indices are reproducible."""
        with open(path) as f:
            return cls(sorted(set(f.read().split())), charset, device)

    @classmethod
    def grouped(cls, word_lists, charset=None, device=None):
        """Per-row lexicons laid end to end: (lexicon, spans), spans an i32 [N, 2] tensor with row n's words at
        [spans[n, 0], spans[n, 1]) -- pass it to `nearest` / `contains`."""
        words, spans = [], []
        for group in word_lists:
            group = list(group)
            spans.append((len(words), len(words) + len(group)))
            words.extend(group)
        return cls(words, charset, device), torch.tensor(spans, dtype=torch.int32).reshape(-1, 2)

    def _tensors(self, device):
        got = self._resident.get(device)
        if got is None:
            sym = np.concatenate([self.sym, np.zeros(1, dtype=np.int32)])      # never an empty allocation (a null pointer)
            fold = None if self.fold is None else torch.tensor(self.fold, dtype=torch.int32, device=device)
            got = self._resident[device] = (torch.from_numpy(sym).to(device), torch.from_numpy(self.off).to(device), fold)
        return got

    def nearest(self, ids, spans=None):
        """ids: i32 [N, S] on the device.  spans: optional i32 [N, 2], row n's candidate words [lo, hi); None: every word.
        Returns {'index', 'distance', 'length'}, i32 [N] device tensors: the lowest index among the nearest candidates and its
        distance (-1 / -1 for an empty candidate range), and the number of symbols of the row.  One call of mr_lexicon_nearest; no
        host work that depends on device data (capturable in a graph after one call outside the capture)."""
        require_cuda(ids)
        if ids.dim() != 2:
            raise ValueError("ids must be [N, S], got %s" % (tuple(ids.shape),))
        dev = ids.device
        if self.device is not None and self.device.index is not None and self.device != dev:
            raise ValueError("ids are on %s, the lexicon was made for %s" % (dev, self.device))
        ids = ids.to(torch.int32).contiguous()
        N, S = ids.shape
        sym, off, fold = self._tensors(dev)
        if spans is not None:
            spans = spans.to(device=dev, dtype=torch.int32).contiguous()
            if tuple(spans.shape) != (N, 2):
                raise ValueError("spans must be [%d, 2], got %s" % (N, tuple(spans.shape)))
        index = torch.empty((N,), dtype=torch.int32, device=dev)
        distance = torch.empty((N,), dtype=torch.int32, device=dev)
        length = torch.empty((N,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            call("mr_lexicon_nearest", ptr(ids), S, N, int(self.blank), int(self.unknown), ptr(fold), ptr(sym), ptr(off),
                 len(self.words), ptr(spans), int(self.classes), ptr(index), ptr(distance), ptr(length))
        return {'index': index, 'distance': distance, 'length': length}

    def contains(self, ids, spans=None):
        """bool [N] on the device: the row, read as the measurer reads a label, is a word of the lexicon."""
        return self.nearest(ids, spans)['distance'] == 0

    def strings(self, index):
        """Host side: the words of an index tensor / sequence; None for -1."""
        if torch.is_tensor(index):
            index = index.cpu().tolist()
        return [None if int(i) < 0 else self.words[int(i)] for i in index]
