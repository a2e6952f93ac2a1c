"""Lexicon-constrained reading on the GPU (csrc/lexicon.hip).  Two rules:
  `Lexicon.nearest` (mr_lexicon_nearest): the nearest lexicon word, by Levenshtein distance, of every predicted id sequence;
  `Lexicon.transcribe` (mr_lexicon_transcribe): the CRNN paper's lexicon-based transcription (Shi et al., section 2.3.2) for CTC
  posteriors -- among the words within edit distance delta of the greedy string the one with the greatest CTC probability
  p(word | y), which is also a per-word confidence.
  The recognition benchmarks the reference's YAML files name (IIIT5K, SVT, IC03 / IC13) are reported
with lexicons -- 50 words per image, 1 k words per set, the "full" lexicon of ~90 k words -- and the rule is the same in all of
them: replace the prediction by the lexicon word with the smallest edit distance.  The reference itself only tests membership
(structure/measurers/sequence_recognition_measurer.py:59-64), on the host; `Lexicon.contains` is that test on id sequences.

    lexicon = Lexicon(words, charset)                       # or Lexicon.from_file(path, charset)
    found = lexicon.nearest(ids)                            # ids: i32 [N, S] on the device (greedy-decode output, blank padded)
    lexicon.strings(found['index']), found['distance']
    found = lexicon.transcribe(pred, max_distance=2)        # pred: [N, C, 1, T] posteriors of a CTC head, on the device
    lexicon.strings(found['index']), found['score']         # log p(word | pred); -1 / -inf where no word is possible

Words and predictions are compared as the measurer compares strings: case folded like `Charset.index`, then through the `.upper()`
canonical-id table (charsets.upper_fold_table).  There is no CPU fallback; the host half (`encode`) needs no GPU."""
import numpy as np
import torch

from .._lib import _DEFINES, call, ptr, require_cuda
from ..charsets import DefaultCharset, upper_fold_table
from .decode import _DT, _posterior, ctc_greedy_decode

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

    def _folded(self, pred, fold, log_probs):
        """The f32 posterior over the folded alphabet: q[n, k, t] = the sum of pred[n, c, t] over fold[c] == k (log input: the
        log of the sum of the exponentials, shifted by the column's maximum).  Classes that are nobody's canonical id get 0 / -inf."""
        index = fold.long()
        pred = pred.float()
        if not log_probs:
            return torch.zeros_like(pred).index_add_(1, index, pred)
        top = pred.amax(dim=1, keepdim=True)
        top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
        return torch.zeros_like(pred).index_add_(1, index, (pred - top).exp()).log() + top

    def transcribe(self, pred, spans=None, max_distance=None, log_probs=False, all_scores=False):
        """pred: [N, C, 1, T] or [N, C, T] on the device, any strides, C == len(charset): the class probabilities of a CTC head
        (the eval head's softmax), or their logs with `log_probs=True`; f32 and bf16 are read as they are, other types through
        f32.  Row n's candidates are the words of spans[n] (None: every word) within `max_distance` edits of the row's greedy
        string (None: all of them).  Returns i32 / f32 [N] device tensors: 'index' the candidate with the greatest CTC
        log-probability (the lowest index among equal scores), 'score' that log-probability, 'distance' the winner's edit distance
        to the greedy string (-1 / -inf / -1 when no candidate is possible), 'length' the symbols of the greedy string,
        'candidates' the number of candidates; with `all_scores=True` also 'scores', f32 [N, L]: every candidate's score, -inf
        elsewhere.  With a case-folding charset the likelihood is taken over the folded alphabet.  Greedy decode, (fold) and one
        call of mr_lexicon_transcribe; no host work that depends on device data (capturable in a graph after one call outside)."""
        require_cuda(pred)
        pred, (N, C, T), _, _ = _posterior(pred, "Lexicon.transcribe", error=ValueError)
        if C != self.classes:
            raise ValueError("pred has %d classes, the lexicon's charset %d" % (C, self.classes))
        dev = pred.device
        if self.device is not None and self.device.index is not None and self.device != dev:
            raise ValueError("pred is on %s, the lexicon was made for %s" % (dev, self.device))
        sym, off, fold = self._tensors(dev)
        if spans is not None:
            spans = spans.to(device=dev, dtype=torch.int32).contiguous()
            if tuple(spans.shape) != (N, 2):
                raise ValueError("spans must be [%d, 2], got %s" % (N, tuple(spans.shape)))
        L = len(self.words)
        out = {'index': torch.empty((N,), dtype=torch.int32, device=dev),
               'score': torch.empty((N,), dtype=torch.float32, device=dev),
               'distance': torch.empty((N,), dtype=torch.int32, device=dev),
               'length': torch.empty((N,), dtype=torch.int32, device=dev),
               'candidates': torch.empty((N,), dtype=torch.int32, device=dev)}
        if all_scores:
            out['scores'] = torch.empty((N, L), dtype=torch.float32, device=dev)
        if N == 0:
            return out
        if T < 1:
            raise ValueError("pred has no columns: %s" % (tuple(pred.shape),))
        with torch.cuda.device(dev):
            ids, _ = ctc_greedy_decode(pred, blank=self.blank, unknown=self.unknown)
            if fold is not None:
                pred = self._folded(pred, fold, log_probs)
            sn, sc, st = pred.stride()
            call("mr_lexicon_transcribe", _DT[pred.dtype], ptr(pred), sn, sc, st, T, int(bool(log_probs)),
                 ptr(ids), T, N, int(self.blank), int(self.unknown), ptr(fold), ptr(sym), ptr(off), L, ptr(spans), C,
                 -1 if max_distance is None else int(max_distance), ptr(out['index']), ptr(out['score']), ptr(out['distance']),
                 ptr(out['length']), ptr(out['candidates']), ptr(out.get('scores')) if all_scores and L else 0)
        return out

    def contains(self, ids, spans=None):
        """bool [N] on the device: the row, read as the measurer reads a label, is a word of the lexicon."""
        return self.nearest(ids, spans)['distance'] == 0

    def ids(self, index):
        """index: integer [N] on the device (what `nearest` / `transcribe` return).  Returns (i32 [N, Smax] blank padded, i32 [N]),
        both on the device: the folded symbols of the words index[n] and their lengths, length 0 where index[n] < 0; Smax is the
        longest word of the lexicon (at least 1).  Tensor indexing on the resident word table: nothing is copied to the host."""
        require_cuda(index)
        if index.dim() != 1:
            raise ValueError("index must be [N], got %s" % (tuple(index.shape),))
        dev = index.device
        sym, off, _ = self._tensors(dev)
        L = len(self.words)
        smax = max(int(np.diff(self.off).max()) if L else 0, 1)
        index = index.long()
        have = (index >= 0) & (index < L)
        word = index.clamp(0, max(L - 1, 0))
        lo = off[word].long()
        length = torch.where(have, off[(word + 1).clamp(max=L)].long() - lo, torch.zeros_like(lo))
        cols = torch.arange(smax, device=dev)
        take = (lo[:, None] + cols[None, :]).clamp(max=sym.numel() - 1)
        out = torch.where(cols[None, :] < length[:, None], sym[take], torch.full_like(take, int(self.blank), dtype=torch.int32))
        return out.to(torch.int32), length.to(torch.int32)

    def strings(self, index):
        """Host side: the words of an index tensor / sequence; None for -1."""
        if torch.is_tensor(index):
            index = index.cpu().tolist()
        return [None if int(i) < 0 else self.words[int(i)] for i in index]
