"""Pure numpy / Python restatement of lexicon-constrained reading, written from the description of mr_lexicon_nearest
(include/megreader_hip.h) and of the reference measurer's lexicon split -- not from the kernel.  The tests compare the library with
it exactly."""
import numpy as np


def compact(row, blank=0, unknown=1, fold=None):
    """The symbols of one id row: blank and unknown dropped, the rest through the fold table."""
    out = [int(v) for v in row if int(v) != blank and int(v) != unknown]
    return out if fold is None else [int(fold[v]) for v in out]


def levenshtein(a, b, unknown=None):
    """Two-row DP.  a: prediction symbols, b: word symbols; a word symbol equal to `unknown` matches nothing."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            same = x == y and y != unknown
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if same else 1))
        prev = cur
    return prev[len(b)]


def nearest(preds, words, blank=0, unknown=1, fold=None, spans=None):
    """(index, distance, length) int32 arrays: per row the lowest index among the nearest candidate words, its distance, and
    the row's number of symbols; -1 / -1 for an empty candidate range.  words: lists of (already folded) ids."""
    N = len(preds)
    index = np.full(N, -1, dtype=np.int32)
    distance = np.full(N, -1, dtype=np.int32)
    length = np.zeros(N, dtype=np.int32)
    cache = {}
    for n in range(N):
        a = compact(preds[n], blank, unknown, fold)
        length[n] = len(a)
        lo, hi = (0, len(words)) if spans is None else (int(spans[n][0]), int(spans[n][1]))
        for l in range(lo, hi):
            key = (tuple(a), tuple(words[l]))
            d = cache.get(key)
            if d is None:
                d = cache[key] = levenshtein(a, words[l], unknown)
            if distance[n] < 0 or d < distance[n]:          # strict: the lowest index keeps a tie
                index[n], distance[n] = l, d
    return index, distance, length


def distance_table(preds, words, blank=0, unknown=1, fold=None):
    """(D int64 [N, L], length int32 [N]): the distance of every row to every word, by the same two-row DP run for all words at
    once (numpy along the word axis).  test_lexicon_cpu.py checks it against `levenshtein`."""
    N, L = len(preds), len(words)
    length = np.zeros(N, dtype=np.int32)
    lens = np.array([len(w) for w in words], dtype=np.int64)
    width = int(lens.max()) if L else 0
    table = np.full((L, width), -1, dtype=np.int64)             # -1 pads: it matches nothing
    for l, w in enumerate(words):
        table[l, :len(w)] = [-1 if s == unknown else s for s in w]
    D = np.zeros((N, L), dtype=np.int64)
    for n in range(N):
        a = compact(preds[n], blank, unknown, fold)
        length[n] = len(a)
        prev = np.tile(np.arange(width + 1, dtype=np.int64), (L, 1))
        for i, x in enumerate(a, 1):
            cur = np.empty_like(prev)
            cur[:, 0] = i
            cost = (table != x).astype(np.int64)
            for j in range(1, width + 1):
                cur[:, j] = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + cost[:, j - 1])
            prev = cur
        D[n] = prev[np.arange(L), lens]
    return D, length


def nearest_in_table(D, length, spans=None):
    """(index, distance, length) from a distance table: the first minimum of each row's candidate range, -1 / -1 if it is empty."""
    N, L = D.shape
    index = np.full(N, -1, dtype=np.int32)
    distance = np.full(N, -1, dtype=np.int32)
    for n in range(N):
        lo, hi = (0, L) if spans is None else (int(spans[n][0]), int(spans[n][1]))
        if hi > lo:
            k = int(np.argmin(D[n, lo:hi]))                     # the first minimum: the lowest index
            index[n], distance[n] = lo + k, D[n, lo + k]
    return index, distance, length.astype(np.int32)


def nearest_rows(preds, words, blank=0, unknown=1, fold=None, spans=None):
    """`nearest` through `distance_table`: what the GPU tests compare with."""
    return nearest_in_table(*distance_table(preds, words, blank, unknown, fold), spans=spans)


MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def bit_parallel(a, b, unknown=None):
    """Global edit distance by the bit-parallel recurrence (Myers 1999 in Hyyro's form) in numpy uint64: a (<= 64 symbols) is the
    pattern, b the text.  Everything is masked to 64 bits: at 64 symbols the carry out of the add and the bits shifted out vanish."""
    m = len(a)
    assert m <= 64
    if m == 0:
        return len(b)
    one = np.uint64(1)
    peq = {}
    for i, x in enumerate(a):
        peq[x] = peq.get(x, np.uint64(0)) | (one << np.uint64(i))
    pv, mv, score, top = MASK, np.uint64(0), m, one << np.uint64(m - 1)
    with np.errstate(over='ignore'):
        for c in b:
            eq = np.uint64(0) if c == unknown else peq.get(c, np.uint64(0))
            xv = eq | mv
            xh = ((((eq & pv) + pv) & MASK) ^ pv) | eq
            ph = mv | (~(xh | pv) & MASK)
            mh = pv & xh
            score += int((ph & top) != 0)
            score -= int((mh & top) != 0)
            ph = ((ph << one) & MASK) | one
            mh = (mh << one) & MASK
            pv = mh | (~(xv | ph) & MASK)
            mv = ph & xv
    return score


def in_lexicon(label_strings, entries):
    """The reference's membership rule (sequence_recognition_measurer.py:59-64): the upper-cased label against the entries
    verbatim -- an entry that is not its own .upper() never matches."""
    entries = set(entries)
    return [s.upper() in entries for s in label_strings]


class Meter(object):
    """concern/average_meter.py."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        with np.errstate(invalid='ignore', divide='ignore'):
            self.avg = self.sum / self.count
        return self


def gather_split(raw_metrics, key):
    """(total, in-lexicon, out-of-lexicon) meters of one key over the batches: sequence_recognition_measurer.py:83-100, the
    per-batch sum / max(len, 1) and the update with a count of zero included."""
    meter, inside, outside = Meter(), Meter(), Meter()
    for m in raw_metrics:
        raw = np.array(m[key])
        flag = np.array(m['in_lexicon'])
        total = len(raw)
        meter.update(raw.sum() / total, total)
        sel = raw[flag == True]  # noqa: E712
        inside.update(sel.sum() / max(len(sel), 1), len(sel))
        sel = raw[flag == False]  # noqa: E712
        outside.update(sel.sum() / max(len(sel), 1), len(sel))
    return meter, inside, outside


def gather(raw_metrics):
    """The six meters of the reference's gather_measure with a lexicon, by name."""
    out = {}
    for key in ('edit_distance', 'accuracy'):
        for name, meter in zip(('total_', 'in_lexicon_', 'out_lexicon_'), gather_split(raw_metrics, key)):
            out[name + key] = meter
    return out
