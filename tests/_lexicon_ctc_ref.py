"""Pure numpy restatement of lexicon transcription by CTC likelihood, written from the description of mr_lexicon_transcribe
(include/megreader_hip.h) -- not from the kernel.  `word_score` is the alpha recursion over the blank-extended word in the dtype
asked for: float64 is the truth the tests hold the device to, float32 shows how much of a difference is rounding at the
magnitude of the scores.  Candidates and distances come from _lexicon_ref.distance_table."""
import numpy as np

import _lexicon_ref as R

NEG = -np.inf


def log_probs(y, dtype):
    """log of the probabilities in `dtype` (0 -> -inf without a warning)."""
    with np.errstate(divide='ignore'):
        return np.log(np.asarray(y).astype(dtype))


def lse(terms):
    """log(sum(exp(term))) over a list of equally shaped arrays, shifted by the greatest term; -inf where every term is."""
    stack = np.stack(terms)
    top = stack.max(axis=0)
    shift = np.where(np.isfinite(top), top, 0).astype(stack.dtype)
    total = np.exp(stack[0] - shift)
    for term in stack[1:]:
        total = total + np.exp(term - shift)
    with np.errstate(divide='ignore'):
        out = shift + np.log(total)
    return np.where(top == NEG, top, out).astype(stack.dtype)


def word_score(lp, word, blank=0, dtype=np.float64, unknown=None):
    """log p(word | lp): lp [T, C] (one row, a scalar comes back) or [N, T, C] (all rows at once, [N] comes back) of
    log-probabilities; every operation in `dtype`.  A word with `unknown` or an id outside [0, C) matches nothing: -inf."""
    lp = np.asarray(lp).astype(dtype)
    single = lp.ndim == 2
    if single:
        lp = lp[None]
    N, T, C = lp.shape
    word = [int(s) for s in word]
    if any(s == unknown or not 0 <= s < C for s in word):
        out = np.full(N, NEG, dtype=dtype)
        return out[0] if single else out
    ext = [blank]
    for s in word:
        ext += [s, blank]
    P = len(ext)
    hop = np.array([s >= 2 and s % 2 == 1 and ext[s] != ext[s - 2] for s in range(P)])
    alpha = np.full((N, P), NEG, dtype=dtype)
    alpha[:, 0] = lp[:, 0, blank]
    if P > 1:
        alpha[:, 1] = lp[:, 0, ext[1]]
    none1 = np.full((N, 1), NEG, dtype=dtype)
    none2 = np.full((N, 2), NEG, dtype=dtype)
    for t in range(1, T):
        one = np.concatenate([none1, alpha[:, :-1]], axis=1)
        two = np.concatenate([none2, alpha[:, :-2]], axis=1)[:, :P] if P > 2 else np.full((N, P), NEG, dtype=dtype)
        two = np.where(hop[None, :], two, np.asarray(NEG, dtype=dtype))
        alpha = (lp[:, t, ext] + lse([alpha, one, two])).astype(dtype)
    out = alpha[:, 0] if P == 1 else lse([alpha[:, P - 1], alpha[:, P - 2]])
    return out[0] if single else out


def score_table(lp, words, blank=0, dtype=np.float64, unknown=None):
    """[N, L]: score(n, l) of every row and word.  lp: [N, T, C]."""
    out = np.full((len(lp), len(words)), NEG, dtype=dtype)
    for l, w in enumerate(words):
        out[:, l] = word_score(lp, w, blank, dtype, unknown)
    return out


def greedy(y, blank=0, unknown=1):
    """mr_ctc_greedy_decode on y [N, T, C]: i32 [N, T] blank padded (arg-max, first index on ties; an `unknown` is skipped without
    becoming `previous`; a symbol equal to `previous` is skipped; blanks are not emitted)."""
    y = np.asarray(y)
    out = np.full(y.shape[:2], blank, dtype=np.int32)
    for n, best in enumerate(np.argmax(y, axis=2)):
        prev, k = blank, 0
        for c in best:
            if c == unknown:
                continue
            if c != prev and c != blank:
                out[n, k] = c
                k += 1
            prev = c
    return out


def candidates(D, spans=None, max_distance=None):
    """bool [N, L]: the words of each row's span within max_distance (None or negative: the whole span)."""
    N, L = D.shape
    mask = np.zeros((N, L), dtype=bool)
    for n in range(N):
        lo, hi = (0, L) if spans is None else (min(max(int(spans[n][0]), 0), L), min(max(int(spans[n][1]), 0), L))
        mask[n, lo:max(lo, hi)] = True
    if max_distance is not None and max_distance >= 0:
        mask &= D <= max_distance
    return mask


def transcribe(S, D, length, spans=None, max_distance=None):
    """The outputs of mr_lexicon_transcribe from a score table S and a distance table D (both [N, L]): a dict of index, score,
    distance, length, candidates and the masked table `scores` (-inf for non-candidates)."""
    mask = candidates(D, spans, max_distance)
    scores = np.where(mask, S, NEG)
    N = len(S)
    index = np.full(N, -1, dtype=np.int32)
    best = np.full(N, NEG, dtype=S.dtype)
    distance = np.full(N, -1, dtype=np.int32)
    for n in range(N):
        if scores.shape[1] and scores[n].max() > NEG:
            index[n] = int(np.argmax(scores[n]))                 # the first maximum: the lowest index
            best[n] = scores[n, index[n]]
            distance[n] = D[n, index[n]]
    return dict(index=index, score=best, distance=distance, length=np.asarray(length, dtype=np.int32),
                candidates=mask.sum(axis=1).astype(np.int32), scores=scores)


def fold_posterior(y, fold, log=False):
    """q[..., k] = the sum of y[..., c] over fold[c] == k (log: the log of the sum of the exponentials); the class axis is last."""
    y = np.asarray(y, dtype=np.float64)
    q = np.zeros_like(y)
    for c, k in enumerate(fold):
        q[..., k] += np.exp(y[..., c]) if log else y[..., c]
    if log:
        with np.errstate(divide='ignore'):
            q = np.log(q)
    return q


def brute_force(y, blank=0):
    """{collapsed word (tuple): probability} by enumerating all C^T paths of y [T, C]."""
    T, C = y.shape
    out = {}
    for code in range(C ** T):
        path, p = [], 1.0
        for t in range(T):
            c = code % C
            code //= C
            path.append(c)
            p *= float(y[t, c])
        word, prev = [], None
        for c in path:
            if c != prev and c != blank:
                word.append(c)
            prev = c
        out[tuple(word)] = out.get(tuple(word), 0.0) + p
    return out
