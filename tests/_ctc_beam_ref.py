"""Pure numpy restatement of CTC prefix beam search, written from the descriptions of mr_ctc_beam_search and, with a character
n-gram model, mr_ctc_beam_search_lm (include/megreader_hip.h) -- not from the kernel.  Hypotheses are keyed by their CONTENT (a tuple of class ids in a dict), every
log mass is held in the dtype asked for: float64 is the truth the tests hold the device to, float32 shows how much of a
difference is rounding.  `lp` is the table of log-probabilities as given -- for the device the f32 table the header defines
(`logs`) -- and is taken to `dtype` for the arithmetic; the symbols of a column are chosen on the table as given.  Besides the
hypotheses a row's result says how far the row was from deciding differently (`margin`) and how often a prefix came back into
the beam beside a child that had stayed (`reentries`), so that a test knows what it may assert.
`enumerate_strings` is the other yardstick: every path, no algorithm."""
import itertools

import numpy as np

from _lexicon_ctc_ref import NEG, log_probs, lse, word_score


def logs(y, log_probs_given=False):
    """lp f32 [..., T, C] of a posterior y [..., T, C] (f32 values): the f32 nearest to the f64 log, 0 -> -inf; logs pass."""
    y = np.asarray(y, dtype=np.float32)
    return y if log_probs_given else log_probs(y, np.float64).astype(np.float32)


def column_symbols(col, top_classes, blank, unknown):
    """(ids of the column's symbols in order, gap between the last one taken and the best one left out -- inf when none is).
    col: [C].  Greatest lp first, the lower id among bit-equal values; blank, unknown and -inf are not eligible."""
    col = np.asarray(col)
    ids = np.arange(len(col))
    ids = ids[(ids != blank) & (ids != unknown) & (col > NEG)]
    ids = ids[np.lexsort((ids, -col[ids]))].tolist()
    taken = ids[:top_classes]
    gap = float(col[taken[-1]]) - float(col[ids[top_classes]]) if len(ids) > top_classes else np.inf
    return taken, gap


def beam_search(lp, beam, nbest, top_classes, blank=0, unknown=1, dtype=np.float64, model=None, alpha=0.0, beta=0.0, end=False):
    """One row.  lp: [T, C].  Returns dict(hyps=[(tuple of ids, score)] -- at most nbest, descending --, margin, reentries).
    With `model` the search is mr_ctc_beam_search_lm's: a state and a sum lm per hypothesis, step 5 and the final order read total +
    lm while the masses stay the pure CTC ones, and hyps are (tuple of ids, score, ctc_score, lm_score).  `model` is anything with
    `start`, `terms(state, c) -> ([backoff weights in the order met], the n-gram's value or None, next state)` and `end(state)`
    (_ngram_lm_ref.DictLM: the state is the history itself).  The model's part is held in `dtype` like the masses: float32 follows
    the header's order -- acc = 0, acc += bow .., g = acc + value; lm += (alpha * g + beta), each operation rounded -- with the
    model's values rounded to float32 first, as the device image holds them.  `margin` is then taken on the fused keys."""
    f = dtype
    lp = np.asarray(lp)
    T, C = lp.shape
    z = lp.astype(f)
    alpha, beta = f(alpha), f(beta)

    def grown(state, lm, c):
        """(lm(p + c), or -inf where g is: no such n-gram down to the empty context, dropped in step 5; state(p + c))"""
        bows, value, nxt = model.terms(state, c)
        if value is None:
            return NEG, nxt
        acc = f(0)
        for b in bows:
            acc = f(acc + f(b))
        g = f(acc + f(value))
        return f(lm + f(f(alpha * g) + beta)), nxt

    prefixes = [()]                                   # the beam, in descending order of what it is ranked by
    pb, pnb = np.zeros(1, dtype=f), np.full(1, NEG, dtype=f)
    if model is not None:
        states, lms = [model.start], [f(0)]
    margin, reentries = np.inf, 0
    for t in range(T):
        syms, gap = column_symbols(lp[t], top_classes, blank, unknown)
        margin = min(margin, gap)
        nb, kc = len(prefixes), len(syms)
        if nb == 0:
            break
        index = {p: i for i, p in enumerate(prefixes)}
        total = lse([pb, pnb])
        last = np.array([p[-1] if p else -1 for p in prefixes])
        # stay
        new_pb = (total + z[t, blank]).astype(f)
        new_pnb = np.where(last >= 0, pnb + z[t, np.maximum(last, 0)], np.asarray(NEG, dtype=f)).astype(f)
        # extend: [nb, kc]
        if kc:
            sym = np.array(syms)
            ext = (np.where(last[:, None] == sym[None, :], pb[:, None], total[:, None]) + z[t, sym][None, :]).astype(f)
        else:
            ext = np.zeros((nb, 0), dtype=f)
        if model is not None:
            ext_lm = np.zeros((nb, kc), dtype=f)
            ext_state = [[None] * kc for _ in range(nb)]
            for p in range(nb):
                for j in range(kc):
                    ext_lm[p, j], ext_state[p][j] = grown(states[p], lms[p], syms[j])
        # merge: an extension that spells a prefix of the beam joins its stay masses (one at most per prefix)
        for q, i in index.items():
            if q and q[:-1] in index and q[-1] in syms:
                p, j = index[q[:-1]], syms.index(q[-1])
                new_pnb[i] = lse([new_pnb[i:i + 1], ext[p:p + 1, j]])[0]
                ext[p, j] = NEG
        # keep: by total, with a model by total + lm
        ranked = np.concatenate([lse([new_pb, new_pnb]), ext.reshape(-1)])
        if model is not None:
            ranked = (ranked + np.concatenate([np.array(lms, dtype=f), ext_lm.reshape(-1)])).astype(f)
        order = np.argsort(-ranked, kind='stable')
        order = [int(k) for k in order if ranked[k] > NEG]
        if len(order) > beam:
            margin = min(margin, float(ranked[order[beam - 1]]) - float(ranked[order[beam]]))
        order = order[:beam]
        kept, kept_pb, kept_pnb, kept_state, kept_lm = [], [], [], [], []
        for k in order:
            if k < nb:
                kept.append(prefixes[k]); kept_pb.append(new_pb[k]); kept_pnb.append(new_pnb[k])
                if model is not None:
                    kept_state.append(states[k]); kept_lm.append(lms[k])
            else:
                p, j = divmod(k - nb, kc)
                kept.append(prefixes[p] + (syms[j],)); kept_pb.append(NEG); kept_pnb.append(ext[p, j])
                if model is not None:
                    kept_state.append(ext_state[p][j]); kept_lm.append(ext_lm[p, j])
        # a prefix that was not in the beam comes in beside a child of it that was and stays: it has been there before (the child
        # was made from it), and a decoder that does not give it its old identity back will not merge the two again
        was, now = set(prefixes), set(kept)
        reentries += sum(1 for s in kept if s not in was and any(q in was and q[:-1] == s for q in now if q))
        prefixes, states, lms = kept, kept_state, kept_lm
        pb, pnb = np.array(kept_pb, dtype=f), np.array(kept_pnb, dtype=f)
    total = lse([pb, pnb]) if prefixes else np.zeros(0, dtype=f)
    if model is None:
        hyps = [(p, total[i]) for i, p in enumerate(prefixes)][:nbest]
        decided = [h[1] for h in hyps]
    else:
        if end:
            lms = [f(lm + f(alpha * f(model.end(s)))) for lm, s in zip(lms, states)]
        ranked = [f(total[i] + lms[i]) for i in range(len(prefixes))]
        order = sorted(range(len(prefixes)), key=lambda i: -ranked[i])       # (stable: the beam's order among equal values)
        hyps = [(prefixes[i], ranked[i], total[i], lms[i]) for i in order[:nbest]]
        decided = [ranked[i] for i in order[:nbest + 1]]                     # the re-ranking also decides who is left out
    for a, b in zip(decided, decided[1:]):
        margin = min(margin, float(a) - float(b))
    return dict(hyps=hyps, margin=float(margin), reentries=reentries)


def decode(lp, beam, nbest, top_classes, blank=0, unknown=1, dtype=np.float64, model=None, alpha=0.0, beta=0.0, end=False):
    """All rows: lp f32 [N, T, C] -> a list of beam_search results."""
    return [beam_search(row, beam, nbest, top_classes, blank, unknown, dtype, model, alpha, beta, end) for row in lp]


def true_score(lp, string, blank=0, unknown=1):
    """log p(string | lp) in float64 over ALL alignments (the alpha recursion of _lexicon_ctc_ref): what a returned score may not
    exceed."""
    return float(word_score(np.asarray(lp), list(string), blank, np.float64, unknown))


def enumerate_strings(y, blank=0, unknown=1):
    """{string (tuple): log probability, float64} over all C^T paths of y [T, C] (probabilities); a path through `unknown` is
    excluded, a string of probability 0 is not listed."""
    y = np.asarray(y, dtype=np.float64)
    T, C = y.shape
    classes = [c for c in range(C) if c != unknown]
    out = {}
    for path in itertools.product(classes, repeat=T):
        p = 1.0
        for t, c in enumerate(path):
            p *= y[t, c]
        word, prev = [], None
        for c in path:
            if c != prev and c != blank:
                word.append(c)
            prev = c
        out[tuple(word)] = out.get(tuple(word), 0.0) + p
    return {w: float(np.log(p)) for w, p in out.items() if p > 0}


def posterior(rng, N, T, C, sharp=1.0):
    """softmax(sharp * normal): f32 [N, T, C] probabilities."""
    x = sharp * rng.standard_normal((N, T, C))
    e = np.exp(x - x.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)
