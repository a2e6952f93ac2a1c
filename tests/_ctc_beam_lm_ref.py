"""Pure numpy restatement of CTC prefix beam search with a character n-gram model, written from the description of
mr_ctc_beam_search_lm (include/megreader_hip.h) -- not from the kernel: `beam_search` of _ctc_beam_ref.py with a model state and a
sum lm per hypothesis.  The masses stay the pure CTC ones; only step 5 and the final order read total + lm.  `model` is anything
with `start`, `terms(state, c) -> ([backoff weights in the order met], the n-gram's value or None, next state)` and `end(state)`
(_ngram_lm_ref.DictLM: the state is the history itself).  Every value is held in `dtype`: float64 is the truth, float32 follows
the header's order -- acc = 0, acc += bow .., g = acc + value; lm += (alpha * g + beta), each operation rounded -- with the
model's values rounded to float32 first, as the device image holds them.  `margin` is taken on the fused keys."""
import numpy as np

from _ctc_beam_ref import column_symbols
from _lexicon_ctc_ref import NEG, lse


def beam_search(lp, model, alpha, beta, end, beam, nbest, top_classes, blank=0, unknown=1, dtype=np.float64):
    """One row.  lp: [T, C].  Returns dict(hyps=[(tuple of ids, score, ctc_score, lm_score)] -- at most nbest, descending by score
    --, margin)."""
    f = dtype
    lp = np.asarray(lp)
    T, C = lp.shape
    z = lp.astype(f)
    alpha, beta = f(alpha), f(beta)

    def grown(state, lm, c):
        """(lm(p + c) or None when g is -inf, state(p + c))"""
        bows, value, nxt = model.terms(state, c)
        if value is None:
            return None, nxt
        acc = f(0)
        for b in bows:
            acc = f(acc + f(b))
        g = f(acc + f(value))
        return f(lm + f(f(alpha * g) + beta)), nxt

    prefixes, states, lms = [()], [model.start], [f(0)]
    pb, pnb = np.zeros(1, dtype=f), np.full(1, NEG, dtype=f)
    margin = np.inf
    for t in range(T):
        syms, gap = column_symbols(lp[t], top_classes, blank, unknown)
        margin = min(margin, gap)
        nb, kc = len(prefixes), len(syms)
        if nb == 0:
            break
        index = {p: i for i, p in enumerate(prefixes)}
        total = lse([pb, pnb])
        last = np.array([p[-1] if p else -1 for p in prefixes])
        new_pb = (total + z[t, blank]).astype(f)
        new_pnb = np.where(last >= 0, pnb + z[t, np.maximum(last, 0)], np.asarray(NEG, dtype=f)).astype(f)
        if kc:
            sym = np.array(syms)
            ext = (np.where(last[:, None] == sym[None, :], pb[:, None], total[:, None]) + z[t, sym][None, :]).astype(f)
        else:
            ext = np.zeros((nb, 0), dtype=f)
        ext_lm = np.zeros((nb, kc), dtype=f)
        ext_state = [[None] * kc for _ in range(nb)]
        for p in range(nb):
            for j in range(kc):
                lm, ext_state[p][j] = grown(states[p], lms[p], syms[j])
                ext_lm[p, j] = NEG if lm is None else lm     # no such n-gram down to the empty context: dropped in step 5
        for q, i in index.items():
            if q and q[:-1] in index and q[-1] in syms:
                p, j = index[q[:-1]], syms.index(q[-1])
                new_pnb[i] = lse([new_pnb[i:i + 1], ext[p:p + 1, j]])[0]
                ext[p, j] = NEG
        stay = lse([new_pb, new_pnb])
        ranked = np.concatenate([(stay + np.array(lms, dtype=f)).astype(f), (ext + ext_lm).astype(f).reshape(-1)])
        order = np.argsort(-ranked, kind='stable')
        order = [int(k) for k in order if ranked[k] > NEG]
        if len(order) > beam:
            margin = min(margin, float(ranked[order[beam - 1]]) - float(ranked[order[beam]]))
        order = order[:beam]
        kept, kept_pb, kept_pnb, kept_state, kept_lm = [], [], [], [], []
        for k in order:
            if k < nb:
                kept.append(prefixes[k]); kept_pb.append(new_pb[k]); kept_pnb.append(new_pnb[k])
                kept_state.append(states[k]); kept_lm.append(lms[k])
            else:
                p, j = divmod(k - nb, kc)
                kept.append(prefixes[p] + (syms[j],)); kept_pb.append(NEG); kept_pnb.append(ext[p, j])
                kept_state.append(ext_state[p][j]); kept_lm.append(ext_lm[p, j])
        prefixes, states, lms = kept, kept_state, kept_lm
        pb, pnb = np.array(kept_pb, dtype=f), np.array(kept_pnb, dtype=f)
    total = lse([pb, pnb]) if prefixes else np.zeros(0, dtype=f)
    if end:
        lms = [f(lm + f(alpha * f(model.end(s)))) for lm, s in zip(lms, states)]
    ranked = [f(total[i] + lms[i]) for i in range(len(prefixes))]
    order = sorted(range(len(prefixes)), key=lambda i: -ranked[i])           # (stable: the beam's order among equal values)
    for a, b in zip(order[:nbest], order[1:nbest + 1]):
        margin = min(margin, float(ranked[a]) - float(ranked[b]))
    hyps = [(prefixes[i], ranked[i], total[i], lms[i]) for i in order[:nbest]]
    return dict(hyps=hyps, margin=float(margin))


def decode(lp, model, alpha, beta, end, beam, nbest, top_classes, blank=0, unknown=1, dtype=np.float64):
    """All rows: lp f32 [N, T, C] -> a list of beam_search results."""
    return [beam_search(row, model, alpha, beta, end, beam, nbest, top_classes, blank, unknown, dtype) for row in lp]
