"""Restatement in numpy of what the attention readers compute (include/megreader_hip.h: mr_attn_read, mr_attn_beam_step,
mr_attn_beam_trace; decoders/attention_decoder.py: AttentionDecoder.read): the replay read and the beam search, each in float64
(the truth the tests measure against) and in float32 with the kernels' order of summation (whose own error against float64 sets
the kernels' tolerance).  The decoder recurrence is the one of tests/test_decode_greedy_gpu.py:_f64, restated."""
import itertools

import numpy as np

LOG2E_X2 = 2.885390081777927        # 2 / ln 2: tanh x = 1 - 2 / (1 + 2^(x * 2 / ln 2)), the kernels' form


def tanh_of(x, dtype):
    if dtype == np.float64:
        return np.tanh(x)
    x = x.astype(np.float32)
    with np.errstate(over='ignore'):
        return (np.float32(1) - np.float32(2) / (np.float32(1) + np.exp2(x * np.float32(LOG2E_X2)))).astype(np.float32)


def lane_tree_sum(terms, lanes, dtype):
    """Sum over the last axis.  float64: plainly.  float32, the kernels' order: element k belongs to lane lanes[k]; a lane adds its
    elements in ascending k starting from 0, then the 64 lanes are added by the xor tree 32, 16, .., 1."""
    if dtype == np.float64:
        return terms.sum(-1)
    terms = terms.astype(np.float32)
    acc = np.zeros(terms.shape[:-1] + (64,), dtype=np.float32)
    order = np.zeros(64, dtype=np.int64)
    rounds = []
    for k, lane in enumerate(lanes):
        r = order[lane]
        order[lane] += 1
        if r == len(rounds):
            rounds.append(([], []))
        rounds[r][0].append(lane)
        rounds[r][1].append(k)
    for lane_r, k_r in rounds:
        acc[..., lane_r] = acc[..., lane_r] + terms[..., k_r]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., idx ^ o]
    return acc[..., 0]


def lanes_strided(K):
    return np.arange(K) % 64


def lanes_of_units(H, vec):
    """The lane of hidden unit h in the energy sum: 16-byte slices (vec elements) dealt round the lanes, or single elements."""
    return (np.arange(H) // vec) % 64 if H % vec == 0 else np.arange(H) % 64


def log_softmax_at(logits, words, dtype):
    """(l[w] - max) - log(sum exp(l - max)) along the last axis; -inf where the word is no class."""
    l = logits.astype(dtype)
    m = l.max(-1, keepdims=True)
    ls = np.log(lane_tree_sum(np.exp(l - m), lanes_strided(l.shape[-1]), dtype)).astype(dtype)
    ok = (words >= 0) & (words < l.shape[-1])
    picked = np.take_along_axis(l, np.where(ok, words, 0)[..., None], -1)[..., 0]
    with np.errstate(invalid='ignore'):
        return np.where(ok, (picked - m[..., 0]) - ls, -np.inf).astype(dtype)


def replay_read(hproj, eproj, v, logits, words, blank, height, width, dtype=np.float64, vec=8):
    """hproj [S, N, H], eproj [N, T, H], v [H], logits [S, N, C], words [N, S] -> dict(att [N, S, T], sym_lp [N, S], moments
    [N, S, 4], length [N], score [N]) in `dtype`."""
    S, N, H = hproj.shape
    T = eproj.shape[1]
    f = dtype
    hp, ep, vv = hproj.astype(f), eproj.astype(f), v.astype(f)
    x = hp.transpose(1, 0, 2)[:, :, None, :] + ep[:, None, :, :]                     # [N, S, T, H]
    e = lane_tree_sum(vv * tanh_of(x, f), lanes_of_units(H, vec), f)               # [N, S, T]
    ex = np.exp(e - e.max(-1, keepdims=True)).astype(f)
    lt = lanes_strided(T)
    att = (ex / lane_tree_sum(ex, lt, f)[..., None]).astype(f)
    t = np.arange(T)
    px, py = (t % width + 0.5).astype(f), (t // width + 0.5).astype(f)
    cx, cy = lane_tree_sum(att * px, lt, f), lane_tree_sum(att * py, lt, f)
    dx, dy = px - cx[..., None], py - cy[..., None]
    sx, sy = np.sqrt(lane_tree_sum(att * (dx * dx), lt, f)), np.sqrt(lane_tree_sum(att * (dy * dy), lt, f))
    sym_lp = log_softmax_at(logits.transpose(1, 0, 2), words[:, :S], f)             # [N, S]
    length, score = string_score(sym_lp, words[:, :S], blank)
    return dict(att=att, sym_lp=sym_lp, moments=np.stack([cx, cy, sx, sy], -1).astype(f), length=length, score=score)


def string_score(sym_lp, words, blank):
    """length[n] = the first blank of words[n] (S: none); score[n] = sym_lp[n, 0] + .. + sym_lp[n, min(length, S - 1)], added in
    that order in sym_lp's type."""
    N, S = words.shape
    length = np.array([next((s for s in range(S) if words[n, s] == blank), S) for n in range(N)], dtype=np.int32)
    score = np.empty(N, dtype=sym_lp.dtype)
    for n in range(N):
        total = sym_lp[n, 0]
        for s in range(1, min(int(length[n]), S - 1) + 1):
            total = total + sym_lp[n, s]
        score[n] = total
    return length, score


def one_hot_moments(x, y):
    """The moments of a map that is 1 at cell (x, y): the cell's centre, no spread."""
    return (x + 0.5, y + 0.5, 0.0, 0.0)


# ---- the decoder (float64; tests/test_decode_greedy_gpu.py:_f64 restated for one step) ----

def _sigmoid(x):
    return (1 / (1 + np.exp(-x))).astype(x.dtype)


def decoder_step(p, h, word, rows=None, dtype=np.float64):
    """One step of the attention GRU cell for the images `rows` (default: all, one hypothesis each).  p: float64 arrays cat_w
    [4H, H], cat_b [4H], eproj [N, T, H], enc [N, T, Ep], v [H], ic_w [3H, Ep], G [C, 3H], out_w [C, H], out_b [C]; h [R, H] the
    states, word [R] the words fed.  Returns (h' [R, H], logits [R, C], attention weights [R, T], hproj [R, H]).  dtype float32:
    every operand and operation in float32 (numpy's own order of summation: the precision of the kernels, not their bits)."""
    H = h.shape[1]
    rows = np.arange(h.shape[0]) if rows is None else rows
    if dtype != np.float64:
        p = {k: a.astype(dtype) for k, a in p.items()}
        h = h.astype(dtype)
    hc = h @ p["cat_w"].T + p["cat_b"]
    hproj, gh = hc[:, :H], hc[:, H:]
    e = np.tanh(hproj[:, None, :] + p["eproj"][rows]) @ p["v"]
    w = np.exp(e - e.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    ctx = np.einsum('rt,rte->re', w, p["enc"][rows])
    gi = p["G"][word] + ctx @ p["ic_w"].T
    r = _sigmoid(gi[:, :H] + gh[:, :H])
    z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    hn = (1 - z) * n + z * h
    return hn, hn @ p["out_w"].T + p["out_b"], w, hproj


def greedy(p, S, blank):
    """Greedy decoding, every step (no early stop): words [N, S] (the first of equal logits), H_all [S + 1, N, H], logits
    [S, N, C], hproj [S, N, H]."""
    N, H = p["eproj"].shape[0], p["eproj"].shape[2]
    h, word = np.zeros((N, H)), np.full(N, blank)
    H_all, words, logits, hprojs = [h], [], [], []
    for _ in range(S):
        h, lg, _, hp = decoder_step(p, h, word)
        word = lg.argmax(1)
        H_all.append(h); words.append(word); logits.append(lg); hprojs.append(hp)
    return np.stack(words, 1).astype(np.int32), np.stack(H_all), np.stack(logits), np.stack(hprojs)


def beam_step(logits, score, finished, length, s, blank, dtype=np.float64):
    """The selection of one step for ONE image (mr_attn_beam_step restated).  logits [B, C], score [B], finished [B], length [B]
    entering step s (s == 0: slot 0 live with score 0, whatever is passed).  Returns dict(parent, word, score, finished, length:
    [B] each, in slot order) and `values`: every candidate's value in descending order of selection followed by the best value
    that was NOT selected (or -inf), for a test's margins."""
    B, C = logits.shape
    f = dtype
    if s == 0:
        score = np.array([0.0] + [-np.inf] * (B - 1))
        finished, length = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int64)
    l = logits.astype(f)
    m = l.max(1, keepdims=True)
    ls = np.log(lane_tree_sum(np.exp(l - m), lanes_strided(C), f)).astype(f)
    cands = []
    for b in range(B):
        if not score[b] > -np.inf:
            continue
        if finished[b]:
            cands.append((f(score[b]), b * C + blank))
            continue
        if not m[b, 0] > -np.inf:
            continue
        val = (f(score[b]) + ((l[b] - m[b, 0]) - ls[b])).astype(f)
        cands.extend((val[c], b * C + c) for c in range(C) if val[c] > -np.inf)
    cands.sort(key=lambda vc: (-vc[0], vc[1]))                 # the greater value, then the smaller b * C + c
    out = dict(parent=np.zeros(B, np.int32), word=np.full(B, blank, np.int32), score=np.full(B, -np.inf, f),
               finished=np.zeros(B, np.int32), length=np.zeros(B, np.int32))
    for j, (val, e) in enumerate(cands[:B]):
        b, c = divmod(e, C)
        out["parent"][j], out["word"][j], out["score"][j] = b, c, val
        out["finished"][j] = int(finished[b] or c == blank)
        out["length"][j] = length[b] if finished[b] else (s if c == blank else s + 1)
    out["values"] = [vc[0] for vc in cands[:B + 1]] + ([-np.inf] if len(cands) <= B else [])
    return out


def beam_search(p, S, blank, B, nbest, dtype=np.float64):
    """Beam search with the decoder and the selection arithmetic in `dtype`.  Returns (ids [N, nbest, S] blank padded,
    lengths [N, nbest], scores [N, nbest] descending, count [N])."""
    N, H = p["eproj"].shape[0], p["eproj"].shape[2]
    ids = np.full((N, nbest, S), blank, dtype=np.int32)
    lengths = np.zeros((N, nbest), dtype=np.int32)
    scores = np.full((N, nbest), -np.inf, dtype=dtype)
    count = np.zeros(N, dtype=np.int32)
    for n in range(N):
        h, feed = np.zeros((B, H)), np.full(B, blank)
        st = dict(score=None, finished=None, length=None)
        parents, words = [], []
        for s in range(S):
            hn, lg, _, _ = decoder_step(p, h, feed, rows=np.full(B, n), dtype=dtype)
            st = beam_step(lg, st["score"], st["finished"], st["length"], s, blank, dtype)
            parents.append(st["parent"]); words.append(st["word"])
            h, feed = hn[st["parent"]], st["word"].astype(np.int64)
        for j in range(nbest):
            if not st["score"][j] > -np.inf:
                continue
            count[n] += 1
            scores[n, j] = st["score"][j]
            lengths[n, j] = st["length"][j] if st["finished"][j] else S
            cur = j
            for s in range(S - 1, -1, -1):
                ids[n, j, s] = words[s][cur]
                cur = parents[s][cur]
    return ids, lengths, scores, count


def enumerate_strings(p, n, S, blank):
    """Every string image n can be read as, with its log-probability, by enumeration of all C^S word sequences of the float64
    decoder: a sequence counts up to its first blank (what follows sums to one), so sequences with the same blank-terminated
    prefix are one string.  [(words before the blank as a tuple, ended by a blank?, log-probability)], descending."""
    C = p["out_w"].shape[0]
    H = p["eproj"].shape[2]
    found = {}
    for seq in itertools.product(range(C), repeat=S):
        h, feed, lp = np.zeros((1, H)), np.array([blank]), 0.0
        key = None
        for s, w in enumerate(seq):
            h, lg, _, _ = decoder_step(p, h, feed, rows=np.array([n]))
            lg = lg[0] - lg[0].max()
            lp += lg[w] - np.log(np.exp(lg).sum())
            feed = np.array([w])
            if w == blank:
                key = (tuple(seq[:s]), True)
                break
        if key is None:
            key = (tuple(seq), False)
        found.setdefault(key, lp)
    return sorted(((k[0], k[1], v) for k, v in found.items()), key=lambda r: -r[2])
