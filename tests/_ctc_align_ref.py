"""numpy restatement of mr_ctc_align, written from the header comment (include/megreader_hip.h), not from the kernel.

    lp = log_table(y)                                   # [.., T, C] probabilities -> the f32 table of logs the kernel is defined on
    row = align_row(lp[n], target, blank, unknown, np.float32)
    out = align(lp, targets, lengths, blank, unknown, np.float32)       # the six outputs as arrays

The arithmetic is in the dtype asked for (np.float32: what the kernel does, bit for bit; np.float64: the truth over the same table),
with the header's tie rule: among equal candidates the smallest step wins.  `margin` (always float64) is the gap between the best
and the second-best alignment's score, inf when there is one alignment only.  `enumerate_alignments` walks all C^T paths."""
import itertools

import numpy as np


def log_table(y):
    """The f32 nearest to the f64 log of y; 0 -> -inf."""
    with np.errstate(divide='ignore'):
        return np.log(np.asarray(y).astype(np.float64)).astype(np.float32)


def alignable(target, C, T, blank, unknown):
    target = [int(s) for s in target]
    if any(s == blank or s == unknown or not 0 <= s < C for s in target):
        return False
    return len(target) + sum(a == b for a, b in zip(target, target[1:])) <= T


def dead_row(T, margin=None):
    return {'score': -np.inf, 'pos': np.full(T, -1, dtype=np.int32), 'begin': [], 'end': [], 'sym_lp': [], 'peak': [],
            'alive': False, 'margin': margin}


def align_row(lp, target, blank=0, unknown=1, dtype=np.float32, margin=False):
    """lp [T, C] (f32 table); target: the K symbols.  dict: score (dtype), pos i32 [T], begin / end / peak (K ints), sym_lp (K of
    dtype), alive, margin (float64 or None)."""
    lp = np.asarray(lp)
    T, C = lp.shape
    target = [int(s) for s in target]
    K = len(target)
    if not alignable(target, C, T, blank, unknown):
        return dead_row(T)
    table = lp.astype(dtype)
    ext = np.full(2 * K + 1, blank, dtype=np.int64)
    ext[1::2] = target
    P = 2 * K + 1
    hop = np.zeros(P, dtype=bool)                      # the s - 2 term: s odd and e[s] != e[s - 2]
    for s in range(3, P, 2):
        hop[s] = ext[s] != ext[s - 2]
    ninf = dtype(-np.inf)
    d = np.full(P, ninf, dtype=dtype)
    d[0] = table[0, blank]
    if K:
        d[1] = table[0, ext[1]]
    back = np.zeros((T, P), dtype=np.int8)
    for t in range(1, T):
        a = d
        b = np.concatenate([[ninf], d])[:P].astype(dtype)
        c = np.concatenate([[ninf, ninf], d])[:P].astype(dtype)
        best, step = a.copy(), np.zeros(P, dtype=np.int8)
        m = b > best                                    # strict: an equal candidate does not replace a smaller step
        best[m], step[m] = b[m], 1
        m = hop & (c > best)
        best[m], step[m] = c[m], 2
        d = (table[t, ext] + best).astype(dtype)        # one addition per cell
        back[t] = step
    if K == 0:
        s = 0
    else:
        s = 2 * K if d[2 * K] >= d[2 * K - 1] else 2 * K - 1
    score = d[s]
    gap = _margin(lp.astype(np.float64), ext, hop, K) if margin else None
    if not score > -np.inf:
        return dead_row(T, gap)
    pos = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        pos[t] = s
        s -= int(back[t, s])
    begin, end, sym_lp, peak = [], [], [], []
    for i in range(K):
        cols = np.nonzero(pos == 2 * i + 1)[0]
        assert len(cols) and np.all(np.diff(cols) == 1)
        begin.append(int(cols[0]))
        end.append(int(cols[-1]) + 1)
        acc = top = table[cols[0], target[i]]
        pk = int(cols[0])
        for t in cols[1:]:
            v = table[t, target[i]]
            acc = dtype(acc + v)
            if v > top:
                top, pk = v, int(t)
        sym_lp.append(acc)
        peak.append(pk)
    return {'score': score, 'pos': pos, 'begin': begin, 'end': end, 'sym_lp': sym_lp, 'peak': peak, 'alive': True, 'margin': gap}


def _margin(table, ext, hop, K):
    """float64: best minus second-best alignment score (two best DISTINCT paths per cell); inf when there is no second one."""
    T, P = table.shape[0], len(ext)
    cells = [[] for _ in range(P)]
    cells[0] = [table[0, ext[0]]]
    if K:
        cells[1] = [table[0, ext[1]]]
    for t in range(1, T):
        nxt = []
        for s in range(P):
            cand = list(cells[s])
            if s >= 1:
                cand += cells[s - 1]
            if hop[s]:
                cand += cells[s - 2]
            cand = sorted((v for v in cand if v > -np.inf), reverse=True)[:2]
            nxt.append([table[t, ext[s]] + v for v in cand if table[t, ext[s]] > -np.inf])
        cells = nxt
    final = list(cells[P - 1]) + (list(cells[P - 2]) if K else [])
    final = sorted((v for v in final if v > -np.inf), reverse=True)
    if not final:
        return 0.0
    return float(final[0] - final[1]) if len(final) > 1 else np.inf


def align(lp, targets, lengths, blank=0, unknown=1, dtype=np.float32, margin=False):
    """lp [N, T, C]; targets i32 [N, S]; lengths [N].  The six outputs as the entry point writes them (score and sym_lp in
    `dtype`), plus 'alive' bool [N] and 'margin' (list, None without `margin`)."""
    lp = np.asarray(lp)
    N, T, C = lp.shape
    targets = np.asarray(targets)
    S = targets.shape[1]
    out = {'score': np.full(N, -np.inf, dtype=dtype), 'pos': np.full((N, T), -1, dtype=np.int32),
           'begin': np.full((N, S), -1, dtype=np.int32), 'end': np.full((N, S), -1, dtype=np.int32),
           'sym_lp': np.full((N, S), -np.inf, dtype=dtype), 'peak': np.full((N, S), -1, dtype=np.int32),
           'alive': np.zeros(N, dtype=bool), 'margin': []}
    for n in range(N):
        K = int(lengths[n])
        if not 0 <= K <= S:
            out['margin'].append(None)
            continue
        row = align_row(lp[n], targets[n, :K], blank, unknown, dtype, margin)
        out['margin'].append(row['margin'])
        if not row['alive']:
            continue
        out['alive'][n] = True
        out['score'][n] = row['score']
        out['pos'][n] = row['pos']
        for key in ('begin', 'end', 'sym_lp', 'peak'):
            out[key][n, :K] = row[key]
    return out


def path_of(pos, target, blank):
    """The class of every column of an alignment given as positions."""
    return tuple(blank if s % 2 == 0 else int(target[s // 2]) for s in pos)


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return tuple(out)


def enumerate_alignments(lp, blank=0):
    """All C^T paths of the f32 table lp [T, C], scored in float64 (added in ascending t): {string: [(score, path), ...] sorted by
    descending score}, paths of probability zero left out."""
    table = np.asarray(lp).astype(np.float64)
    T, C = table.shape
    found = {}
    for path in itertools.product(range(C), repeat=T):
        score = table[0, path[0]]
        for t in range(1, T):
            score = score + table[t, path[t]]
        if score > -np.inf:
            found.setdefault(collapse(path, blank), []).append((float(score), path))
    for key in found:
        found[key].sort(key=lambda item: -item[0])
    return found
