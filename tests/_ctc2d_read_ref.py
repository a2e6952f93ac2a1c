"""Pure numpy restatement of mr_ctc2d_marginal and mr_ctc2d_char_rows, written from their description in include/megreader_hip.h
-- not from the kernels -- with the same operations in the same order in float32: every product an np.float32 product rounded on
its own, the reduction a loop over h in ascending order (not np.sum, whose order is numpy's own), the log taken in float64 and
rounded once.  The kernels are held to these bit for bit."""
import numpy as np


def marginal(classify, mask, reduce='sum', log=False):
    """classify [N, C, H, W], mask [N, 1, H, W] (values that float32 holds exactly) -> float32 [N, C, W]."""
    cl = np.asarray(classify).astype(np.float32)
    mk = np.asarray(mask).astype(np.float32)
    N, C, H, W = cl.shape
    assert mk.shape == (N, 1, H, W)
    acc = np.zeros((N, C, W), dtype=np.float32)
    for h in range(H):
        prod = (cl[:, :, h, :] * mk[:, :, h, :]).astype(np.float32)          # one float32 rounding per product
        if h == 0:
            acc = prod
        elif reduce == 'max':
            acc = np.fmax(acc, prod)
        else:
            acc = (acc + prod).astype(np.float32)                              # one float32 addition per height
    if log:
        with np.errstate(divide='ignore'):
            acc = np.log(acc.astype(np.float64)).astype(np.float32)
    return acc


def char_rows(classify, mask, targets, lengths, pos, begin, end, blank=0):
    """rows int32 [N, W], row_lo and row_hi int32 [N, S] from pos [N, W], begin and end [N, S] as mr_ctc_align writes them."""
    cl = np.asarray(classify).astype(np.float32)
    mk = np.asarray(mask).astype(np.float32)
    N, C, H, W = cl.shape
    targets = np.asarray(targets, dtype=np.int32)
    S = targets.size // max(N, 1)
    targets = targets.reshape(N, S)
    rows = np.full((N, W), -1, dtype=np.int32)
    lo = np.full((N, S), -1, dtype=np.int32)
    hi = np.full((N, S), -1, dtype=np.int32)
    for n in range(N):
        K = min(max(int(lengths[n]), 0), S)
        for w in range(W):
            s = int(pos[n][w])
            if not 0 <= s <= 2 * K:
                continue
            c = int(targets[n, s // 2]) if s % 2 else blank
            if not 0 <= c < C:
                continue
            best, at = None, -1
            for h in range(H):
                prod = np.float32(cl[n, c, h, w]) * np.float32(mk[n, 0, h, w])
                if h == 0 or prod > best:                                      # strictly greater: the lowest h of equal values
                    best, at = prod, h
            rows[n, w] = at
        for i in range(K):
            b, e = int(begin[n][i]), int(end[n][i])
            if 0 <= b < e <= W:
                lo[n, i] = rows[n, b:e].min()
                hi[n, i] = rows[n, b:e].max()
    return {'rows': rows, 'row_lo': lo, 'row_hi': hi}


def tie_free(classify, mask):
    """Whether no two products of a column are equal where it matters to a greedy decode: the greatest product of every (n, w)
    over (c, h) is attained once."""
    heat = (np.asarray(classify, dtype=np.float32) * np.asarray(mask, dtype=np.float32)).astype(np.float32)
    N, C, H, W = heat.shape
    flat = np.sort(heat.transpose(0, 3, 1, 2).reshape(N, W, C * H), axis=2)
    return bool(np.all(flat[:, :, -1] > flat[:, :, -2])) if C * H > 1 else True


def greedy_cases(count=50, shape=(3, 6, 4, 9), seed=0):
    """The seeded random heads of the greedy tests: [(classify [N, C, H, W], mask [N, 1, H, W])] in float32, softmax over the
    classes and over the heights."""
    rng = np.random.RandomState(seed)
    N, C, H, W = shape
    out = []
    for _ in range(count):
        z = rng.randn(N, C, H, W) * 2.0
        a = rng.randn(N, 1, H, W) * 2.0
        cl = np.exp(z - z.max(axis=1, keepdims=True))
        cl /= cl.sum(axis=1, keepdims=True)
        mk = np.exp(a - a.max(axis=2, keepdims=True))
        mk /= mk.sum(axis=2, keepdims=True)
        out.append((cl.astype(np.float32), mk.astype(np.float32)))
    return out
