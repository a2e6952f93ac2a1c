"""The restatement of lexicon transcription by CTC likelihood (tests/_lexicon_ctc_ref.py) against two independent computations:
brute-force enumeration of every path, and torch's ctc_loss on the CPU in float64.  No GPU."""
import numpy as np
import torch

import _lexicon_ctc_ref as Q


def softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def test_float64_restatement_equals_enumeration_of_all_paths():
    rng = np.random.RandomState(0)
    words = [[], [1], [2], [1, 1], [1, 2], [2, 2, 1], [1, 2, 1], [3, 3], [1, 1, 1], [1, 2, 3, 1], [2, 1, 2, 1, 2], [1, 1, 1, 1],
             [1, 2, 3, 2, 1, 3]]                                   # K = 0, repeats, K == T, K > T
    for T, C, zeros in ((1, 3, False), (2, 4, False), (3, 4, True), (4, 4, True), (5, 3, False), (5, 4, True)):
        y = softmax(rng.randn(T, C))
        if zeros:                                                # exact zeros: a whole class in one column, the blank in another
            y[T // 2, 1] = 0.0
            y[0, 0] = 0.0
            y /= y.sum(axis=1, keepdims=True)
        paths = Q.brute_force(y, blank=0)
        assert abs(sum(paths.values()) - 1.0) < 1e-12
        lp = Q.log_probs(y, np.float64)
        for w in (w for w in words if all(s < C for s in w)):
            want = paths.get(tuple(w), 0.0)
            got = Q.word_score(lp, w, blank=0, dtype=np.float64)
            assert not np.isnan(got)
            if want == 0.0:
                assert got == -np.inf, (T, C, w, got)
            else:
                assert abs(np.exp(got) - want) <= 1e-12 * want, (T, C, w, got, np.log(want))
        assert Q.word_score(lp, [1] * (T + 1), 0) == -np.inf       # cannot fit
        if T >= 2:
            assert Q.word_score(lp, [1, 1] + [2] * (T - 2), 0) == -np.inf   # K == T with a repeat: one column short


def test_float64_restatement_equals_minus_ctc_loss():
    rng = np.random.RandomState(1)
    N, T, C, L = 6, 32, 38, 60
    for blank in (0, 5):
        y = softmax(rng.randn(N, T, C) * 3.0)
        lp = Q.log_probs(y, np.float64)
        ids = [i for i in range(C) if i != blank]
        words = [rng.choice(ids, size=k).tolist() for k in rng.randint(0, 13, size=L)]
        words[3] = [7, 7, 7, 7]
        words[4] = [9] * 17                                      # 17 symbols + 16 repeats > 32 columns
        S = Q.score_table(lp, words, blank=blank)
        logp = torch.from_numpy(lp).permute(1, 0, 2).contiguous()  # [T, N, C]
        for l, w in enumerate(words):
            target = torch.tensor([w] * N, dtype=torch.long).reshape(N, len(w))
            loss = torch.nn.functional.ctc_loss(logp, target, torch.full((N,), T, dtype=torch.long),
                                                torch.full((N,), len(w), dtype=torch.long), blank=blank, reduction='none')
            want = -loss.numpy()
            if l == 4:
                assert np.all(S[:, l] == -np.inf) and np.all(np.isinf(want))
            else:
                assert np.all(np.abs(S[:, l] - want) <= 1e-9), (l, w, S[:, l], want)


def test_float32_restatement_is_the_same_rule_rounded():
    rng = np.random.RandomState(2)
    y = softmax(rng.randn(5, 32, 38) * 4.0).astype(np.float32)
    words = [rng.randint(2, 38, size=k).tolist() for k in rng.randint(0, 13, size=40)]
    S64 = Q.score_table(Q.log_probs(y, np.float64), words)
    S32 = Q.score_table(Q.log_probs(y, np.float32), words, dtype=np.float32)
    assert S32.dtype == np.float32 and np.array_equal(np.isfinite(S32), np.isfinite(S64))
    fin = np.isfinite(S64)
    e32 = np.abs(S32[fin].astype(np.float64) - S64[fin]).max()
    print("e32 = %.3g at scores down to %.1f" % (e32, S64[fin].min()))
    assert 0 < e32 < 1e-5 * np.abs(S64[fin]).max()


def test_unknown_and_out_of_range_symbols_match_nothing():
    lp = Q.log_probs(softmax(np.random.RandomState(3).randn(6, 5)), np.float64)
    assert Q.word_score(lp, [2, 1, 3], blank=0, unknown=1) == -np.inf
    assert Q.word_score(lp, [2, 5], blank=0) == -np.inf and Q.word_score(lp, [-1], blank=0) == -np.inf
    assert np.isfinite(Q.word_score(lp, [2, 1, 3], blank=0))       # without an `unknown` id, 1 is a class like any other


def test_fold_rule_on_a_four_class_toy():
    """Classes: 0 blank, 1 unknown, 2 'A', 3 'a' -> 'A'.  The folded likelihood of "A" counts every path over {A, a}."""
    fold = [0, 1, 2, 2]
    y = softmax(np.random.RandomState(4).randn(4, 4))
    q = Q.fold_posterior(y, fold)
    assert np.allclose(q[:, 2], y[:, 2] + y[:, 3]) and np.all(q[:, 3] == 0) and np.allclose(q.sum(axis=1), 1.0)
    # every path over the four classes, folded symbol by symbol and THEN collapsed: "Aa" in adjacent columns is one run of A
    want = {}
    for code in range(4 ** 4):
        path = [(code // 4 ** t) % 4 for t in range(4)]
        p = float(np.prod([y[t, c] for t, c in enumerate(path)]))
        word, prev = [], None
        for c in (fold[c] for c in path):
            if c != prev and c != 0:
                word.append(c)
            prev = c
        want[tuple(word)] = want.get(tuple(word), 0.0) + p
    for folded in ([2], [2, 2], [], [2, 1], [1, 2, 1]):
        got = Q.word_score(Q.log_probs(q, np.float64), folded, blank=0)
        assert abs(np.exp(got) - want[tuple(folded)]) <= 1e-12, folded
    assert np.exp(Q.word_score(Q.log_probs(q, np.float64), [2], 0)) > Q.brute_force(y)[(2,)] + Q.brute_force(y)[(3,)]
    qlog = Q.fold_posterior(np.log(y), fold, log=True)
    assert np.allclose(np.exp(qlog), q) and np.all(qlog[:, 3] == -np.inf)


def test_selection_lowest_index_on_ties_and_no_finite_candidate():
    S = np.array([[-3.0, -1.0, -1.0, -np.inf], [-np.inf] * 4, [-2.0, -5.0, -1.0, -0.5]])
    D = np.array([[0, 2, 1, 0], [0, 0, 0, 0], [3, 1, 2, 4]])
    got = Q.transcribe(S, D, [4, 0, 3])
    assert got['index'].tolist() == [1, -1, 3] and got['distance'].tolist() == [2, -1, 4]
    assert got['candidates'].tolist() == [4, 4, 4] and got['score'].tolist() == [-1.0, -np.inf, -0.5]
    got = Q.transcribe(S, D, [4, 0, 3], max_distance=1)
    assert got['index'].tolist() == [2, -1, 1] and got['candidates'].tolist() == [3, 4, 1]
    got = Q.transcribe(S, D, [4, 0, 3], spans=[[3, 4], [1, 1], [0, 2]], max_distance=2)
    assert got['index'].tolist() == [-1, -1, 1] and got['candidates'].tolist() == [1, 0, 1]
    assert got['scores'][2].tolist() == [-np.inf, -5.0, -np.inf, -np.inf]


def test_greedy_restatement():
    y = np.zeros((1, 8, 5))
    for t, c in enumerate([0, 2, 2, 1, 2, 0, 2, 3]):             # the unknown (1) between two 2s does not separate them
        y[0, t, c] = 1.0
    assert Q.greedy(y)[0].tolist() == [2, 2, 3, 0, 0, 0, 0, 0]
