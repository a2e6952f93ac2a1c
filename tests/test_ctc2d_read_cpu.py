"""What reading a 2D-CTC head with the 1-D readers rests on, checked without a GPU (megreader_amd/ops/decode.py: ctc2d_marginal,
ctc2d_char_rows; the kernels are held to tests/_ctc2d_read_ref.py in tests/test_ctc2d_read_gpu.py):

  1. the 2D-CTC recursion sums alpha over the heights of the previous column before every step, so its log-likelihood is the 1-D
     CTC log-likelihood of q = sum_h classify * mask -- oracle/ctc2d.py (pinned to the reference) against the float64 alpha of
     tests/_lexicon_ctc_ref.py on the float64 marginal, to 1e-12 relative (measured: 1e-15);
  2. greedy decoding of max_h classify * mask is the reference's 2-D greedy rule where no two products tie;
  3. the restatement of the heights of an alignment on a hand-built case;
  4. one height: the marginal is the product, the heights are all 0."""
import numpy as np
import pytest

import _ctc2d_read_ref as R
import _lexicon_ctc_ref as Q
from oracle import ctc2d as O
from oracle import decode as D

SHAPES = [(5, 1, 3, 4), (7, 3, 4, 5), (16, 4, 5, 38), (12, 8, 3, 2)]          # (T, H, N, C)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_2d_likelihood_is_the_1d_likelihood_of_the_sum_marginal(shape):
    T, H, N, C = shape
    rng = np.random.RandomState(T * 100 + C)
    lp = O.synthetic_lp(T, H, N, C, seed=T + H)[0].astype(np.float64)          # [T, H, N, C], log(mask * classify)
    input_lengths = np.array([T if n % 2 == 0 else max(2, T - 1 - n) for n in range(N)])
    assert (input_lengths < T).any() and (input_lengths == T).any()
    S = 8
    # lengths >= 1 that fit the row's columns even when every symbol repeats (C = 2 has one symbol: L + (L - 1) columns)
    target_lengths = np.array([rng.randint(1, min(S, (tb + 1) // 2) + 1) for tb in input_lengths])
    targets = rng.randint(1, C, size=(N, S))
    nll = O.ctc2d(lp, targets, input_lengths, target_lengths, blank=0)['nll']
    with np.errstate(divide='ignore'):
        q = np.log(np.exp(lp).sum(axis=1))                                     # [T, N, C]: the float64 sum-marginal, its log
    worst = 0.0
    for n in range(N):
        want = Q.word_score(q[:input_lengths[n], n, :], targets[n, :target_lengths[n]], blank=0, dtype=np.float64)
        assert np.isfinite(want) and np.isfinite(nll[n])
        worst = max(worst, abs(-nll[n] - want) / abs(want))
    print("T=%d H=%d N=%d C=%d lengths %s: max relative difference %.3g" % (T, H, N, C, target_lengths.tolist(), worst))
    assert worst <= 1e-12


def test_the_empty_target_is_the_documented_exception():
    """The reference's recursion does not run for L = 0: only column 0 counts; the 1-D readers give the all-blank probability."""
    lp = O.synthetic_lp(6, 3, 2, 5, seed=1)[0].astype(np.float64)
    nll = O.ctc2d(lp, np.zeros((2, 2), dtype=np.int64), [6, 6], [0, 0])['nll']
    q = np.log(np.exp(lp).sum(axis=1))
    all_blank = np.array([Q.word_score(q[:, n, :], [], blank=0) for n in range(2)])
    assert np.all(np.isfinite(all_blank)) and not np.allclose(-nll, all_blank, rtol=1e-3)


def test_greedy_of_the_max_marginal_is_the_2d_greedy_rule():
    cases = R.greedy_cases(50, (3, 6, 4, 9), seed=0)
    mismatches = 0
    for cl, mk in cases:
        assert R.tie_free(cl, mk)
        m = R.marginal(cl, mk, reduce='max')
        got = D.greedy_decode(m[:, :, None, :])
        want = D.greedy_decode_2d(cl, mk)
        mismatches += int(not np.array_equal(got, want))
    assert mismatches == 0


def hand_built():
    """One row, W = 9, H = 4, C = 5 (blank 0): the word [2, 3, 2] on the path b 2 2 b 3 3 3 2 b.  Every named class has its mass on
    one height per column, which changes along the word: symbol 0 on heights 1 then 3, symbol 1 on 2, 2, 0, symbol 2 on 1; the
    blanks on 0, 3 and, a tie of all heights, the lowest.  The other classes peak elsewhere and must not be looked at."""
    C, H, W = 5, 4, 9
    path_class = [0, 2, 2, 0, 3, 3, 3, 2, 0]
    path_height = [0, 1, 3, 3, 2, 2, 0, 1, 0]
    cl = np.full((1, C, H, W), 0.05, dtype=np.float32)
    mk = np.full((1, 1, H, W), 0.25, dtype=np.float32)
    for w, (c, h) in enumerate(zip(path_class, path_height)):
        if w == W - 1:
            continue                                                           # the last blank: every height equal, h = 0 wins
        cl[0, c, h, w] = 0.8
        cl[0, 4, (h + 1) % H, w] = 0.9                                         # a class the string does not name, higher still
    pos = np.array([[0, 1, 1, 2, 3, 3, 3, 5, 6]], dtype=np.int32)
    begin = np.array([[1, 4, 7, -1]], dtype=np.int32)
    end = np.array([[3, 7, 8, -1]], dtype=np.int32)
    targets = np.array([[2, 3, 2, 4]], dtype=np.int32)
    return cl, mk, targets, np.array([3]), pos, begin, end, path_height


def test_rows_restatement_on_a_hand_built_case():
    cl, mk, targets, lengths, pos, begin, end, heights = hand_built()
    got = R.char_rows(cl, mk, targets, lengths, pos, begin, end)
    assert got['rows'].tolist() == [heights]
    assert got['row_lo'].tolist() == [[1, 0, 1, -1]] and got['row_hi'].tolist() == [[3, 2, 1, -1]]
    # a tie between two heights of a symbol's column: the lowest h
    cl[0, 3, 3, 4] = cl[0, 3, 2, 4]
    cl[0, 3, 1, 5] = cl[0, 3, 2, 5]
    tied = R.char_rows(cl, mk, targets, lengths, pos, begin, end)
    assert tied['rows'][0].tolist() == [0, 1, 3, 3, 2, 1, 0, 1, 0] and tied['row_lo'][0, 1] == 0 and tied['row_hi'][0, 1] == 2
    # an unaligned row (pos -1, empty slots) and a length outside the string
    none = R.char_rows(cl, mk, targets, lengths, np.full_like(pos, -1), np.full_like(begin, -1), np.full_like(end, -1))
    assert np.all(none['rows'] == -1) and np.all(none['row_lo'] == -1) and np.all(none['row_hi'] == -1)
    short = R.char_rows(cl, mk, targets, np.array([1]), pos, begin, end)       # K = 1: positions above 2 name nothing
    assert short['rows'][0].tolist() == [0, 1, 3, 3, -1, -1, -1, -1, -1] and short['row_lo'][0].tolist() == [1, -1, -1, -1]


def test_one_height():
    rng = np.random.RandomState(3)
    cl = rng.rand(2, 5, 1, 7).astype(np.float32)
    mk = rng.rand(2, 1, 1, 7).astype(np.float32)
    for reduce in ('sum', 'max'):
        assert np.array_equal(R.marginal(cl, mk, reduce), (cl * mk)[:, :, 0, :])
    with np.errstate(divide='ignore'):
        assert np.array_equal(R.marginal(cl, mk, 'sum', log=True), np.log((cl * mk)[:, :, 0, :].astype(np.float64)).astype(np.float32))
    pos = np.tile(np.array([0, 1, 1, 2, 3, 4, 4], dtype=np.int32), (2, 1))
    begin, end = np.array([[1, 4]] * 2, dtype=np.int32), np.array([[3, 5]] * 2, dtype=np.int32)
    got = R.char_rows(cl, mk, np.array([[2, 3]] * 2), np.array([2, 2]), pos, begin, end)
    assert np.all(got['rows'] == 0) and np.all(got['row_lo'] == 0) and np.all(got['row_hi'] == 0)


def test_the_sum_is_in_ascending_h_in_float32():
    """Three heights whose float32 sum depends on the order: (1 + 2^-24) + 2^-24 rounds to 1 twice, 2^-24 + 2^-24 + 1 does not."""
    cl = np.array([1.0, 2.0 ** -24, 2.0 ** -24], dtype=np.float32).reshape(1, 1, 3, 1)
    mk = np.ones((1, 1, 3, 1), dtype=np.float32)
    assert R.marginal(cl, mk)[0, 0, 0] == np.float32(1.0)
    assert R.marginal(cl[:, :, ::-1], mk)[0, 0, 0] == np.float32(1.0) + np.float32(2.0 ** -23)
