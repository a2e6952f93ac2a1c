"""The rules of the attention readers, checked on the numpy restatement alone (tests/_attn_ref.py; no GPU): the beam against
exhaustive enumeration, beam 1 against greedy decoding, the string score's summation rule, the moments of a one-hot map, and
the argument checks of TextReader(decode='attention')."""
import numpy as np
import pytest

import _attn_ref as ref

C, S, H, T, EP, BLANK = 3, 3, 8, 5, 6, 0


def _decoder(N, seed):
    g = np.random.default_rng(seed)
    return dict(cat_w=g.normal(size=(4 * H, H)) * 0.5, cat_b=g.normal(size=4 * H) * 0.1, eproj=g.normal(size=(N, T, H)),
                enc=g.normal(size=(N, T, EP)), v=g.normal(size=H), ic_w=g.normal(size=(3 * H, EP)) * 0.4,
                G=g.normal(size=(C, 3 * H)), out_w=g.normal(size=(C, H)) * 1.5, out_b=g.normal(size=C) * 0.3)


def test_a_wide_beam_is_exhaustive_enumeration():
    N, B = 3, 32                                       # 32 >= 27 word sequences: nothing is pruned
    p = _decoder(N, 11)
    ids, lengths, scores, count = ref.beam_search(p, S, BLANK, B, B)
    for n in range(N):
        want = ref.enumerate_strings(p, n, S, BLANK)
        assert len(want) == 15 == count[n]             # 8 strings of three symbols, 1 + 2 + 4 that a blank ends
        assert np.all(np.diff(scores[n, :15]) <= 0) and np.all(np.isneginf(scores[n, 15:]))
        for j, (string, ended, lp) in enumerate(want):
            assert tuple(ids[n, j, :lengths[n, j]]) == string and lengths[n, j] == len(string)
            assert ended == bool(np.all(ids[n, j, len(string):] == BLANK) and len(string) < S)
            assert abs(scores[n, j] - lp) < 1e-12
        assert abs(np.exp(scores[n, :15]).sum() - 1.0) < 1e-12           # the strings partition the probability


def test_beam_one_is_greedy_cut_at_the_first_blank():
    N = 6
    p = _decoder(N, 5)
    words, _, logits, _ = ref.greedy(p, S, BLANK)
    ids, lengths, scores, count = ref.beam_search(p, S, BLANK, 1, 1)
    assert np.all(count == 1)
    cut, _ = ref.string_score(np.zeros((N, S)), words, BLANK)
    assert len(set(cut.tolist())) > 1                                    # strings with and without a blank
    for n in range(N):
        k = int(cut[n])
        assert lengths[n, 0] == k and np.array_equal(ids[n, 0, :k], words[n, :k]) and np.all(ids[n, 0, k:] == BLANK)
    sym_lp = ref.log_softmax_at(logits.transpose(1, 0, 2), words, np.float64)
    _, want = ref.string_score(sym_lp, words, BLANK)
    assert np.allclose(scores[:, 0], want, rtol=0, atol=1e-12)


def test_score_is_the_sum_up_to_and_with_the_terminating_blank():
    sym_lp = np.log(np.array([[0.5, 0.25, 0.125, 0.5], [0.5, 0.25, 0.125, 0.5], [0.5, 0.25, 0.125, 0.5]]))
    words = np.array([[2, 1, 0, 2], [0, 0, 0, 0], [1, 2, 1, 2]], dtype=np.int32)
    length, score = ref.string_score(sym_lp, words, BLANK)
    assert length.tolist() == [2, 0, 4]
    assert np.allclose(np.exp(score), [0.5 * 0.25 * 0.125, 0.5, 0.5 * 0.25 * 0.125 * 0.5], rtol=1e-15)
    # the order is part of the rule: float32 sums are those of ascending s
    lp32 = np.array([[1e8, 1.0, -1e8, 1.0]], dtype=np.float32)
    _, s32 = ref.string_score(lp32, np.array([[1, 1, 1, 1]], dtype=np.int32), BLANK)
    assert s32.dtype == np.float32 and s32[0] == np.float32(1.0)          # ((1e8 + 1) - 1e8) + 1 in float32


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_moments_of_a_one_hot_map(dtype):
    height, width, Hh = 3, 7, 8
    Tn = height * width
    cells = [(0, 0), (6, 2), (3, 1)]
    # eproj[n, t] = +big on cell n's position, -big elsewhere: the energies differ by 2 * Hh * v * tanh(big) = 1600, and
    # exp(-1600) is 0 in either type
    eproj = np.full((len(cells), Tn, Hh), -20.0)
    for n, (x, y) in enumerate(cells):
        eproj[n, y * width + x] = 20.0
    out = ref.replay_read(np.zeros((2, len(cells), Hh)), eproj, np.full(Hh, 100.0), np.zeros((2, len(cells), 3)),
                          np.zeros((len(cells), 2), dtype=np.int32), BLANK, height, width, dtype=dtype)
    for n, (x, y) in enumerate(cells):
        assert out["att"][n, 0, y * width + x] == 1.0 and out["att"][n, 0].sum() == 1.0
        assert tuple(out["moments"][n, 1]) == ref.one_hot_moments(x, y)
    assert np.allclose(out["sym_lp"], np.log(1.0 / 3.0))


def test_text_reader_argument_checks():
    from megreader_amd import TextReader
    from megreader_amd.charsets import EnglishCharset

    class Reads(object):
        def read(self, crops, beam=1, nbest=1):
            raise AssertionError("not called")

    charset = EnglishCharset()
    with pytest.raises(ValueError, match="needs a recogniser with read"):
        TextReader(None, object(), charset, decode='attention')
    with pytest.raises(ValueError, match="beam_width"):
        TextReader(None, Reads(), charset, decode='attention', beam_width=2, nbest=3)
    with pytest.raises(ValueError, match="beam_width"):
        TextReader(None, Reads(), charset, decode='attention', nbest=2)                  # the default is greedy: one string
    with pytest.raises(ValueError, match="beam_width"):
        TextReader(None, Reads(), charset, decode='attention', beam_width=65)
    with pytest.raises(ValueError, match="needs decode='ctc'"):
        TextReader(None, Reads(), charset, decode='attention', lexicon=["A"], lexicon_rule='likelihood')
    with pytest.raises(ValueError, match="attention_extent"):
        TextReader(None, Reads(), charset, decode='attention', attention_extent=-1.0)
    with pytest.raises(ValueError, match="'attention'"):
        TextReader(None, Reads(), charset, decode='greedy')
    with pytest.raises(ValueError, match="chars=True"):
        TextReader(None, Reads(), charset, decode='ids', chars=True)
