"""`CharNgramLM` (megreader_amd/ops/language_model.py) on the host: the automaton against a dict-of-n-grams scorer written from the
ARPA definition (tests/_ngram_lm_ref.py), the device image against a lookup that follows the header's hash rule, training, the
ARPA round trip, the refusals -- and the restatement of mr_ctc_beam_search_lm (tests/_ctc_beam_ref.py, with a model) against enumeration of
every path plus the model's own score.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import _ctc_beam_ref as B
import _ngram_lm_ref as R
from megreader_amd import _lib
from megreader_amd.charsets import Charset
from megreader_amd.ops.language_model import BOS, EOS, CharNgramLM, arc_hash

CHARSET = Charset("abeht ", case_sensitive=True)        # blank 0, unknown 1, ' ' 2, a 3, b 4, e 5, h 6, t 7

ARPA3 = """
\\data\\
ngram 1=7
ngram 2=6
ngram 3=3

\\1-grams:
-99 <s> -0.5
-0.9 </s>
-0.8 t -0.4
-0.7 h -0.3
-0.6 e -0.2
-1.2 b
-1.5 <space> -0.1

\\2-grams:
-0.3 <s> t -0.25
-0.2 t h -0.15
-0.9 t b
-0.1 h e -0.05
-0.4 e </s>
-0.6 e <space>

\\3-grams:
-0.05 <s> t h
-0.02 t h e
-0.3 h e </s>

\\end\\
"""


def dict_model(lm, text=None):
    """The dict scorer of the same model: from ARPA text where one is given, else from the class's n-gram dict (the same tokens)."""
    if text is not None:
        ngrams, order, unk = R.parse_arpa(text, lm.charset.index)
    else:
        ngrams, order, unk = lm.ngrams, lm.order, None
    return R.DictLM(ngrams, order, lm.eligible(), unk)


def walk(lm, ctx):
    """The automaton's state after the tokens of `ctx` (a leading BOS: from the start state)."""
    state = lm.start_state if ctx[:1] == (BOS,) else 0
    for c in ctx[1:] if ctx[:1] == (BOS,) else ctx:
        state = lm.step(state, c)[1]
    return state


def contexts(lm, longest):
    for n in range(longest + 1):
        for ctx in itertools.product(lm.eligible(), repeat=n):
            yield ctx
            if n < longest and (BOS,) in lm.ngrams:
                yield (BOS,) + ctx


def test_hand_written_arpa_equals_the_dict_scorer():
    lm = CharNgramLM.from_arpa(ARPA3, CHARSET)
    ref = dict_model(lm, ARPA3)
    assert (lm.order, lm.skipped, lm.start_state) == (3, 0, lm.state_of[(BOS,)])
    assert lm.states == 1 + 6 + 5 and lm.backoff[0] == -1          # every listed n-gram below the order without </s>: a bow of 0 counts
    assert lm.floor == pytest.approx(-1.5 * math.log(10))         # 'a' is not listed: the smallest unigram value
    seen_levels = set()
    for ctx in contexts(lm, 3):                                   # lengths 0..order, those that are no state included
        state = walk(lm, ctx)
        assert lm.contexts[state] == ctx[len(ctx) - len(lm.contexts[state]):]
        for c in lm.eligible():
            bows, value, _ = ref.terms(ctx, c)
            seen_levels.add(len(bows))
            assert lm.step(state, c)[0] == pytest.approx(ref.g(ctx, c), abs=1e-12), (ctx, c)
        assert lm.end_lp[state] == pytest.approx(ref.end(ctx), abs=1e-12), ctx
    assert seen_levels == {0, 1, 2}                               # found at once, and backed off through every level
    t, h, e, a, b = (CHARSET.index(ch) for ch in "theab")
    assert lm.log_prob([t, h, e]) == pytest.approx(math.log(10) * (-0.3 - 0.05 - 0.02 - 0.3), abs=1e-12)
    assert lm.log_prob([a], end=False) == pytest.approx(math.log(10) * (-0.5 - 1.5), abs=1e-12)
    assert lm.log_prob([t, 1]) == -math.inf and lm.log_prob([0]) == -math.inf
    for word in ([], [t], [t, h, e, 2, t, h, e], [a, a, b], [e, e, h, t, b, 2]):
        for end in (True, False):
            assert lm.log_prob(word, end) == pytest.approx(ref.log_prob(word, end), abs=1e-12)


def sparse_model(order):
    """One chain `a b e h t ..` listed at every order and nothing else but the unigrams: contexts whose suffixes are no states."""
    chain = [CHARSET.index(ch) for ch in "abeht ab"][:order]
    ngrams = {(c,): (-1.0 - 0.1 * c, -0.05 * c) for c in range(2, 8)}
    ngrams[(EOS,)] = (-2.0, 0.0)
    for n in range(2, order + 1):
        ngrams[tuple(chain[:n])] = (-0.1 * n, -0.01 * n if n < order else 0.0)
    return CharNgramLM(ngrams, CHARSET, order=order), chain


def test_sparse_order_five_comes_back_to_the_higher_order_state():
    lm, chain = sparse_model(5)
    ref = dict_model(lm)
    assert lm.start_state == 0 and lm.states == 1 + 6 + 3
    a, b, e, h, t = chain
    state = walk(lm, (a, b, e))
    assert lm.contexts[state] == (a, b, e)
    g, state = lm.step(state, a)                                   # no `a b e a`: through (a b e), (b e) no state, (e), to `a`
    assert lm.contexts[state] == (a,) and g == pytest.approx(lm.bow[lm.state_of[(a, b, e)]] + lm.bow[lm.state_of[(e,)]]
                                                             + lm.ngrams[(a,)][0])
    for c, want in ((b, (a, b)), (e, (a, b, e)), (h, (a, b, e, h)), (t, (t,))):     # a b e h t is no state: its suffix t is
        state = lm.step(state, c)[1]
        assert lm.contexts[state] == want
    rng = np.random.RandomState(0)
    for _ in range(200):
        word = [chain[i] if rng.rand() < 0.7 else int(rng.randint(2, 8)) for i in rng.randint(0, 5, size=rng.randint(0, 9))]
        assert lm.log_prob(word) == pytest.approx(ref.log_prob(word), abs=1e-12), word


def image_lookup(img, state, sym):
    """(g accumulated in float64 from the image's f32 values, next state, probes of the deepest lookup): the header's rule."""
    acc, deepest = 0.0, 0
    for _ in range(img['order']):
        key, h = (state << 32) | (sym + 1), arc_hash(state, sym, img['slots'])
        for probe in range(1, img['max_probe'] + 1):
            deepest = max(deepest, probe)
            if int(img['keys'][h]) == key:
                return acc + float(img['arc_lp'][h]), int(img['arc_next'][h]), deepest
            if int(img['keys'][h]) == 0:
                break
            h = (h + 1) % img['slots']
        if state == 0:
            break
        acc += float(img['bow'][state])
        state = int(img['backoff'][state])
    return -math.inf, 0, deepest


@pytest.mark.parametrize("C", [8, 40])
def test_device_image_follows_the_header(C):
    for lm in (CharNgramLM.from_arpa(ARPA3, CHARSET), sparse_model(_lib._DEFINES["MR_NGRAM_ORDER_MAX"])[0]):
        img = lm.image(C)
        used = int((img['keys'] != 0).sum())
        assert 2 * used <= img['slots'] and used == len(lm.arcs) + sum((0, c) not in lm.arcs for c in lm.eligible(C))
        assert img['keys'].dtype == np.uint64 and img['arc_lp'].dtype == np.float32 and img['arc_next'].dtype == np.int32
        assert img['bow'].dtype == np.float32 and img['backoff'].dtype == np.int32 and img['end_lp'].dtype == np.float32
        assert img['backoff'][0] == -1 and img['start_state'] == lm.start_state and img['order'] == lm.order
        deepest = 0
        for state in range(lm.states):
            for c in lm.eligible(C):
                g, nxt, probes = image_lookup(img, state, c)
                deepest = max(deepest, probes)
                want, want_next = lm.step(state, c)
                assert g == pytest.approx(want, rel=1e-6) and nxt == want_next, (state, c)
            assert float(img['end_lp'][state]) == pytest.approx(lm.end_lp[state], rel=1e-6)
        own = [1 + (h - arc_hash(int(k) >> 32, (int(k) & 0xffffffff) - 1, img['slots'])) % img['slots']
               for h, k in enumerate(img['keys']) if k]
        assert img['max_probe'] == max(own) and deepest <= img['max_probe']      # really the maximum, and never exceeded
        assert image_lookup(img, 0, 0)[0] == -math.inf and image_lookup(img, 0, 1)[0] == -math.inf    # blank, unknown: no arc
    with pytest.raises(ValueError, match="classes"):
        lm.image(7)


WORDS = ["the", "teeth", "that", "hat", "heat", "tea", "bet", "beta", "at", "a bat", "be at", "the hat"]


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_train_is_normalised_and_ranks_seen_above_unseen(order):
    lm = CharNgramLM.train(WORDS + ["quiz"], CHARSET, order=order)
    assert lm.skipped == 1 and lm.order == order and lm.has_end
    for state in range(lm.states):
        mass = sum(math.exp(lm.step(state, c)[0]) for c in lm.eligible()) + math.exp(lm.end_lp[state])
        assert mass == pytest.approx(1.0, abs=1e-12), lm.contexts[state]
    t, h, e, b = (CHARSET.index(ch) for ch in "theb")
    if order >= 2:
        assert lm.step(walk(lm, (t,)), h)[0] > lm.step(walk(lm, (t,)), b)[0]        # `t h` is seen, `t b` is not
        assert lm.log_prob([t, h, e]) > lm.log_prob([t, b, e])
    assert lm.log_prob([t, h, e]) == pytest.approx(dict_model(lm).log_prob([t, h, e]), abs=1e-12)


def test_arpa_round_trip():
    for lm in (CharNgramLM.train(WORDS, CHARSET, order=3), CharNgramLM.from_arpa(ARPA3, CHARSET), sparse_model(5)[0]):
        again = CharNgramLM.from_arpa(lm.to_arpa(), CHARSET)
        assert set(again.ngrams) == set(lm.ngrams) and (again.order, again.states, again.start_state) == \
            (lm.order, lm.states, lm.start_state)
        for gram, (lp, bow) in lm.ngrams.items():
            assert again.ngrams[gram][0] == pytest.approx(lp, rel=1e-6) and again.ngrams[gram][1] == pytest.approx(bow, rel=1e-6)


def test_arpa_from_a_file(tmp_path):
    path = tmp_path / "model.arpa"
    path.write_text(ARPA3)
    assert CharNgramLM.from_arpa(str(path), CHARSET).ngrams == CharNgramLM.from_arpa(ARPA3, CHARSET).ngrams


def test_unknown_characters_are_skipped_and_counted():
    text = ARPA3.replace("ngram 1=7", "ngram 1=9").replace("-1.2 b\n", "-1.2 b\n-2.5 <unk>\n-1.1 z -0.3\n") \
        .replace("ngram 2=6", "ngram 2=8").replace("-0.9 t b\n", "-0.9 t b\n-0.7 z t\n-0.7 t <unk>\n")
    lm = CharNgramLM.from_arpa(text, CHARSET)
    assert lm.skipped == 3 and set(lm.ngrams) == set(CharNgramLM.from_arpa(ARPA3, CHARSET).ngrams)
    assert lm.floor == pytest.approx(-2.5 * math.log(10))                            # <unk> keeps its meaning
    assert lm.log_prob([CHARSET.index('a')], end=False) == pytest.approx(math.log(10) * (-0.5 - 2.5))


@pytest.mark.parametrize("bad,why", [
    (ARPA3.replace("\\end\\", ""), "end"),
    (ARPA3.replace("ngram 2=6", "ngram 2=5"), "counts"),
    (ARPA3.replace("-0.02 t h e", "-0.02 b h e"), "context"),
    (ARPA3.replace("-0.9 t b", "-0.9 t"), "tokens"),
    (ARPA3.replace("-0.9 t b", "x t b"), "number"),
    (ARPA3.replace("-0.9 t b", "-0.9 t th"), "one character"),
    (ARPA3.replace("-0.9 t b", "-0.2 t h"), "twice"),
    (ARPA3.replace("\\3-grams:", "\\4-grams:"), "sections"),
    ("ngram 1=1\n" + ARPA3, "data"),
    ("no such file.arpa", "neither"),
])
def test_malformed_arpa_is_refused(bad, why):
    with pytest.raises(ValueError, match=why):
        CharNgramLM.from_arpa(bad, CHARSET)


def test_orders_above_the_maximum_are_refused():
    top = _lib._DEFINES["MR_NGRAM_ORDER_MAX"]
    assert top == 8
    counts = "".join("ngram %d=1\n" % n for n in range(1, top + 2))
    with pytest.raises(ValueError, match="MR_NGRAM_ORDER_MAX"):
        CharNgramLM.from_arpa("\\data\\\n" + counts + "\n\\1-grams:\n-1 t\n\\end\\\n", CHARSET)
    with pytest.raises(ValueError, match="MR_NGRAM_ORDER_MAX"):
        CharNgramLM.train(WORDS, CHARSET, order=top + 1)
    assert CharNgramLM.train(WORDS, CHARSET, order=top).order == top
    with pytest.raises(ValueError, match="discount"):
        CharNgramLM.train(WORDS, CHARSET, discount=1.0)


# ---- the restatement of mr_ctc_beam_search_lm itself: with nothing pruned it is enumeration + the model

@pytest.mark.parametrize("alpha,beta,end", [(1.0, 0.0, True), (0.5, 0.3, False), (0.0, 0.7, True)])
@pytest.mark.parametrize("C,T", [(4, 3), (4, 5), (5, 4), (5, 5)])
def test_restatement_equals_enumeration_plus_model(C, T, alpha, beta, end):
    charset = Charset("abc"[:C - 2], case_sensitive=True)
    lm = CharNgramLM.train(["ab", "abba", "cab", "bc", "a"], charset, order=3)
    ref = dict_model(lm)
    y = B.posterior(np.random.RandomState(C * 16 + T), 3, T, C, sharp=1.5)
    for row in y:
        lp = B.logs(row)
        truth = B.enumerate_strings(np.exp(lp.astype(np.float64)), 0, 1)
        got = B.beam_search(lp, 10 ** 6, 10 ** 6, C, 0, 1, np.float64, ref, alpha, beta, end)['hyps']
        assert {p for p, _, _, _ in got} == set(truth)
        assert [s for _, s, _, _ in got] == sorted((s for _, s, _, _ in got), reverse=True)
        for p, score, ctc, part in got:
            assert ctc == pytest.approx(truth[p], abs=1e-12)
            assert part == pytest.approx(alpha * lm.log_prob(p, end) + beta * len(p), abs=1e-12)
            assert score == pytest.approx(truth[p] + alpha * lm.log_prob(p, end) + beta * len(p), abs=1e-12)
