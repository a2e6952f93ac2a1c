"""mr_ctc_beam_search_lm (csrc/ctc_beam.hip) and `ctc_beam_search_decode(lm=...)` against enumeration of every path plus the
model's own float64 score, and against the numpy restatement (tests/_ctc_beam_ref.py, with a model) over the dict scorer
(tests/_ngram_lm_ref.py) of the same n-grams.

Tolerance: the convention of tests/test_ctc_beam_gpu.py.  Each case runs the restatement in float64 and in float32; e32 is the
largest |score32 - score64| over the rows where both return the same strings, the kernel gets tol = 8 * e32, and a row is CLEAR
when its float64 margin (on the fused keys: the B-th against the (B+1)-th candidate, the Kc-th symbol against the best one left
out, two consecutive returned scores) exceeds 2 tol.  On clear rows strings, order, lengths and count equal the float64
restatement; on every row: scores descend and are exactly the f32 sum ctc_scores + lm_scores, no NaN, slots past count are
(0, -inf in all three, blanks), ctc_scores is at most the float64 log-probability of its string over ALL alignments + tol, and
all three scores are within tol of the restatement's for every string it returned too.  At most a quarter of a pruned run's rows
may be non-clear (seeds and sharpness were chosen with the restatement alone)."""
import math
import string

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ctc_beam_ref as B  # noqa: E402
import _ngram_lm_ref as R  # noqa: E402
import test_ctc_beam_gpu as G  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.charsets import Charset  # noqa: E402
from megreader_amd.ops.decode import ctc_beam_search_decode  # noqa: E402
from megreader_amd.ops.language_model import CharNgramLM, EOS  # noqa: E402

DEV = "cuda"
KEYS = ('ids', 'lengths', 'scores', 'ctc_scores', 'lm_scores', 'count')
PLAIN = ('ids', 'lengths', 'scores', 'count')
SCORES = ('scores', 'ctc_scores', 'lm_scores')

ENGLISH = Charset(string.digits + string.ascii_uppercase[:25])                          # 37 classes
WORDS = ["THE", "THEN", "THAT", "THERE", "HAT", "HEAT", "TEA", "BET", "BETA", "AT", "BAT", "BE", "HE", "SHE", "READ", "READER",
         "TEXT", "BEAM", "SEARCH", "MODEL", "LANGUAGE", "CHARACTER", "STRING", "SCORE", "42", "2024", "A1", "ROOM 101"]
SMALL = Charset("abeht", case_sensitive=True)                                           # blank, unknown, a b e h t: 7 classes
SMALL_WORDS = ["the", "the", "the", "the", "the", "hat", "tea", "bet", "beta", "that", "at"]


eval_layout = G.eval_layout


def host(out, keys=KEYS):
    return G.host(out, keys)


def dict_model(lm, C=None):
    """The dict scorer over the class's n-grams (the same tokens): no automaton."""
    return R.DictLM(lm.ngrams, lm.order, lm.eligible(C), None)


def strings(out, n):
    """[(tuple of ids, score, ctc_score, lm_score)] of row n as returned."""
    return G.strings(out, n, SCORES)


class Reference(object):
    """The two restatements of one case, computed once: lp [N, T, C], the f32 table of logs."""

    def __init__(self, lp, lm, weights, beam, nbest, top, blank=0, unknown=1):
        self.lp, self.lm, self.weights, self.args, self.blank, self.unknown = lp, lm, weights, (beam, nbest, top), blank, unknown
        alpha, beta, end = weights
        model = dict_model(lm, lp.shape[2])
        self.r64 = B.decode(lp, beam, nbest, top, blank, unknown, np.float64, model, alpha, beta, end)
        self.r32 = B.decode(lp, beam, nbest, top, blank, unknown, np.float32, model, alpha, beta, end)
        self.e32 = 0.0
        for a, b in zip(self.r64, self.r32):
            if [h[0] for h in a['hyps']] == [h[0] for h in b['hyps']]:
                self.e32 = max([self.e32] + [abs(float(y[1]) - float(x[1])) for x, y in zip(a['hyps'], b['hyps'])])
        self.tol = 8.0 * self.e32
        self.clear = [r['margin'] > 2 * self.tol for r in self.r64]


def compare(out, ref, name="", need_clear=None, truth=None, ctc_tol=None):
    """Every assertion of the module docstring; `truth`: per row {string: float64 log-probability} from enumeration, which then
    replaces the restatement as what the scores are held to (with the model's own float64 `log_prob`), and must list exactly the
    strings returned; its ctc_scores are held to `ctc_tol`.  Returns worst / e32."""
    lp, (beam, nbest, top), blank, lm = ref.lp, ref.args, ref.blank, ref.lm
    alpha, beta, end = ref.weights
    N, T = lp.shape[:2]
    tol, worst = ref.tol, 0.0
    assert out['ids'].shape == (N, nbest, T) and out['count'].shape == (N,)
    for key in SCORES:
        assert out[key].shape == (N, nbest) and out[key].dtype == np.float32 and not np.isnan(out[key]).any(), key
    for n in range(N):
        got, want = strings(out, n), ref.r64[n]['hyps']
        k = len(got)
        assert 0 <= k <= nbest
        assert np.all(out['lengths'][n, k:] == 0) and np.all(out['ids'][n, k:] == blank), n
        for key in SCORES:
            assert np.all(out[key][n, k:] == -np.inf), (n, key)
        for j in range(k):
            assert np.all(out['ids'][n, j, out['lengths'][n, j]:] == blank), (n, j)
            assert all(np.isfinite(v) for v in got[j][1:]), (n, j)
            assert out['scores'][n, j] == np.float32(out['ctc_scores'][n, j] + out['lm_scores'][n, j]), (n, j)
        scores = [h[1] for h in got]
        assert scores == sorted(scores, reverse=True), (n, scores)
        assert len({h[0] for h in got}) == k, "a string twice in row %d: %r" % (n, got)
        theirs = {h[0]: h[1:] for h in want}
        for p, s, ctc, part in got:
            assert blank not in p and ref.unknown not in p
            bound = truth[n][p] if truth is not None else B.true_score(lp[n], p, blank, ref.unknown)
            assert ctc <= bound + tol, (n, p, ctc, bound, tol)
            if p in theirs:
                for mine, other, what in zip((s, ctc, part), theirs[p], SCORES):
                    err = abs(mine - float(other))
                    worst = max(worst, err)
                    assert err <= tol, "row %d %r %s: |kernel - float64| = %.3g, tol = %.3g (e32 = %.3g)" \
                        % (n, p, what, err, tol, ref.e32)
        if truth is not None:
            assert {h[0] for h in got} == set(truth[n]), n
            for p, s, ctc, part in got:
                fused = truth[n][p] + alpha * lm.log_prob(p, end) + beta * len(p)
                worst = max(worst, abs(s - fused))
                assert abs(s - fused) <= tol, "row %d %r: |kernel - (enumeration + model)| = %.3g, tol = %.3g" \
                    % (n, p, abs(s - fused), tol)
                assert abs(ctc - truth[n][p]) <= ctc_tol, (n, p, ctc, truth[n][p], ctc_tol)
        if ref.clear[n]:
            assert [h[0] for h in got] == [h[0] for h in want], (n, got, want)
    ratio = worst / ref.e32 if ref.e32 > 0 else 0.0
    print("%s: N=%d T=%d C=%d B=%d K=%d Kc=%d order=%d weights=%r e32=%.3g tol=%.3g worst=%.3g (%.2f e32), %d of %d rows clear"
          % (name, N, T, lp.shape[2], beam, nbest, top, lm.order, ref.weights, ref.e32, tol, worst, ratio, sum(ref.clear), N))
    if need_clear is not None:
        assert sum(ref.clear) >= need_clear, "only %d of %d rows are clear" % (sum(ref.clear), N)
    return ratio


def run(y, lm, weights, beam, nbest, top, blank=0, unknown=1, name="", need_clear=None, dtype=torch.float32, truth=None,
        ctc_tol=None):
    """y: f32 [N, T, C] probabilities.  Decode on the device, restate, compare; returns (outputs, reference)."""
    pred = eval_layout(y, dtype)
    seen = pred.float().cpu().numpy()[:, :, 0, :].transpose(0, 2, 1)              # what the kernel reads (bf16: rounded)
    alpha, beta, end = weights
    out = host(ctc_beam_search_decode(pred, beam=beam, nbest=nbest, top_classes=top, blank=blank, unknown=unknown, lm=lm,
                                      lm_weight=alpha, lm_bonus=beta, lm_end=end))
    ref = Reference(B.logs(seen), lm, weights, beam, nbest, top, blank, unknown)
    compare(out, ref, name, need_clear, truth, ctc_tol)
    return out, ref


def three_quarters(N):
    return -(-3 * N // 4)


def english(order=3):
    return CharNgramLM.train(WORDS, ENGLISH, order=order)


def chain_model(order):
    """An order-`order` model that is NOT closed under suffixes: the unigrams, and two chains listed at every order."""
    ids = [c for c in range(len(ENGLISH)) if c > 1]
    ngrams = {(c,): (-2.0 - 0.05 * c, -0.02 * (c % 7)) for c in ids}
    ngrams[(EOS,)] = (-3.0, 0.0)
    chains = [[ENGLISH.index(ch) for ch in word[:order]] for word in ("ABCDEFGH", "CDEXYABC")]
    for chain in chains:
        for n in range(2, order + 1):
            ngrams[tuple(chain[:n])] = (-0.05 * n, -0.3 - 0.01 * n if n < order else 0.0)
        ngrams[tuple(chain[:order - 1]) + (EOS,)] = (-0.5, 0.0)
    return CharNgramLM(ngrams, ENGLISH, order=order), chains


# ---- the masses stay pure

def test_zero_weights_are_the_plain_search():
    y = B.posterior(np.random.RandomState(1), 24, 16, 37, 2.0)
    y[3, 5, 7] = 0.0
    pred = eval_layout(y)
    for beam, nbest, top in ((8, 8, 16), (1, 1, 4), (64, 5, 37)):
        plain = host(ctc_beam_search_decode(pred, beam=beam, nbest=nbest, top_classes=top), PLAIN)
        fused = host(ctc_beam_search_decode(pred, beam=beam, nbest=nbest, top_classes=top, lm=english(), lm_weight=0.0,
                                            lm_bonus=0.0, lm_end=False))
        for key in ('ids', 'lengths', 'count'):
            assert np.array_equal(fused[key], plain[key]), (beam, key)
        assert np.all(fused['ctc_scores'] == plain['scores']) and np.all(fused['scores'] == plain['scores'])
        live = np.arange(nbest)[None, :] < fused['count'][:, None]
        assert np.all(fused['lm_scores'][live] == 0.0) and np.all(fused['lm_scores'][~live] == -np.inf)


# ---- exhaustive: against enumeration and the model's own float64 score

class NoUnknown(object):
    """An alphabet whose every class but the blank is a character: unknown = -1, "there is none"."""
    blank, unknown = 0, -1

    def __init__(self, chars):
        self.chars = chars

    def __len__(self):
        return 1 + len(self.chars)

    def __getitem__(self, i):
        return self.chars[i - 1]

    def index(self, ch):
        return self.chars.index(ch) + 1 if ch in self.chars else self.unknown


@pytest.mark.parametrize("weights", [(1.0, 0.0, True), (0.5, 0.3, False)])
@pytest.mark.parametrize("C,T,unknown", [(4, 4, -1), (5, 4, 1), (4, 4, 1), (4, 5, 1)])
def test_exhaustive_equals_enumeration_plus_model(C, T, unknown, weights):
    """Every case whose labelings fit a beam of 64: three symbols have 61 in four columns and 148 in five (C = 5 at T = 5, and C =
    4 without an unknown at T = 5, cannot be exhaustive); two symbols have 25 in five."""
    charset = Charset("abc"[:C - 2], case_sensitive=True) if unknown == 1 else NoUnknown("abc"[:C - 1])
    assert len(charset) == C
    lm = CharNgramLM.train(["ab", "abba", "cab", "bc", "a", "dab"], charset, order=3)
    y = B.posterior(np.random.RandomState(C * 16 + T), 16, T, C, sharp=1.5)
    truth = [B.enumerate_strings(np.exp(B.logs(row).astype(np.float64)), 0, unknown) for row in y]
    assert max(len(t) for t in truth) <= 64
    plain_tol = G.Reference(B.logs(y), 64, 64, 64, 0, unknown).tol
    out, ref = run(y, lm, weights, 64, 64, 64, unknown=unknown, name="exhaustive C=%d T=%d" % (C, T), truth=truth,
                   ctc_tol=plain_tol)
    assert [int(c) for c in out['count']] == [len(t) for t in truth]


# ---- pruned

def test_pruned_english_order_three():
    y = B.posterior(np.random.RandomState(3), 64, 24, 37, 2.0)
    run(y, english(3), (0.8, 0.5, True), 8, 8, 16, name="english", need_clear=three_quarters(64))


def test_pruned_maximum_candidates():
    charset = Charset(string.digits + string.ascii_letters + "!?", case_sensitive=True)        # 66 classes: 64 symbols
    lm = CharNgramLM.train(["the", "Then", "a1", "b2!", "What?", "42"], charset, order=2)
    y = B.posterior(np.random.RandomState(5), 6, 3, 66, 2.0)
    out, _ = run(y, lm, (1.0, 0.2, True), 64, 64, 64, name="64 x 64", need_clear=three_quarters(6))
    assert np.all(out['count'] == 64)


def test_pruned_sparse_model_of_the_greatest_order():
    order = _lib._DEFINES["MR_NGRAM_ORDER_MAX"]
    lm, chains = chain_model(order)
    rng = np.random.RandomState(9)
    y = B.posterior(rng, 32, 12, 37, 1.5)
    for n in range(32):                                    # the rows spell along a chain, from some point of it, with noise
        chain, at = chains[n % 2], int(rng.randint(0, 4))
        for t in range(12):
            y[n, t, chain[(at + t // 2) % order] if t % 3 else 0] += 1.5
    y /= y.sum(axis=2, keepdims=True)
    out, ref = run(y.astype(np.float32), lm, (1.0, 0.3, True), 8, 8, 8, name="order %d" % order, need_clear=three_quarters(32))
    deep = 0
    for n in range(32):
        state = lm.start_state
        for c in out['ids'][n, 0, :out['lengths'][n, 0]]:
            state = lm.step(state, int(c))[1]
            deep = max(deep, len(lm.contexts[state]))
    assert deep >= 5, "the strings read never reach a context of five symbols (%d)" % deep


def test_wide_alphabet_takes_the_unigram_floor():
    """C = 6 000, past the staged column; the model lists 40 classes, every other one scores the floor."""
    charset = Charset([chr(0x4e00 + i) for i in range(5998)], case_sensitive=True)
    listed = [chr(0x4e00 + 7 * i) for i in range(40)]
    lines = ["-99 <s> -0.3", "-1.2 </s>"] + ["%.3f %s -0.2" % (-1.0 - 0.02 * i, ch) for i, ch in enumerate(listed)]
    pairs = ["%.3f %s %s" % (-0.2 - 0.01 * i, listed[i], listed[i + 1]) for i in range(39)]
    text = "\\data\\\nngram 1=%d\nngram 2=%d\n\n\\1-grams:\n%s\n\n\\2-grams:\n%s\n\n\\end\\\n" \
        % (len(lines), len(pairs), "\n".join(lines), "\n".join(pairs))
    lm = CharNgramLM.from_arpa(text, charset)
    assert lm.classes == 6000 and lm.floor == pytest.approx(-1.78 * math.log(10)) and len(lm.arcs) == 40 + 39
    rng = np.random.RandomState(2)
    y = B.posterior(rng, 12, 8, 6000, 3.0)
    for n in range(12):
        for t in range(8):
            y[n, t, charset.index(listed[(n + t // 2) % 40])] += 0.02           # some listed classes among the column's best
    y /= y.sum(axis=2, keepdims=True)
    out, _ = run(y.astype(np.float32), lm, (1.0, 0.0, True), 4, 4, 16, name="wide", need_clear=three_quarters(12))
    ids = set(int(c) for c in out['ids'].ravel()) - {0}
    inside = {charset.index(ch) for ch in listed}
    assert ids & inside and ids - inside                   # both kinds are read


# ---- the model decides

def small(order=3):
    return CharNgramLM.train(SMALL_WORDS, SMALL, order=order)


def crafted(columns):
    """[1, T, 7] over SMALL: per column {character or '' for the blank: probability}; the rest is spread over the other classes."""
    y = np.zeros((1, len(columns), 7), dtype=np.float32)
    for t, column in enumerate(columns):
        rest = (1.0 - sum(column.values())) / (7 - len(column))
        y[0, t, :] = rest
        for ch, p in column.items():
            y[0, t, SMALL.index(ch) if ch else 0] = p
    return y


def text_of(out, n=0, k=0):
    return SMALL.label_to_string(out['ids'][n, k, :out['lengths'][n, k]])


def test_the_model_prefers_the_to_tbe():
    y = crafted([{'t': 0.9}, {'b': 0.5, 'h': 0.4}, {'e': 0.9}])
    pred = eval_layout(y)
    plain = host(ctc_beam_search_decode(pred, beam=8, nbest=2, top_classes=5), PLAIN)
    assert text_of(plain) == "tbe" and text_of(plain, k=1) == "the"
    out, ref = run(y, small(), (1.0, 0.0, True), 8, 2, 5, name="tbe")
    assert ref.clear[0] and text_of(out) == "the" and text_of(out, k=1) != "tbe"        # the model has never seen `t b`
    assert out['ctc_scores'][0, 0] == pytest.approx(plain['scores'][0, 1], abs=1e-5) and out['lm_scores'][0, 0] < 0.0


def test_bonus_lengthens_and_the_end_reorders():
    y = B.posterior(np.random.RandomState(6), 32, 10, 7, 1.0)
    short, _ = run(y, small(), (0.0, 0.0, False), 8, 1, 5, name="no bonus")
    long, ref = run(y, small(), (0.0, 1.5, False), 8, 1, 5, name="bonus 1.5", need_clear=three_quarters(32))
    want = [len(r['hyps'][0][0]) for r in ref.r64]
    assert [int(k) for k, ok in zip(long['lengths'][:, 0], ref.clear) if ok] == [k for k, ok in zip(want, ref.clear) if ok]
    assert long['lengths'][:, 0].sum() > short['lengths'][:, 0].sum()
    assert np.all(long['lm_scores'][:, 0] == np.float32(1.5) * long['lengths'][:, 0])
    # "th" is the likelier reading and "the" the likelier word: the end of the string is what tells them apart
    y = crafted([{'t': 0.95}, {'h': 0.95}, {'e': 0.42, '': 0.55}])
    off, ref_off = run(y, small(), (1.0, 0.0, False), 8, 2, 5, name="end off")
    on, ref_on = run(y, small(), (1.0, 0.0, True), 8, 2, 5, name="end on")
    assert ref_off.clear[0] and ref_on.clear[0]
    assert (text_of(off), text_of(off, k=1)) == ("th", "the") and (text_of(on), text_of(on, k=1)) == ("the", "th")


# ---- shapes, types, layouts

def test_bf16_posterior():
    y = B.posterior(np.random.RandomState(33), 16, 12, 37, 2.0)
    run(y, english(), (0.8, 0.5, True), 4, 4, 16, name="bf16", need_clear=three_quarters(16), dtype=torch.bfloat16)


def test_one_column_beam_of_one_and_one_row():
    run(B.posterior(np.random.RandomState(11), 8, 1, 7, 1.0), small(), (1.0, 0.2, True), 4, 4, 5, name="T=1")
    out, _ = run(B.posterior(np.random.RandomState(12), 8, 12, 7, 2.0), small(), (1.0, 0.2, True), 1, 1, 5, name="B=1")
    assert np.all(out['count'] == 1)
    run(B.posterior(np.random.RandomState(14), 1, 9, 7, 1.5), small(), (1.0, 0.2, True), 4, 4, 5, name="N=1")
    empty = ctc_beam_search_decode(torch.zeros((0, 7, 1, 5), device=DEV), beam=4, nbest=2, lm=small())
    assert [tuple(empty[k].shape) for k in KEYS] == [(0, 2, 5), (0, 2), (0, 2), (0, 2), (0, 2), (0,)]
    raw_call(torch.zeros((0, 7, 5), device=DEV), small(), 4, 2, 5, override=dict(ws=0, ws_bytes=0))      # MR_OK without a launch


def test_nbest_below_and_at_the_beam():
    y = B.posterior(np.random.RandomState(13), 8, 12, 7, 2.0)
    few, _ = run(y, small(), (1.0, 0.2, True), 8, 3, 5, name="K=3 of B=8")
    full, _ = run(y, small(), (1.0, 0.2, True), 8, 8, 5, name="K=8 of B=8")
    for key in ('ids', 'lengths') + SCORES:
        assert np.array_equal(few[key].view(np.int32), full[key][:, :3].view(np.int32)), key
    assert np.array_equal(few['count'], np.minimum(full['count'], 3))


def test_layouts_and_logs_give_the_same_bits():
    y = B.posterior(np.random.RandomState(20), 10, 14, 7, 2.0)
    y[3, 5, 4] = 0.0
    args = dict(beam=6, nbest=4, top_classes=4, lm=small(), lm_weight=0.9, lm_bonus=0.1)
    base = host(ctc_beam_search_decode(eval_layout(y), **args))
    compare(base, Reference(B.logs(y), args['lm'], (0.9, 0.1, True), 6, 4, 4), "layout base")
    ntc = torch.from_numpy(y).to(DEV)                                              # [N, T, C]: the class stride is 1
    views = {"[N, C, T]": eval_layout(y).select(2, 0), "class-fast": ntc.permute(0, 2, 1),
             "sliced": torch.from_numpy(np.repeat(y, 2, axis=0)).to(DEV).permute(0, 2, 1)[::2],
             "float64": eval_layout(y).double()}
    assert views["[N, C, T]"].stride(2) == 1 and views["class-fast"].stride(1) == 1 and not views["sliced"].is_contiguous()
    for name, pred in views.items():
        got = host(ctc_beam_search_decode(pred, **args))
        for key in KEYS:
            assert np.array_equal(got[key].view(np.int32), base[key].view(np.int32)), (name, key)
    logs = torch.from_numpy(B.logs(y)).to(DEV).permute(0, 2, 1)
    got = host(ctc_beam_search_decode(logs, log_probs=True, **args))
    for key in KEYS:
        assert np.array_equal(got[key].view(np.int32), base[key].view(np.int32)), ("logs", key)


def test_a_column_on_unknown_kills_the_row():
    y = B.posterior(np.random.RandomState(18), 4, 9, 7, 1.5)
    y[2, 4, :] = 0.0
    y[2, 4, 1] = 1.0
    out, _ = run(y, small(), (1.0, 0.2, True), 4, 4, 5, name="unknown column")
    assert out['count'].tolist()[2] == 0 and np.all(out['count'][[0, 1, 3]] > 0)
    assert np.all(out['ids'][2] == 0) and np.all(out['lengths'][2] == 0)
    for key in SCORES:
        assert np.all(out[key][2] == -np.inf), key


def test_the_model_has_to_fit_the_call():
    pred = eval_layout(B.posterior(np.random.RandomState(4), 2, 5, 7, 1.0))
    with pytest.raises(ValueError, match="the model is over 37 classes"):
        ctc_beam_search_decode(pred, lm=english())
    with pytest.raises(ValueError, match="blank"):
        ctc_beam_search_decode(pred, lm=small(), blank=2)
    with pytest.raises(ValueError, match="unknown"):
        ctc_beam_search_decode(pred, lm=small(), unknown=-1)
    with pytest.raises(ValueError, match="finite"):
        ctc_beam_search_decode(pred, lm=small(), lm_weight=float('nan'))
    # more classes than the model's: those take the floor
    run(B.posterior(np.random.RandomState(4), 2, 5, 9, 1.0), small(), (1.0, 0.0, True), 4, 4, 7, name="C=9 over 7")


# ---- invariance

def raw_call(pred, lm, beam, nbest, top, weights=(1.0, 0.2, True), blank=0, unknown=1, expect=0, override=()):
    """The C entry point with every output and the workspace pre-filled with garbage; `override` replaces arguments by name.
    Returns (return code, outputs as numpy)."""
    if pred.dim() == 4:
        pred = pred.select(2, 0)
    N, C, T = pred.shape
    K = max(1, min(nbest, 64))
    ids = torch.full((N, K, T), 12345, dtype=torch.int32, device=DEV)
    lengths = torch.full((N, K), 12345, dtype=torch.int32, device=DEV)
    count = torch.full((N,), 12345, dtype=torch.int32, device=DEV)
    scores, ctc_scores, lm_scores = (torch.full((N, K), 777.0, dtype=torch.float32, device=DEV) for _ in range(3))
    nbytes = _lib.load().mr_ctc_beam_ws_bytes(max(N, 1), T, max(1, min(beam, 64)), max(1, min(top, 64)))
    ws = torch.full((nbytes // 8 + 1,), -0x5454545454545455, dtype=torch.int64, device=DEV)
    sn, sc, st = pred.stride()
    m = lm._tensors(torch.device(DEV, torch.cuda.current_device()), C)
    a = dict(dtype={torch.float32: 0, torch.bfloat16: 1}[pred.dtype], pred=ptr(pred), sn=sn, sc=sc, st=st, N=N, C=C, T=T,
             log_probs=0, blank=blank, unknown=unknown, beam=beam, nbest=nbest, top=top, keys=ptr(m['keys']),
             arc_lp=ptr(m['arc_lp']), arc_next=ptr(m['arc_next']), bow=ptr(m['bow']), backoff=ptr(m['backoff']),
             end_lp=ptr(m['end_lp']), states=m['states'], slots=m['slots'], max_probe=m['max_probe'],
             start_state=m['start_state'], order=m['order'], alpha=weights[0], beta=weights[1], end=int(weights[2]), ids=ptr(ids),
             lengths=ptr(lengths), scores=ptr(scores), ctc_scores=ptr(ctc_scores), lm_scores=ptr(lm_scores), count=ptr(count),
             ws=ptr(ws), ws_bytes=ws.numel() * 8)
    a.update(dict(override))
    names = ("dtype", "pred", "sn", "sc", "st", "N", "C", "T", "log_probs", "blank", "unknown", "beam", "nbest", "top", "keys",
             "arc_lp", "arc_next", "bow", "backoff", "end_lp", "states", "slots", "max_probe", "start_state", "order", "alpha",
             "beta", "end", "ids", "lengths", "scores", "ctc_scores", "lm_scores", "count", "ws", "ws_bytes")
    rc = _lib.load().mr_ctc_beam_search_lm(*[a[k] for k in names], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.load().mr_last_error().decode())
    return rc, host(dict(ids=ids, lengths=lengths, scores=scores, ctc_scores=ctc_scores, lm_scores=lm_scores, count=count))


def test_deterministic_row_independent_and_every_output_written():
    y = B.posterior(np.random.RandomState(21), 9, 16, 37, 2.0)
    pred, lm = eval_layout(y), english()
    args = dict(beam=8, nbest=5, top_classes=8, lm=lm, lm_weight=1.0, lm_bonus=0.2)
    one = host(ctc_beam_search_decode(pred, **args))
    two = host(ctc_beam_search_decode(pred, **args))
    _, raw = raw_call(pred, lm, 8, 5, 8)                                           # outputs and workspace start as garbage
    for key in KEYS:
        assert np.array_equal(one[key].view(np.int32), two[key].view(np.int32)), key
        assert np.array_equal(one[key].view(np.int32), raw[key].view(np.int32)), key
    for n in (0, 4, 8):
        alone = host(ctc_beam_search_decode(pred[n:n + 1], **args))
        for key in KEYS:
            assert np.array_equal(alone[key][0].view(np.int32), one[key][n].view(np.int32)), (n, key)


def test_capturable_in_a_graph_and_the_model_is_only_read():
    y = B.posterior(np.random.RandomState(22), 6, 16, 37, 2.0)
    pred, other, lm = eval_layout(y), eval_layout(y[::-1].copy()), english()
    args = dict(beam=8, nbest=3, top_classes=8, lm=lm, lm_weight=1.0, lm_bonus=0.2)
    eager = {k: v.clone() for k, v in ctc_beam_search_decode(pred, **args).items()}          # the call outside: the upload
    eager_other = {k: v.clone() for k, v in ctc_beam_search_decode(other, **args).items()}
    image = lm._tensors(pred.device, 37)
    arrays = ('keys', 'arc_lp', 'arc_next', 'bow', 'backoff', 'end_lp')
    before = {k: image[k].clone() for k in arrays}
    static = pred.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        found = ctc_beam_search_decode(static, **args)
    for source, want in ((other, eager_other), (pred, eager)):                               # new contents of the same tensor
        static.copy_(source)
        graph.replay()
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(found[key].view(torch.int32), want[key].view(torch.int32)), key
    assert not torch.equal(eager['ids'], eager_other['ids'])
    assert lm._tensors(pred.device, 37) is image
    for k in arrays:
        assert torch.equal(image[k], before[k]), k


# ---- C ABI

def test_bad_arguments_are_refused_and_nothing_is_written():
    pred = eval_layout(B.posterior(np.random.RandomState(23), 3, 6, 7, 1.0)).select(2, 0)
    lm = small()
    cap, top = _lib._DEFINES["MR_SEQ_MEASURE_MAX"], _lib._DEFINES["MR_NGRAM_ORDER_MAX"]
    need = _lib.load().mr_ctc_beam_ws_bytes(3, 6, 4, 3)
    refused = [dict(T=0), dict(T=cap + 1), dict(C=1), dict(blank=7), dict(blank=-1), dict(beam=0), dict(beam=65), dict(nbest=0),
               dict(nbest=5), dict(top=0), dict(top=65), dict(ws=0), dict(ws_bytes=need - 1), dict(N=-1),
               dict(keys=0), dict(arc_lp=0), dict(arc_next=0), dict(bow=0), dict(backoff=0), dict(end_lp=0),
               dict(order=0), dict(order=top + 1), dict(states=0), dict(slots=0), dict(max_probe=0), dict(start_state=-1),
               dict(start_state=lm.states), dict(alpha=float('nan')), dict(alpha=float('inf')), dict(beta=float('-inf')),
               dict(ctc_scores=0), dict(lm_scores=0)]
    for override in refused:
        _, out = raw_call(pred, lm, 4, 4, 3, expect=1, override=override)
        assert np.all(out['ids'] == 12345) and np.all(out['lengths'] == 12345) and np.all(out['count'] == 12345), override
        for key in SCORES:
            assert np.all(out[key] == 777.0), (override, key)
    _, out = raw_call(pred, lm, 4, 4, 3, expect=2, override=dict(dtype=2))
    assert np.all(out['count'] == 12345)
    with pytest.raises(RuntimeError, match="mr_ctc_beam_search_lm: order=0"):
        call("mr_ctc_beam_search_lm", 0, ptr(pred), 42, 6, 1, 3, 7, 6, 0, 0, 1, 4, 1, 3, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 1.0, 0.0,
             1, 0, 0, 0, 0, 0, 0, 0, 0)
    raw_call(pred, lm, 4, 4, 3, override=dict(ws_bytes=need))                      # exactly what the query says is enough
