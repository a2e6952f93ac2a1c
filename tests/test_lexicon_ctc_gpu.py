"""mr_lexicon_transcribe (csrc/lexicon.hip) and `Lexicon.transcribe` against the numpy restatement (tests/_lexicon_ctc_ref.py).

Tolerance: none is fixed.  Each case computes e32 = max |S32 - S64| over its finite scores from the two restatements alone, on the
f32 probabilities the kernel reads, and the kernel gets tol = 8 * e32 (its exp / log and order of summation differ from numpy's;
e32 itself is rounding at the magnitude of the scores).  Per row, no row excluded: |best_score - S64[n, index]| <= tol;
S64[n, index] >= max S64[n] - 2 tol; the index is exact where the float64 top-two gap exceeds 2 tol (at least 9 rows in 10 must be
of that kind); the full table is within tol where finite and -inf exactly where the restatement is; candidates, distance and
length are exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lexicon_ctc_ref as Q  # noqa: E402
import _lexicon_ref as R  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.charsets import EnglishCharset, EnglishPrintableCharset, upper_fold_table  # noqa: E402
from megreader_amd.ops.decode import ctc_greedy_decode  # noqa: E402
from megreader_amd.ops.lexicon import Lexicon  # noqa: E402

DEV = "cuda"
KEYS = ('index', 'score', 'distance', 'length', 'candidates')


def eval_layout(y):
    """y [N, T, C] numpy -> the eval head's [N, C, T] f32 device tensor (a class's T values contiguous)."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(y, (0, 2, 1)))).to(DEV)


def device_transcribe(pred, words, blank=0, unknown=1, spans=None, max_distance=-1, log_probs=False, table=True, C=None,
                      T=None, dtype=None):
    """The C entry point: pred an [N, C, T] device tensor (any strides, f32 / bf16), the greedy ids from ctc_greedy_decode on it.
    Every output starts as garbage: the call writes all of them.  Returns numpy arrays by name (and the greedy ids)."""
    N, C_, T_ = pred.shape
    ids, _ = ctc_greedy_decode(pred, blank=blank, unknown=unknown)
    off = np.zeros(len(words) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(w) for w in words])
    sym = np.array([s for w in words for s in w] + [0], dtype=np.int32)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    d_sym, d_off, d_span = t(sym), t(off), t(spans)
    ints = torch.full((4, N), 12345, dtype=torch.int32, device=DEV)
    score = torch.full((N,), 777.0, dtype=torch.float32, device=DEV)
    scores = torch.full((N, len(words)), 777.0, dtype=torch.float32, device=DEV) if table else None
    sn, sc, st = pred.stride()
    code = {torch.float32: 0, torch.bfloat16: 1}[pred.dtype] if dtype is None else dtype
    call("mr_lexicon_transcribe", code, ptr(pred), sn, sc, st, T_ if T is None else T, int(log_probs), ptr(ids), T_, N, blank,
         unknown, 0, ptr(d_sym), ptr(d_off), len(words), ptr(d_span), C_ if C is None else C, max_distance, ptr(ints[0]),
         ptr(score), ptr(ints[1]), ptr(ints[2]), ptr(ints[3]), ptr(scores) if table and len(words) else 0)
    out = dict(index=ints[0], distance=ints[1], length=ints[2], candidates=ints[3], score=score)
    if table:
        out['scores'] = scores
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out['ids'] = ids.cpu().numpy()
    return out


class Reference(object):
    """The restatement of one case, computed once: y [N, T, C] f32 probabilities as the kernel reads them."""

    def __init__(self, y, words, blank=0, unknown=1):
        self.y, self.words, self.blank, self.unknown = y, words, blank, unknown
        self.S64 = Q.score_table(Q.log_probs(y, np.float64), words, blank, np.float64, unknown)
        self.S32 = Q.score_table(Q.log_probs(y, np.float32), words, blank, np.float32, unknown)
        fin = np.isfinite(self.S64)
        assert np.array_equal(fin, np.isfinite(self.S32))
        self.e32 = float(np.abs(self.S32[fin].astype(np.float64) - self.S64[fin]).max()) if fin.any() else 0.0
        self.tol = 8.0 * self.e32
        self.ids = Q.greedy(y, blank, unknown)
        self.D, self.length = R.distance_table(self.ids, words, blank, unknown)


def compare(got, ref, spans=None, max_distance=None, name="", need_exact=None):
    """Every assertion of the module docstring; returns the largest |kernel - S64| / e32."""
    N = len(ref.y)
    assert np.array_equal(got['ids'], ref.ids), "greedy ids"
    want = Q.transcribe(ref.S64, ref.D, ref.length, spans, max_distance)
    assert np.array_equal(got['length'], want['length']), (got['length'], want['length'])
    assert np.array_equal(got['candidates'], want['candidates']), (got['candidates'], want['candidates'])
    tol, worst, exact = ref.tol, 0.0, 0
    if 'scores' in got:
        fin = np.isfinite(want['scores'])
        assert np.all(got['scores'][~fin] == -np.inf), "-inf exactly where the restatement is"
        assert not np.isnan(got['scores']).any()
        if fin.any():
            err = np.abs(got['scores'][fin].astype(np.float64) - want['scores'][fin])
            worst = float(err.max())
            assert worst <= tol, "table: |kernel - S64| = %.3g, tol = %.3g (e32 = %.3g)" % (worst, tol, ref.e32)
    for n in range(N):
        row = want['scores'][n]
        order = np.sort(row[np.isfinite(row)])[::-1] if len(row) else np.zeros(0)
        i = int(got['index'][n])
        if len(order) == 0:
            assert (i, got['score'][n], got['distance'][n]) == (-1, -np.inf, -1), n
            exact += 1
            continue
        assert 0 <= i < len(row) and np.isfinite(row[i]), (n, i)
        err = abs(float(got['score'][n]) - row[i])
        worst = max(worst, err)
        assert err <= tol, (n, err, tol)
        assert row[i] >= order[0] - 2 * tol, (n, row[i], order[0])
        assert got['distance'][n] == ref.D[n, i], n
        if len(order) == 1 or order[0] - order[1] > 2 * tol:
            assert i == want['index'][n], (n, i, want['index'][n])
            exact += 1
    ratio = worst / ref.e32 if ref.e32 > 0 else 0.0
    print("%s: N=%d L=%d e32=%.3g tol=%.3g max|kernel-S64|=%.3g (%.2f e32), index exact on %d of %d rows" %
          (name, N, len(ref.words), ref.e32, tol, worst, ratio, exact, N))
    if need_exact is None:
        need_exact = -(-9 * N // 10)
    assert exact >= need_exact, "only %d of %d rows have a decisive float64 gap" % (exact, N)
    return ratio


def softmax32(logits):
    return torch.softmax(torch.from_numpy(logits.astype(np.float32)), dim=-1).numpy()


_CASES = {}


def random_case(kind, sharp):
    """The three shapes of the issue, seeded; computed once per (kind, sharp) and shared.  A few words are appended to the random
    ones: rows' own greedy strings, whole and edited, so that the distance filter has rows with and without members."""
    key = (kind, sharp)
    if key not in _CASES:
        N, T, C, L, longest = {"english": (24, 32, 38, 300, 12), "narrow": (16, 26, 12, 300, 30), "wide": (8, 32, 5360, 200, 10)}[kind]
        rng = np.random.RandomState(100 + 10 * sharp + len(kind))
        y = softmax32(rng.randn(N, T, C) * sharp)
        words = [rng.randint(2, C, size=k).tolist() for k in rng.randint(0, longest + 1, size=L)]
        if kind == "wide":
            words[0] = [C - 1, C - 2, C - 1]
            words[1] = [C - 1]
        for n in range(0, N, 4):
            g = R.compact(Q.greedy(y[n:n + 1])[0])
            words += [g, g[:3] + g[4:], g[:2] + [g[2] % (C - 2) + 2] + g[3:-2]]       # distance 0, 1 and (at most) 3
        _CASES[key] = (Reference(y, words), eval_layout(y))
    return _CASES[key]


@pytest.mark.parametrize("sharp", [1, 4])
@pytest.mark.parametrize("kind", ["english", "narrow", "wide"])
def test_random_posteriors_whole_lexicon_and_within_two_edits(kind, sharp):
    ref, pred = random_case(kind, sharp)
    everything = device_transcribe(pred, ref.words)
    compare(everything, ref, name="%s sharp %d, every word" % (kind, sharp))
    if kind == "narrow":
        share = float(np.mean(~np.isfinite(ref.S64)))
        print("infeasible pairs: %.0f %%" % (100 * share))
        assert share > 0.1
    near = device_transcribe(pred, ref.words, max_distance=2)
    compare(near, ref, max_distance=2, name="%s sharp %d, within 2" % (kind, sharp))
    cand = np.isfinite(near['scores'])
    assert cand.any()
    # purity: the bound changes which words are scored, not one bit of a score
    assert np.array_equal(near['scores'][cand].view(np.int32), everything['scores'][cand].view(np.int32))
    plain = device_transcribe(pred, ref.words, max_distance=2, table=False)           # without the table: the same five outputs
    for k in KEYS:
        assert np.array_equal(plain[k].view(np.int32), near[k].view(np.int32)), k


@pytest.mark.parametrize("delta", [0, 1, 3])
def test_distance_filter_counts_and_empty_rows(delta):
    ref, pred = random_case("english", 4)
    N, L = len(ref.y), len(ref.words)
    got = device_transcribe(pred, ref.words, max_distance=delta)
    compare(got, ref, max_distance=delta, name="delta %d" % delta)
    count = (ref.D <= delta).sum(axis=1)
    assert np.array_equal(got['candidates'], count)
    if delta <= 1:                                              # rows without a planted word have nothing that near
        assert (count == 0).any() and (count > 0).any()
        none = count == 0
        assert np.all(got['index'][none] == -1) and np.all(got['score'][none] == -np.inf) and np.all(got['distance'][none] == -1)
    # empty, one-word and clamped spans under the same bound
    spans = [[n * 5, n * 5 + 40] for n in range(N)]
    spans[1], spans[2], spans[3], spans[4] = [7, 7], [L, L], [L - 3, L + 50], [-4, 1]
    spans[0], spans[8] = [L - 18, L - 17], [L - 12, L]         # row 0's own greedy string alone; row 8's three planted words
    got = device_transcribe(pred, ref.words, spans=spans, max_distance=delta)
    compare(got, ref, spans=spans, max_distance=delta, name="delta %d with spans" % delta, need_exact=0)
    assert got['candidates'][1] == 0 and got['candidates'][2] == 0 and got['index'][1] == -1
    assert (got['index'][0], got['distance'][0], got['candidates'][0]) == (L - 18, 0, 1)


def small_case(T, C, words, seed, sharp=2.0, blank=0, unknown=1, rows=6):
    rng = np.random.RandomState(seed)
    y = softmax32(rng.randn(rows, T, C) * sharp)
    return Reference(y, words, blank, unknown), y


def test_one_and_three_columns_and_the_empty_word():
    words = [[], [2], [3], [2, 2], [2, 3], [3, 2, 3], [2, 2, 3], [2, 3, 4, 5], [4]]
    for T in (1, 3):
        ref, y = small_case(T, 6, words, seed=T)
        got = device_transcribe(eval_layout(y), words)
        compare(got, ref, name="T = %d" % T, need_exact=0)
        assert np.all(np.isfinite(got['scores'][:, 0]))                        # K = 0: the sum of the blank's logs
        fits = [len(w) + sum(a == b for a, b in zip(w, w[1:])) <= T for w in words]
        assert np.array_equal(np.isfinite(got['scores'][0]), fits)


def test_repeated_symbols_need_a_column_for_the_blank():
    words = [[2, 2, 3], [2, 3, 3], [2, 3, 2], [4, 4, 4], [2, 2], [4, 4, 4, 4]]     # AAB: 3 symbols + 1 blank = 4 columns
    for T, finite in ((4, [True, True, True, False, True, False]), (3, [False, False, True, False, True, False]),
                      (5, [True, True, True, True, True, False]), (7, [True] * 6)):
        ref, y = small_case(T, 5, words, seed=10 + T)
        got = device_transcribe(eval_layout(y), words)
        compare(got, ref, name="AAB at T = %d" % T, need_exact=0)
        assert np.isfinite(got['scores']).tolist() == [finite] * len(y)


@pytest.mark.parametrize("T", [129, 130])
def test_words_of_63_and_64_symbols(T):
    """Lane 63 holds the last symbol of a 64-symbol word and the blank after it has no lane of its own; 63 symbols are the longest
    word without that.  T = 129 / 130: eight blocks of 16 columns and a tail of one / two."""
    rng = np.random.RandomState(T)
    w64 = rng.randint(2, 8, size=64).tolist()
    apart = [2 + (i % 3) for i in range(64)]                                       # no two neighbours equal
    words = [w64[:63], w64, apart, apart[:63], [7] * 64, [7] * 63, w64[:62], [], [5], [3] * 63 + [4]]
    ref, y = small_case(T, 8, words, seed=T, sharp=1.0, rows=4)
    got = device_transcribe(eval_layout(y), words)
    compare(got, ref, name="63 / 64 symbols at T = %d" % T, need_exact=0)
    assert np.all(np.isfinite(got['scores']))                                       # [7] * 64 needs 127 columns: all of them fit
    near = device_transcribe(eval_layout(y), words, max_distance=200)             # the ballot path scores them too, same bits
    assert np.array_equal(near['scores'].view(np.int32), got['scores'].view(np.int32))


def test_a_word_longer_than_64_symbols_is_read_up_to_the_cap():
    """The Python layer refuses such words; the kernel reads MR_LEXICON_MAX_WORD symbols whatever lex_off says."""
    rng = np.random.RandomState(5)
    long_word = rng.randint(2, 6, size=70).tolist()
    y = softmax32(rng.randn(3, 140, 6))
    got = device_transcribe(eval_layout(y), [long_word, long_word[:64]])
    assert np.array_equal(got['scores'][:, 0].view(np.int32), got['scores'][:, 1].view(np.int32))
    assert np.all(np.isfinite(got['scores'])) and got['index'].tolist() == [0, 0, 0]


def test_exact_zeros_in_the_posterior_flow_through():
    words = [[2, 3], [3], [2], [], [4, 2, 4], [2, 4], [3, 3]]
    y = softmax32(np.random.RandomState(20).randn(6, 6, 5) * 2.0)
    for t, c in [(1, 2), (2, 0), (0, 3), (5, 3), (4, 0), (3, 0), (3, 4)]:
        y[:, t, c] = 0.0
    y[3, :, 2] = 0.0                                                                # one row where class 2 is impossible throughout
    ref = Reference(y, words)
    got = device_transcribe(eval_layout(y), words)
    compare(got, ref, name="zeros", need_exact=0)
    assert not np.isnan(got['scores']).any() and not np.isnan(got['score']).any()
    assert np.all(got['scores'][3, [0, 2, 4, 5]] == -np.inf) and np.isfinite(got['scores'][3, 1])
    all_zero = np.zeros((2, 4, 5), dtype=np.float32)                                # nothing is possible: -1 / -inf / -1
    got = device_transcribe(eval_layout(all_zero), words)
    assert got['index'].tolist() == [-1, -1] and np.all(got['score'] == -np.inf) and got['distance'].tolist() == [-1, -1]
    assert np.all(got['scores'] == -np.inf) and got['candidates'].tolist() == [7, 7]


def test_unknown_in_a_word_and_ids_outside_the_alphabet():
    words = [[2, 1, 3], [2, 3], [1], [2, 6], [2, -1], [3, 2]]
    ref, y = small_case(8, 6, words, seed=21)
    got = device_transcribe(eval_layout(y), words)
    compare(got, ref, name="unknown", need_exact=0)
    assert np.all(got['scores'][:, [0, 2, 3, 4]] == -np.inf) and np.all(np.isfinite(got['scores'][:, [1, 5]]))
    assert got['candidates'].tolist() == [6] * len(y)                               # candidates all the same: the count ignores scores


def test_other_blank_and_unknown_ids():
    rng = np.random.RandomState(22)
    ids = [0, 1, 2, 4, 6, 7]
    words = [rng.choice(ids, size=k).tolist() for k in rng.randint(0, 9, size=60)] + [[3, 4], [4, 3, 0]]
    ref, y = small_case(20, 8, words, seed=22, blank=5, unknown=3, rows=10)         # T = 20: one block of 16-byte loads and a tail
    got = device_transcribe(eval_layout(y), words, blank=5, unknown=3)
    compare(got, ref, name="blank 5 unknown 3", need_exact=0)
    got = device_transcribe(eval_layout(y), words, blank=5, unknown=3, max_distance=4)
    compare(got, ref, max_distance=4, name="blank 5 unknown 3 within 4", need_exact=0)
    assert np.all(got['scores'][:, -2:] == -np.inf)


@pytest.mark.parametrize("kind", ["english", "wide"])
def test_bfloat16_posterior(kind):
    ref32, pred = random_case(kind, 4)
    half = pred.to(torch.bfloat16)
    y = np.ascontiguousarray(half.float().permute(0, 2, 1).cpu().numpy())          # what the kernel reads, as f32
    ref = Reference(y, ref32.words)
    got = device_transcribe(half, ref.words)
    compare(got, ref, name="bf16")
    got = device_transcribe(half, ref.words, max_distance=3)
    compare(got, ref, max_distance=3, name="bf16 within 3")


def test_strided_views_give_the_same_bits():
    ref, pred = random_case("narrow", 4)
    want = device_transcribe(pred, ref.words, max_distance=3)
    tnc = pred.permute(2, 0, 1).contiguous()                                        # [T, N, C] as the decoder's logits lie
    view = tnc.permute(1, 2, 0)
    assert view.stride() != pred.stride() and view.stride(1) == 1
    got = device_transcribe(view, ref.words, max_distance=3)
    compare(got, ref, max_distance=3, name="[T, N, C] view")
    for k in KEYS + ('scores',):
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
    # the wide alphabet is read from global memory as it is scored: 16-byte loads there, single loads here
    ref, pred = random_case("wide", 4)
    want = device_transcribe(pred, ref.words, max_distance=3)
    got = device_transcribe(pred.permute(2, 0, 1).contiguous().permute(1, 2, 0), ref.words, max_distance=3)
    for k in KEYS + ('scores',):
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
    # class rows that are contiguous but not 16-byte aligned: the same values, the same bits
    padded = torch.zeros((pred.shape[0], pred.shape[1], pred.shape[2] + 4), device=DEV)
    padded[:, :, 1:-3] = pred
    assert padded[:, :, 1:-3].data_ptr() % 16 == 4 and padded.stride(1) % 4 == 0
    got = device_transcribe(padded[:, :, 1:-3], ref.words, max_distance=3)
    for k in KEYS + ('scores',):
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k


@pytest.mark.parametrize("kind", ["english", "narrow", "wide"])
def test_log_probabilities_in_give_the_same_bits(kind):
    ref, pred = random_case(kind, 4)
    pred = pred.clone()
    pred[0, 3, :] = 0.0                                                             # log 0 = -inf comes in as it is
    want = device_transcribe(pred, ref.words, max_distance=3)
    logs = pred.double().log().float()                                              # the f32 nearest to the log, as the header says
    got = device_transcribe(logs, ref.words, max_distance=3, log_probs=True)
    for k in KEYS + ('scores',):
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
    assert np.isfinite(want['score']).any()


def test_duplicated_words_lowest_index_and_equal_bits():
    ref, pred = random_case("english", 4)
    base = ref.words[-3]                                                            # row 20's greedy string: its most probable word
    n = 4 * ((len(ref.words) - 300) // 3 - 1)
    words = [[9, 9, 9]] * 3 + [base] * 5 + [base[:-1]] * 4 + [base] * 300
    got = device_transcribe(pred, words)
    assert got['index'][n] == 3
    bits = got['scores'][:, 3:8].view(np.int32)
    assert np.all(bits == bits[:, :1]) and np.all(got['scores'][:, 12:].view(np.int32) == bits[:, :1])
    spans = [[5, 312]] * len(ref.y)
    spans[n] = [12, 312]
    got2 = device_transcribe(pred, words, spans=spans)
    assert got2['index'][n] == 12 and got2['score'][n].view(np.int32) == got['score'][n].view(np.int32)
    assert np.all(got2['index'] >= 5)
    # every row: the winner is the lowest index among the words with the winning bits
    for r in range(len(ref.y)):
        top = got['scores'][r].max()
        assert got['index'][r] == int(np.argmax(got['scores'][r] == top)) and got['score'][r] == top


def test_one_word_spans_reproduce_the_table_bit_for_bit():
    ref, pred = random_case("narrow", 1)
    full = device_transcribe(pred, ref.words)
    N = len(ref.y)
    for l in list(range(0, 40)) + [len(ref.words) - 1]:
        one = device_transcribe(pred, ref.words, spans=[[l, l + 1]] * N, table=False)
        assert np.array_equal(one['score'].view(np.int32), full['scores'][:, l].view(np.int32)), l
        finite = np.isfinite(full['scores'][:, l])
        assert np.array_equal(one['index'], np.where(finite, l, -1)) and one['candidates'].tolist() == [1] * N
    # ... and a row's score does not depend on the other rows of the batch
    alone = device_transcribe(pred[5:6], ref.words)
    assert np.array_equal(alone['scores'].view(np.int32), full['scores'][5:6].view(np.int32))


@pytest.mark.parametrize("place", ["first", "middle", "last"])
def test_one_row_against_five_thousand_words(place):
    ref, pred = random_case("english", 4)
    rng = np.random.RandomState(30)
    L = 5000
    words = [rng.randint(2, 38, size=k).tolist() for k in rng.randint(6, 16, size=L)]
    at = {"first": 0, "middle": L // 2 + 77, "last": L - 1}[place]
    words[at] = ref.words[300]                                                      # row 0's greedy string
    sample = sorted(set(range(0, L, 50)) | {at})
    sub = Reference(ref.y[:1], [words[i] for i in sample])
    for delta in (-1, 40):                                                          # many workgroups on either path
        got = device_transcribe(pred[:1], words, max_distance=delta)
        assert got['index'][0] == at and got['distance'][0] == 0 and got['candidates'][0] == L
        assert np.abs(got['scores'][0, sample].astype(np.float64) - sub.S64[0]).max() <= sub.tol
        assert got['score'][0] == got['scores'][0].max() == got['scores'][0, at]


def test_three_hundred_rows_seven_words():
    rng = np.random.RandomState(31)
    words = [rng.randint(2, 6, size=k).tolist() for k in (0, 1, 2, 3, 3, 5, 9)]
    ref, y = small_case(12, 6, words, seed=31, rows=300)
    pred = eval_layout(y)
    compare(device_transcribe(pred, words), ref, name="300 rows")
    compare(device_transcribe(pred, words, max_distance=4), ref, max_distance=4, name="300 rows within 4", need_exact=0)


def spelled(charset, columns, T=10, floor=1e-4):
    """A [1, C, 1, T] posterior: columns is a list of {character or '' (blank): probability}; the rest of each column's mass is
    spread over all classes, the columns after the list are blank."""
    C = len(charset)
    y = np.full((T, C), floor, dtype=np.float64)
    for t in range(T):
        given = columns[t] if t < len(columns) else {'': 1.0}
        for ch, p in given.items():
            y[t, getattr(charset, 'blank', 0) if ch == '' else charset.index(ch)] += p
    y /= y.sum(axis=1, keepdims=True)
    return torch.from_numpy(y.T.astype(np.float32)).reshape(1, C, 1, T).to(DEV)


def helo(charset, second_l):
    """The arg-max path spells HELO; the rest of the mass sits on a second L in the gap, or on P in O's column."""
    gap = {'': 0.55, 'L': 0.4} if second_l else {'': 0.97}
    last = {'O': 0.9} if second_l else {'O': 0.5, 'P': 0.45}
    return spelled(charset, [{'H': 0.9}, {'E': 0.9}, {'L': 0.9}, {'': 0.9}, gap, last])


def test_the_rule_itself_help_or_hello():
    cs = EnglishCharset()
    lex = Lexicon(["HELP", "HELLO"], cs)
    for second_l, want in ((True, 1), (False, 0)):
        pred = helo(cs, second_l)
        ids, _ = ctc_greedy_decode(pred, blank=cs.blank, unknown=cs.unknown)
        assert cs.label_to_string(ids[0].cpu().numpy()) == "HELO"
        near = lex.nearest(ids)
        assert near['index'].tolist() == [0] and near['distance'].tolist() == [1]  # both one edit away: the first listed
        for delta in (None, 1):
            found = lex.transcribe(pred, max_distance=delta, all_scores=True)
            assert found['index'].tolist() == [want] and found['distance'].tolist() == [1]
            assert found['candidates'].tolist() == [2] and found['length'].tolist() == [4]
            scores = found['scores'][0].cpu().numpy()
            assert scores[want] > scores[1 - want] + 1.0 and found['score'].item() == scores[want]
        assert lex.transcribe(pred, max_distance=0)['index'].tolist() == [-1]     # HELO itself is not a word


def test_python_layer_layouts_spans_and_keys():
    cs = EnglishCharset()
    ref, pred = random_case("english", 1)
    texts = [cs.label_to_string(np.array(w)) for w in ref.words]
    keep = [l for l, (t, w) in enumerate(zip(texts, ref.words)) if len(t) == len(w)]
    lex = Lexicon([texts[l] for l in keep], cs)
    assert [lex.sym[lex.off[i]:lex.off[i + 1]].tolist() for i in range(len(lex))] == [ref.words[l] for l in keep]
    want = device_transcribe(pred, [ref.words[l] for l in keep], blank=cs.blank, unknown=cs.unknown, max_distance=2)
    for given in (pred, pred.unsqueeze(2)):                                         # [N, C, T] and [N, C, 1, T]
        found = lex.transcribe(given, max_distance=2, all_scores=True)
        assert sorted(found) == ['candidates', 'distance', 'index', 'length', 'score', 'scores']
        for k in KEYS + ('scores',):
            assert np.array_equal(found[k].cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    assert sorted(lex.transcribe(pred)) == sorted(KEYS)
    grouped, spans = Lexicon.grouped([["AB", "ABC"], [], ["B"]] * 8, cs)
    found = grouped.transcribe(pred, spans)
    assert found['candidates'].tolist() == [2, 0, 1] * 8 and found['index'].tolist()[1::3] == [-1] * 8
    assert all(i in (3 * k, 3 * k + 1) for k, i in enumerate(found['index'].tolist()[0::3]))
    empty = lex.transcribe(pred[:0])
    assert all(tuple(empty[k].shape) == (0,) and empty[k].is_cuda for k in KEYS)
    f64 = lex.transcribe(pred.double(), max_distance=2)                             # other types go through f32
    assert torch.equal(f64['index'].cpu(), torch.from_numpy(want['index']))


@pytest.mark.parametrize("log_probs", [False, True])
def test_case_folding_charset_scores_the_folded_alphabet(log_probs):
    cs = EnglishPrintableCharset(case_sensitive=True)
    fold = upper_fold_table(cs)
    assert fold is not None
    C, N, T = len(cs), 6, 12
    rng = np.random.RandomState(40)
    letters = [cs.index(ch) for ch in "abcABC"]
    logits = np.full((N, T, C), -6.0)
    logits[:, :, letters] = rng.randn(N, T, len(letters)) * 2
    logits[:, :, cs.blank] = rng.randn(N, T) * 2
    y = softmax32(logits)
    entries = ["abc", "ABC", "Cab", "", "bb", "aAa", "cB"]
    lex = Lexicon(entries, cs)
    pred = eval_layout(y)
    found = lex.transcribe(pred.log() if log_probs else pred, log_probs=log_probs, all_scores=True)
    q = Q.fold_posterior(y, fold).astype(np.float32)
    words = [lex.sym[lex.off[l]:lex.off[l + 1]].tolist() for l in range(len(lex))]
    ref = Reference(q, words, cs.blank, cs.unknown)
    got = found['scores'].cpu().numpy()
    # the folded posterior is summed in f32 on the device in another order than numpy's float64: its rounding (a few 1e-7
    # relative per column, T columns) joins the tolerance of the recursion
    tol = ref.tol + T * 4e-7 * (2 if log_probs else 1)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref.S64)) and np.abs(got - ref.S64)[np.isfinite(got)].max() <= tol
    assert np.array_equal(got[:, 0].view(np.int32), got[:, 1].view(np.int32))      # "abc" and "ABC" are one word
    ids, _ = ctc_greedy_decode(pred, blank=cs.blank, unknown=cs.unknown)
    D, length = R.distance_table(ids.cpu().numpy(), words, cs.blank, cs.unknown, fold)
    assert found['length'].cpu().tolist() == length.tolist()
    index = found['index'].cpu().numpy()
    assert np.array_equal(found['distance'].cpu().numpy(), D[np.arange(N), index])
    assert np.all(ref.S64[np.arange(N), index] >= ref.S64.max(axis=1) - 2 * tol)


def test_capturable_in_a_graph():
    ref, pred = random_case("english", 4)
    cs = EnglishCharset()
    lex = Lexicon([cs.label_to_string(np.array(w)) for w in ref.words], cs)
    other = pred.flip(0).contiguous()
    eager = {k: v.clone() for k, v in lex.transcribe(pred, max_distance=3, all_scores=True).items()}   # the warm-up call
    eager_other = {k: v.clone() for k, v in lex.transcribe(other, max_distance=3, all_scores=True).items()}
    static = pred.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        found = lex.transcribe(static, max_distance=3, all_scores=True)
    for source, want in ((pred, eager), (other, eager_other)):                      # two replays on different posteriors
        static.copy_(source)
        graph.replay()
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(found[key].view(torch.int32), want[key].view(torch.int32)), key
    assert not torch.equal(eager['index'], eager_other['index'])


def test_bad_arguments_are_refused():
    ref, pred = random_case("english", 1)
    words = ref.words[:5]
    with pytest.raises(RuntimeError, match="mr_lexicon_transcribe: T=0"):
        device_transcribe(pred, words, T=0)
    with pytest.raises(RuntimeError, match="C=1 classes"):
        device_transcribe(pred, words, C=1)
    with pytest.raises(RuntimeError, match="bad dtype 2"):
        device_transcribe(pred, words, dtype=2)
    with pytest.raises(RuntimeError, match="blank=38 is not a class"):
        device_transcribe(pred, words, blank=38)
    lex = Lexicon(["AB"], EnglishCharset())
    with pytest.raises(NotImplementedError):
        lex.transcribe(torch.zeros((1, 38, 1, 8)))
    with pytest.raises(ValueError, match="37 classes"):
        lex.transcribe(torch.zeros((1, 37, 1, 8), device=DEV))
    with pytest.raises(ValueError):
        lex.transcribe(torch.zeros((1, 38, 2, 8), device=DEV))
    with pytest.raises(ValueError, match="no columns"):
        lex.transcribe(torch.zeros((1, 38, 1, 0), device=DEV))
