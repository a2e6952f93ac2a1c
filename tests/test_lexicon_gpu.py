"""mr_lexicon_nearest (csrc/lexicon.hip) and its Python layers -- `Lexicon.nearest` / `contains`, the measurer's lexicon split --
against tests/_lexicon_ref.py.  Every comparison is exact: index, distance and length of every row."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lexicon_ref as R  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.charsets import EnglishCharset, EnglishPrintableCharset, upper_fold_table  # noqa: E402
from megreader_amd.ops.lexicon import Lexicon  # noqa: E402
from megreader_amd.structure.measurers import SequenceRecognitionMeasurer  # noqa: E402
from megreader_amd.structure.representers import CTCRepresenter  # noqa: E402

DEV = "cuda"


def device_nearest(preds, words, C, blank=0, unknown=1, fold=None, spans=None):
    """The C entry point on raw ids: (index, distance, length) as numpy.  Outputs start as garbage: the call writes every row."""
    preds = np.asarray(preds, dtype=np.int32).reshape(len(preds), -1)
    N, S = preds.shape
    off = np.zeros(len(words) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(w) for w in words])
    sym = np.array([s for w in words for s in w] + [0], dtype=np.int32)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    d_preds, d_sym, d_off, d_fold, d_span = t(preds), t(sym), t(off), t(fold), t(spans)
    out = torch.full((3, N), 12345, dtype=torch.int32, device=DEV)
    call("mr_lexicon_nearest", ptr(d_preds) if N and S else 0, S, N, blank, unknown, ptr(d_fold), ptr(d_sym), ptr(d_off),
         len(words), ptr(d_span), C, ptr(out[0]), ptr(out[1]), ptr(out[2]))
    return tuple(out.cpu().numpy())


def check(preds, words, C, table=None, **kw):
    """The device against the restatement; `table`: a distance table of these rows and words computed before (R.distance_table)."""
    got = device_nearest(preds, words, C, **kw)
    want = R.nearest_rows(preds, words, **kw) if table is None else R.nearest_in_table(*table, spans=kw.get('spans'))
    for name, g, w in zip(("index", "distance", "length"), got, want):
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(w)), (name, g.tolist(), w.tolist())
    return got


def random_case(seed, N, S, L, alphabet, blank=0, unknown=1, max_word=64, classes=None):
    """Rows of S ids with blanks and unknowns scattered through them; words of 0..max_word symbols."""
    rng = np.random.RandomState(seed)
    ids = [i for i in range(alphabet + 2) if i not in (blank, unknown)][:alphabet] if classes is None else classes
    preds = rng.choice(ids, size=(N, S))
    holes = rng.rand(N, S)
    preds[holes < 0.25] = blank
    preds[holes > 0.9] = unknown
    preds[0] = blank                                                    # one empty row
    words = [rng.choice(ids, size=k).tolist() for k in rng.randint(0, max_word + 1, size=L)]
    return preds, words


@pytest.mark.parametrize("alphabet", [4, 36])
def test_random_rows_and_the_tie_break(alphabet):
    preds, words = random_case(alphabet, N=37, S=40, L=300, alphabet=alphabet)
    index, distance, _ = check(preds, words, C=alphabet + 2)
    if alphabet == 4:       # most rows have several words at the minimum: the lowest index must win
        D, _ = R.distance_table(preds, words)
        ties = int(((D == distance[:, None]).sum(axis=1) > 1).sum())
        print("rows with more than one nearest word: %d of %d" % (ties, len(preds)))
        assert ties > len(preds) // 2


def boundary_words(rng):
    w64 = rng.randint(2, 8, size=64).tolist()
    return [[], [3], rng.randint(2, 8, size=63).tolist(), w64, w64[:-1] + [w64[-1] % 6 + 2], [7] * 64, w64[:63], [2]]


def row_of(symbols, S):
    """The symbols with a blank in front, an unknown after the first symbol and blank padding: S ids."""
    symbols = list(symbols)
    row = [0] + symbols[:1] + [1] + symbols[1:]
    return row + [0] * (S - len(row))


def test_boundary_lengths_fast_path():
    rng = np.random.RandomState(1)
    words = boundary_words(rng)
    w64 = words[3]
    rows = [[], [3], [4], rng.randint(2, 8, size=63).tolist(), words[2], rng.randint(2, 8, size=64).tolist(),
            w64,                                   # equal to a 64-symbol word: distance 0
            w64[:-1] + [w64[-1] % 6 + 2],          # differs from it only in the last symbol (and equals the next word)
            w64[:-1] + [9],                        # differs from both only in the last symbol: distance 1, lowest index
            [9] + w64[1:], [7] * 64, [7] * 63]
    preds = [row_of(r, 70) for r in rows]
    index, distance, length = check(preds, words, C=10)
    assert length.tolist() == [len(r) for r in rows]
    assert (index[6], distance[6]) == (3, 0) and (index[7], distance[7]) == (4, 0) and (index[8], distance[8]) == (3, 1)
    # every row against every word on its own (one-word ranges): the whole table of boundary distances
    table = R.distance_table(preds, words)
    for l in range(len(words)):
        check(preds, words, C=10, table=table, spans=[[l, l + 1]] * len(preds))


def test_rows_longer_than_a_machine_word_and_mixed_batches():
    rng = np.random.RandomState(2)
    words = boundary_words(rng)
    w64 = words[3]
    long_rows = [rng.randint(2, 8, size=65).tolist(), w64 + [5], rng.randint(2, 8, size=130).tolist(), w64 + w64 + [2, 3],
                 [7] * 130]
    S = 140
    check([row_of(r, S) for r in long_rows], words, C=10)
    mixed = [[], long_rows[0], [3], long_rows[2], w64, long_rows[1], w64[:63], long_rows[3]]
    index, distance, length = check([row_of(r, S) for r in mixed], words, C=10)
    assert length.tolist() == [len(r) for r in mixed]
    assert (index[5], distance[5]) == (3, 1)       # the 64-symbol word plus one symbol
    table = R.distance_table([row_of(r, S) for r in mixed], words)
    for l in range(len(words)):
        check([row_of(r, S) for r in mixed], words, C=10, table=table, spans=[[l, l + 1]] * len(mixed))


def test_other_blank_and_unknown_ids():
    preds, words = random_case(3, N=20, S=30, L=120, alphabet=6, blank=5, unknown=3, max_word=20)
    check(preds, words, C=8, blank=5, unknown=3)


def test_fold_table_joins_upper_and_lower_case():
    cs = EnglishPrintableCharset(case_sensitive=True)
    fold = upper_fold_table(cs)
    rng = random.Random(4)
    letters = "abcdeABCDE"
    texts = ["".join(rng.choice(letters) for _ in range(rng.randrange(0, 12))) for _ in range(60)]
    words = [[fold[cs.index(ch)] for ch in t] for t in texts]                      # the host folds the words
    preds = np.zeros((25, 16), dtype=np.int32)
    for n in range(25):
        t = "".join(rng.choice(letters) for _ in range(rng.randrange(0, 14)))
        preds[n, :len(t)] = [cs.index(ch) for ch in t]                             # ... the kernel the predictions
    check(preds, words, C=len(cs), fold=fold)
    lower, upper = [[cs.index(ch) for ch in "abcde"]], [[fold[cs.index(ch)] for ch in "ABCDE"]]
    got = device_nearest(lower, upper, len(cs), fold=fold)
    assert (got[0][0], got[1][0]) == (0, 0)
    assert device_nearest(lower, upper, len(cs))[1][0] == 5                        # without the table they are 5 apart


def test_a_word_that_holds_unknown_is_never_at_distance_zero():
    words = [[4, 1, 5], [1], [4, 5, 1], [1, 1]]
    preds = [[4, 1, 5, 0], [4, 5, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [4, 0, 5, 1]]
    index, distance, length = check(preds, words, C=6)
    assert (distance > 0).all() and length.tolist() == [2, 2, 0, 0, 2]
    assert distance.tolist() == [1, 1, 1, 1, 1]


def test_wide_alphabet_dense_table():
    C = 5360
    classes = np.concatenate([np.arange(2, 40), np.arange(C - 40, C)])             # ids up to C - 1
    preds, words = random_case(6, N=24, S=36, L=200, alphabet=0, max_word=40, classes=classes)
    preds[1, :3] = C - 1
    words[0] = [C - 1] * 3
    index, distance, _ = check(preds, words, C=C)
    assert (preds[:, :] == C - 1).any() and any(C - 1 in w for w in words)


def test_wider_alphabet_compact_table():
    C = 70000
    classes = np.concatenate([np.arange(2, 20), np.arange(9000, 9020), np.arange(C - 30, C)])
    preds, words = random_case(7, N=24, S=70, L=200, alphabet=0, max_word=64, classes=classes)
    full = np.arange(C - 64, C)[::-1].tolist()                                     # 64 distinct symbols: a full compact table
    preds[2] = full + [0] * 6
    words[5] = full
    index, distance, length = check(preds, words, C=C)
    assert (index[2], distance[2], length[2]) == (5, 0, 64)
    long_row = row_of(np.arange(C - 100, C).tolist(), 110)                        # ... and a row past 64 symbols beside it
    check([long_row, full + [0] * 46], words, C=C)


def test_spans():
    preds, words = random_case(8, N=12, S=20, L=50, alphabet=5, max_word=12)
    spans = [[0, 50], [7, 7], [50, 50], [0, 0], [9, 10], [49, 50], [10, 30], [20, 40], [25, 50], [0, 1], [3, 50], [30, 31]]
    index, distance, _ = check(preds, words, C=7, spans=spans)
    for n in (1, 2, 3):
        assert (index[n], distance[n]) == (-1, -1)                                 # empty ranges
    assert index[4] == 9 and index[5] == 49 and index[11] == 30                    # one-word ranges


def test_duplicated_words_give_the_lowest_index():
    word = [2, 3, 4, 5]
    words = [[9, 9, 9]] * 3 + [word] * 5 + [[2, 3, 4]] * 4 + [word] * 300
    preds = [word + [0], [2, 3, 4, 0, 0], [9, 9, 9, 9, 0], [2, 3, 5, 5, 0]]
    index, distance, _ = check(preds, words, C=10)
    assert index.tolist() == [3, 8, 0, 3] and distance.tolist() == [0, 0, 1, 1]
    index, _, _ = check(preds, words, C=10, spans=[[5, 312], [9, 312], [1, 312], [12, 312]])
    assert index.tolist() == [5, 9, 1, 12]


def test_one_word_no_word_no_row():
    preds, _ = random_case(9, N=5, S=10, L=1, alphabet=4)
    check(preds, [[2, 3]], C=6)
    index, distance, length = check(preds, [], C=6)
    assert index.tolist() == [-1] * 5 and distance.tolist() == [-1] * 5
    assert length.tolist() == [len(R.compact(r)) for r in preds]
    lex = Lexicon(["AB", "CD"], EnglishCharset())
    found = lex.nearest(torch.zeros((0, 7), dtype=torch.int32, device=DEV))
    assert all(tuple(found[k].shape) == (0,) and found[k].dtype == torch.int32 and found[k].is_cuda
               for k in ('index', 'distance', 'length'))
    found = lex.nearest(torch.zeros((3, 0), dtype=torch.int32, device=DEV))       # S == 0: every row is empty
    assert found['length'].tolist() == [0, 0, 0] and found['distance'].tolist() == [2, 2, 2] and found['index'].tolist() == [0] * 3


def test_bad_arguments_are_refused():
    cap = 4096
    ids = torch.zeros((1, cap + 1), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="mr_lexicon_nearest: S=%d exceeds" % (cap + 1)):
        Lexicon(["AB"], EnglishCharset()).nearest(ids)
    with pytest.raises(RuntimeError, match="C=1 classes"):
        device_nearest([[0, 0]], [[0]], C=1)
    with pytest.raises(NotImplementedError):
        Lexicon(["AB"], EnglishCharset()).nearest(torch.zeros((1, 4), dtype=torch.int32))


@pytest.mark.parametrize("place", ["first", "middle", "last"])
def test_one_row_spread_over_many_workgroups(place):
    rng = np.random.RandomState(10)
    L = 5000
    words = [rng.randint(2, 12, size=k).tolist() for k in rng.randint(6, 16, size=L)]
    rows = [rng.randint(2, 12, size=11).tolist() for _ in range(3)]
    at = {"first": [0, 1, 2], "middle": [L // 2 + 77, L // 2 + 377, L // 2 + 677], "last": [L - 1, L - 2, L - 3]}[place]
    for k, r in zip(at, rows):
        words[k] = r                                                               # each row's own best word, found nowhere else
    preds = [row_of(r, 16) for r in rows]
    index, distance, _ = check(preds, words, C=12)
    assert index.tolist() == at and distance.tolist() == [0, 0, 0]


def test_many_rows_few_words():
    preds, words = random_case(11, N=300, S=12, L=7, alphabet=4, max_word=10)
    check(preds, words, C=6)


def encode_rows(charset, texts, S):
    rows = np.zeros((len(texts), S), dtype=np.int32)
    for n, t in enumerate(texts):
        rows[n, :len(t)] = [charset.index(ch) for ch in t]
    return rows


def test_lexicon_nearest_and_contains_on_strings():
    cs = EnglishCharset()
    entries = ["HELLO", "WORLD", "hello", "HELP", "", "A-B", "X" * 64, "W0RLD"]
    lex = Lexicon(entries, cs)
    texts = ["HELLO", "hello", "HELO", "WORLD", "WORLDS", "", "AB", "A?B", "X" * 64, "X" * 63, "W0RLD", "ZZZZZZ"]
    ids = torch.from_numpy(encode_rows(cs, texts, 70)).to(DEV)
    found = lex.nearest(ids)
    decoded = [cs.label_to_string(r) for r in ids.cpu().numpy()]
    folded = {w.upper() for w in entries if all(ch.upper() in cs._lut for ch in w)}   # entries that a decoded string can spell
    assert lex.contains(ids).cpu().tolist() == [s in folded for s in decoded]
    want = R.nearest_rows(ids.cpu().numpy(), [sy.tolist() for sy in np.split(lex.sym, lex.off[1:-1])])
    for key, w in zip(('index', 'distance', 'length'), want):
        assert torch.equal(found[key].cpu(), torch.from_numpy(w)), key
    assert lex.strings(found['index'])[:5] == ["HELLO", "HELLO", "HELLO", "WORLD", "WORLD"]
    grouped, spans = Lexicon.grouped([["HELP"], [], ["WORLD", "HELLO"]] * 4, cs)
    got = grouped.nearest(ids, spans)
    assert got['index'].cpu().tolist()[:3] == [0, -1, 2] and got['distance'].cpu().tolist()[:3] == [2, -1, 1]
    assert grouped.contains(ids, spans).cpu().tolist()[:4] == [False, False, False, False]


def test_measurer_lexicon_split():
    cs = EnglishCharset()
    T = 24
    labels = ["HELLO", "WORLD", "HELP", "MEGVII", "", "ABC", "hello", "W0RLD"]
    spelt = ["HELLO", "WORLO", "HELP", "MEGVI", "A", "ABD", "HELLO", "WORLD"]
    pred = torch.zeros((len(labels), len(cs), 1, T), dtype=torch.float32)
    for n, text in enumerate(spelt):
        ids = [0] * T
        ids[1:2 * len(text):2] = [cs.index(ch) for ch in text]
        pred[n, ids, 0, torch.arange(T)] = 1.0
    batch = {'label': torch.stack([torch.from_numpy(cs.string_to_label(t, 32)) for t in labels]).to(DEV)}
    output = CTCRepresenter(charset=cs).represent(batch, pred.to(DEV))
    assert [o['pred_string'] for o in output] == spelt
    entries = ["HELLO", "world", "HELP", "ABD", "MEGVII", "W0RLD", "WORLD2"]        # 'world' is lower case: never a member
    plain = SequenceRecognitionMeasurer(charset=cs).measure(batch, output)
    assert sorted(plain) == ['accuracy', 'edit_distance']
    with_lexicon = SequenceRecognitionMeasurer(charset=cs, lexicon=entries).measure(batch, output)
    assert sorted(with_lexicon) == ['accuracy', 'edit_distance', 'in_lexicon']
    label_strings = [o['label_string'] for o in output]
    assert with_lexicon['in_lexicon'] == R.in_lexicon(label_strings, entries)
    assert with_lexicon['in_lexicon'] == [True, False, True, True, False, False, True, True]
    corrected = SequenceRecognitionMeasurer(charset=cs, lexicon=Lexicon(entries, cs), correct=True).measure(batch, output)
    assert sorted(corrected) == ['accuracy', 'edit_distance', 'in_lexicon', 'lexicon_accuracy']
    assert corrected['in_lexicon'] == with_lexicon['in_lexicon']
    # restated: the label (upper-cased) equals the upper-cased lexicon word nearest to the prediction (lowest index on ties, in
    # the measurer's order: members first)
    order = [w for w in entries if w == w.upper()] + [w for w in entries if w != w.upper()]
    enc = [[cs.index(ch) for ch in w] for w in order]
    index, _, _ = R.nearest([o['pred_ids'].cpu().tolist() for o in output], enc)
    want = [label_strings[n].upper() == order[index[n]].upper() for n in range(len(labels))]
    assert corrected['lexicon_accuracy'] == want
    assert want == [True, True, True, True, False, False, True, False]
    for m in (with_lexicon, corrected):                                            # the non-lexicon keys: bit-identical
        assert m['accuracy'] == plain['accuracy'] and m['edit_distance'] == plain['edit_distance']
    gathered = SequenceRecognitionMeasurer(charset=cs, lexicon=entries, correct=True).gather_measure([corrected, corrected])
    assert gathered['lexicon_accuracy'].avg == sum(want) / len(want) and len(gathered) == 7


def test_capturable_in_a_graph():
    cs = EnglishCharset()
    rng = random.Random(12)
    entries = ["".join(rng.choice("ABCDE") for _ in range(rng.randrange(1, 9))) for _ in range(700)]
    lex = Lexicon(entries, cs)
    texts = ["".join(rng.choice("ABCDE") for _ in range(rng.randrange(0, 10))) for _ in range(9)]
    ids = torch.from_numpy(encode_rows(cs, texts, 12)).to(DEV)
    other = torch.from_numpy(encode_rows(cs, texts[::-1], 12)).to(DEV)
    eager = {k: v.clone() for k, v in lex.nearest(ids).items()}                    # the warm-up call before the capture
    eager_other = {k: v.clone() for k, v in lex.nearest(other).items()}
    static = ids.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        found = lex.nearest(static)
    for source, want in ((ids, eager), (other, eager_other)):                      # two replays, the second on other rows
        static.copy_(source)
        graph.replay()
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(found[key], want[key]), key
