"""GPU greedy decode + metrics (csrc/pipeline.hip, megreader_amd.ops.decode / structure.representers / measurers)
bit-exact against the golden vectors produced by the unmodified reference and against oracle/decode.py on adversarial
and random inputs (ties, unknown runs, T > 64 = several wave chunks, non-contiguous layouts, bf16 / f64 scores).
Second half: sequences of 64 symbols and more through mr_seq_measure (every output of every row, up to the length cap and the
refusal past it), the decoders at 5 360 classes, with other blank / unknown ids, on empty batches, on constructed carries over the
64-step chunk boundary and, in 2-D, on signed scores and masks."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd.ops.decode import ctc2d_greedy_decode, ctc_greedy_decode, sequence_measure  # noqa: E402
from megreader_amd.structure.measurers import SequenceRecognitionMeasurer  # noqa: E402
from megreader_amd.structure.representers import CTCRepresenter, CTCRepresenter2D  # noqa: E402
from oracle.decode import greedy_decode, greedy_decode_2d, measure  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(os.path.join(golden_dir, "decode_golden.pt"), weights_only=False)


def test_decode_1d_matches_reference_golden(golden):
    ids, ln = ctc_greedy_decode(golden['pred_1d'].to(DEV))
    assert torch.equal(ids.cpu(), golden['decode_1d'])
    assert ln.cpu().tolist() == [int((r != 0).sum()) for r in golden['decode_1d']]
    out = CTCRepresenter().represent({'label': golden['labels']}, golden['pred_1d'].to(DEV))
    assert [o['pred_string'] for o in out] == golden['pred_strings_1d']
    assert [o['label_string'] for o in out] == golden['label_strings']
    m = SequenceRecognitionMeasurer().measure({'label': golden['labels']}, out)
    assert m['accuracy'] == golden['accuracy_1d'] and m['edit_distance'] == golden['edit_distance_1d']


def test_decode_2d_matches_reference_golden(golden):
    cl, mk = golden['classify'].to(DEV), golden['mask'].to(DEV)
    ids, _ = ctc2d_greedy_decode(cl, mk)
    assert torch.equal(ids.cpu(), golden['decode_2d'])
    # NHWC-strided inputs (what the HIP head produces): same answer
    cl2 = cl.contiguous(memory_format=torch.channels_last)
    mk2 = mk.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    ids2, _ = ctc2d_greedy_decode(cl2, mk2)
    assert torch.equal(ids2.cpu(), golden['decode_2d'])
    out = CTCRepresenter2D().represent({'label': golden['labels']}, (cl, mk))
    assert [o['pred_string'] for o in out] == golden['pred_strings_2d']
    m = SequenceRecognitionMeasurer().measure({'label': golden['labels']}, out)
    assert m['accuracy'] == golden['accuracy_2d'] and m['edit_distance'] == golden['edit_distance_2d']


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("N,C,T", [(256, 38, 33), (7, 5, 1), (3, 38, 64), (5, 38, 65), (4, 100, 200)])
def test_decode_1d_random_vs_oracle(dtype, N, C, T):
    g = torch.Generator().manual_seed(N * 1000 + T)
    p = torch.rand(N, C, 1, T, generator=g)
    p[:, :3] *= 1.6                                       # plenty of blank / unknown / class-2 runs
    p = (p * 8).round() / 8                               # coarse grid: many exact ties, exactly representable in bf16
    p = p.to(dtype)
    want = greedy_decode(p.double().numpy())
    ids, ln = ctc_greedy_decode(p.to(DEV))
    assert np.array_equal(ids.cpu().numpy(), want)
    assert ln.cpu().tolist() == [int((r != 0).sum()) for r in want]
    # permuted memory layout ([T, N, C] storage viewed as [N, C, 1, T])
    q = p[:, :, 0, :].permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0).unsqueeze(2)
    ids2, _ = ctc_greedy_decode(q)
    assert np.array_equal(ids2.cpu().numpy(), want)


@pytest.mark.parametrize("N,C,H,W", [(256, 38, 8, 32), (5, 38, 4, 16), (3, 7, 1, 70), (2, 38, 3, 130)])
def test_decode_2d_random_vs_oracle(N, C, H, W):
    g = torch.Generator().manual_seed(N + W)
    cl = ((torch.rand(N, C, H, W, generator=g) * 8).round() / 8)
    mk = ((torch.rand(N, 1, H, W, generator=g) * 4).round() / 4)
    want = greedy_decode_2d(cl.numpy(), mk.numpy())
    ids, ln = ctc2d_greedy_decode(cl.to(DEV), mk.to(DEV))
    assert np.array_equal(ids.cpu().numpy(), want)
    assert ln.cpu().tolist() == [int((r != 0).sum()) for r in want]


def test_measure_random_vs_oracle():
    g = torch.Generator().manual_seed(9)
    N = 300
    lab = torch.randint(0, 12, (N, 32), generator=g, dtype=torch.int32)
    pred = lab.clone()
    # edits: substitutions, deletions (-> blank), unknowns, shifted copies, empty labels, full-length sequences
    noise = torch.rand(N, 32, generator=g)
    pred[noise < 0.15] = torch.randint(0, 12, (int((noise < 0.15).sum()),), generator=g, dtype=torch.int32)
    pred[5] = 0
    lab[6] = 0
    lab[7] = torch.arange(32, dtype=torch.int32) % 10 + 2
    pred[7] = lab[7].roll(3)
    pred[8] = lab[8]
    pred2 = torch.cat([pred, torch.randint(0, 12, (N, 8), generator=g, dtype=torch.int32)], dim=1)   # S2 != S
    for p in (pred, pred2):
        acc, eds = measure(lab.numpy(), p.numpy(), charset=[None, None] + list("ABCDEFGHIJ"))
        m = sequence_measure(lab.to(DEV), p.to(DEV))
        assert m['accuracy'].cpu().tolist() == acc
        assert m['edit_distance'].cpu().tolist() == eds        # identical IEEE double operations
    # case folding table: ids 2..6 <-> 7..11 are the same letters in another case
    fold = torch.arange(12, dtype=torch.int32)
    fold[7:12] = torch.arange(2, 7, dtype=torch.int32)
    cs = [None, None] + list("ABCDE") + list("abcde")
    acc, eds = measure(lab.numpy(), pred.numpy(), charset=cs)
    m = sequence_measure(lab.to(DEV), pred.to(DEV), fold=fold)
    assert m['accuracy'].cpu().tolist() == acc and m['edit_distance'].cpu().tolist() == eds


# ------------------------------------------------------------------------------------------- sequences past one wave
# mr_seq_measure keeps rows with both sides <= 63 symbols on the anti-diagonal path and sends longer rows through the row-by-row
# path; every output of every row is compared exactly with oracle/decode.py.

AJ = [None, None] + list("ABCDEFGHIJ")                    # ids 2 .. 11
LENGTHS = (0, 1, 62, 63, 64, 65, 100, 127, 128, 200)
PAIRS = sorted(set(
    [(a, b) for a in (62, 63, 64, 65) for b in (62, 63, 64, 65)] +           # every pair around the 63 / 64 threshold
    [(0, 0), (0, 1), (1, 0), (1, 1), (0, 64), (64, 0), (0, 200), (200, 0), (1, 64), (64, 1), (1, 200), (127, 1),
     (62, 100), (100, 62), (63, 200), (200, 63), (65, 128), (128, 62), (100, 100), (100, 127), (127, 128), (128, 127),
     (128, 128), (100, 200), (200, 100), (200, 200), (65, 200), (64, 127)]))


def _edited(rng, src, length, lo=2, hi=12):
    """a sequence of `length` ids derived from `src` by deletions or insertions and 10 % substitutions"""
    seq = list(src)
    while len(seq) > length:
        del seq[rng.randint(len(seq))]
    while len(seq) < length:
        seq.insert(rng.randint(len(seq) + 1), int(rng.randint(lo, hi)))
    return [int(rng.randint(lo, hi)) if rng.rand() < 0.1 else s for s in seq]


def _scatter(rng, seq, width):
    """`seq` in order at random positions of a row of `width` ids, blanks (0) and unknowns (1) everywhere else"""
    row = rng.randint(0, 2, size=width).astype(np.int32)
    if len(seq):
        row[np.sort(rng.choice(width, size=len(seq), replace=False))] = seq
    return row


def _rows(pairs, S, S2, seed):
    rng = np.random.RandomState(seed)
    lab = np.zeros((len(pairs), S), np.int32)
    pred = np.zeros((len(pairs), S2), np.int32)
    for r, (la, lb) in enumerate(pairs):
        a = [int(v) for v in rng.randint(2, 12, size=la)]
        lab[r], pred[r] = _scatter(rng, a, S), _scatter(rng, _edited(rng, a, lb), S2)
    return lab, pred


def _check_measure(lab, pred, charset=AJ, fold=None):
    """every output of sequence_measure against oracle.decode; returns the distances"""
    from oracle.decode import label_to_string, levenshtein
    acc, eds = measure(lab, pred, charset=charset)
    strings = [(label_to_string(a, charset).upper(), label_to_string(b, charset).upper()) for a, b in zip(lab, pred)]
    dist = [levenshtein(a, b) for a, b in strings]
    m = sequence_measure(torch.from_numpy(lab).to(DEV), torch.from_numpy(pred).to(DEV), fold=fold)
    got = m['distance'].cpu().tolist()
    bad = [(r, len(a), len(b), d, g) for r, ((a, b), d, g) in enumerate(zip(strings, dist, got)) if d != g]
    print("sequence_measure: %d rows, %d with a side above 63 symbols, wrong distances (row, la, lb, want, got): %s"
          % (len(dist), sum(max(len(a), len(b)) > 63 for a, b in strings), bad))
    assert m['distance'].dtype == torch.int32 and m['label_length'].dtype == torch.int32
    assert got == dist and min(got) >= 0
    assert m['label_length'].cpu().tolist() == [len(a) for a, _ in strings]
    assert m['accuracy'].dtype == torch.bool and m['accuracy'].cpu().tolist() == acc
    assert m['edit_distance'].dtype == torch.float64 and m['edit_distance'].cpu().tolist() == eds   # IEEE-identical doubles
    return dist


@pytest.mark.parametrize("S,S2", [(256, 256), (70, 201)])
def test_measure_long_rows_vs_oracle(S, S2):
    """lengths drawn from LENGTHS on both sides of the 63 / 64 threshold, the symbols scattered among blanks and unknowns so that
    the compaction crosses 64-lane chunks; S != S2 in the second case (the label side then holds at most 70 symbols)"""
    pairs = [(a, b) for a, b in PAIRS if a <= S and b <= S2]
    assert all(a in LENGTHS and b in LENGTHS for a, b in pairs) and len(pairs) >= 30
    assert (63, 64) in pairs and (64, 63) in pairs and (64, 64) in pairs and (63, 63) in pairs
    lab, pred = _rows(pairs, S, S2, seed=S)
    dist = _check_measure(lab, pred)
    assert len(set(dist)) > 10                       # the rows are not all of one kind


def test_measure_long_rows_targeted():
    rng = np.random.RandomState(5)
    S = 256
    a64 = [int(v) for v in rng.randint(2, 12, size=64)]
    a100 = [int(v) for v in rng.randint(2, 12, size=100)]
    a70 = [int(v) for v in rng.randint(2, 11, size=70)]
    differs_last = a70[:69] + [11]                                   # the finding: equal for 69 symbols, the last one differs
    differs_64th = a64[:63] + [a64[63] % 10 + 2 if a64[63] % 10 + 2 != a64[63] else 11]
    assert differs_64th[:63] == a64[:63] and differs_64th[63] != a64[63] and 2 <= differs_64th[63] < 12
    cases = [
        (a64, a64, True, 0), (a100, a100, True, 0),                  # equal sequences of 64 and of 100 symbols
        (a64, differs_64th, False, 1),                               # equal for 63 symbols, then one differing symbol
        (a70, differs_last, False, 1),
        (a100, a100[:64], False, 36), (a100[:63], a100, False, 37),  # one side a strict prefix of the other
        (a64, a64[:63], False, 1), (a64[:63], a64, False, 1),
        ([], [], True, 0),                                           # both empty
        (a100, [], False, 100), ([], a100, False, 100),              # all-unknown / all-blank prediction, empty label
        (a64[:63], a64[:63], True, 0),                               # the last row of the short path
        ([2] * 200, [3] * 130, False, 200), ([2] * 64, [2] * 65, False, 1),
    ]
    lab = np.stack([_scatter(rng, a, S) for a, _, _, _ in cases])
    pred = np.stack([_scatter(rng, b, S) for _, b, _, _ in cases])
    pred[9] = 1                                                      # all unknown
    pred[8] = 1
    lab[8] = 0
    dist = _check_measure(lab, pred)
    m = sequence_measure(torch.from_numpy(lab).to(DEV), torch.from_numpy(pred).to(DEV))
    assert m['accuracy'].cpu().tolist() == [c[2] for c in cases]
    assert dist == [c[3] for c in cases]
    assert float(m['edit_distance'][3]) == 1 - 1 / 70 and float(m['edit_distance'][2]) == 1 - 1 / 64


def test_measure_long_rows_with_fold_table():
    """the fold table of test_measure_random_vs_oracle (ids 2..6 and 7..11 are one letter in two cases) on long rows"""
    fold = torch.arange(12, dtype=torch.int32)
    fold[7:12] = torch.arange(2, 7, dtype=torch.int32)
    cs = [None, None] + list("ABCDE") + list("abcde")
    pairs = [(64, 64), (63, 64), (64, 63), (100, 100), (65, 128), (200, 127), (62, 62), (0, 70), (70, 0)]
    lab, pred = _rows(pairs, 256, 256, seed=11)
    rng = np.random.RandomState(12)
    a = rng.randint(2, 12, size=100)
    lab = np.concatenate([lab, _scatter(rng, a, 256)[None], _scatter(rng, a, 256)[None]])
    other_case = np.where(a < 7, a + 5, a - 5)
    pred = np.concatenate([pred, _scatter(rng, other_case, 256)[None], _scatter(rng, a, 256)[None]])
    dist = _check_measure(lab, pred, charset=cs, fold=fold)
    assert dist[-2:] == [0, 0]                                       # equal up to case: accuracy True through the fold
    # without the table the two cases of a letter are different symbols
    assert _check_measure(lab[-2:], pred[-2:])[1] == 0
    m = sequence_measure(torch.from_numpy(lab[-2:]).to(DEV), torch.from_numpy(pred[-2:]).to(DEV))
    assert m['accuracy'].cpu().tolist() == [False, True]


def test_measure_one_column_and_no_rows():
    lab = np.array([[0], [1], [5], [5], [0], [7]], np.int32)
    pred = np.array([[0], [5], [5], [6], [6], [1]], np.int32)
    assert _check_measure(lab, pred) == [0, 1, 0, 1, 1, 1]
    m = sequence_measure(torch.zeros((0, 40), dtype=torch.int32, device=DEV), torch.zeros((0, 90), dtype=torch.int32, device=DEV))
    assert [tuple(m[k].shape) for k in ('accuracy', 'edit_distance', 'distance', 'label_length')] == [(0,)] * 4


def test_measure_at_and_past_the_length_cap():
    """1024 symbols a side against the Python oracle; the largest row the library takes (MR_SEQ_MEASURE_MAX ids a side, all of them
    symbols) on rows whose distance is known without the quadratic oracle; one id more is refused with the library's message"""
    from megreader_amd import _lib
    cap = _lib._DEFINES["MR_SEQ_MEASURE_MAX"]
    assert cap >= 1024
    lab, pred = _rows([(1024, 1024)], 1024, 1024, seed=21)
    _check_measure(lab, pred)
    rng = np.random.RandomState(22)
    a = rng.randint(2, 12, size=cap).astype(np.int32)
    lab = np.stack([a, a, a, np.full(cap, 2, np.int32), a])
    pred = np.stack([a, np.concatenate([a[:-1], [0]]), np.concatenate([[1], a[1:]]), np.full(cap, 3, np.int32),
                     np.concatenate([a[:-1], [a[-1] % 10 + 2 if a[-1] % 10 + 2 != a[-1] else 11]])]).astype(np.int32)
    m = sequence_measure(torch.from_numpy(lab).to(DEV), torch.from_numpy(pred).to(DEV))
    # equal; a strict prefix (>= the length difference, <= one deletion); the first symbol unknown; no common symbol (no match can
    # lower max(la, lb)); the last symbol substituted (not equal, one substitution)
    assert m['distance'].cpu().tolist() == [0, 1, 1, cap, 1]
    assert m['accuracy'].cpu().tolist() == [True, False, False, False, False]
    assert m['label_length'].cpu().tolist() == [cap] * 5
    assert m['edit_distance'].cpu().tolist() == [1.0, float(1 - 1 * 1.0 / cap), float(1 - 1 * 1.0 / cap), 0.0, float(1 - 1 * 1.0 / cap)]
    for S, S2 in ((cap + 1, 8), (8, cap + 1)):
        with pytest.raises(RuntimeError, match=r"mr_seq_measure: S=%d S2=%d exceed MR_SEQ_MEASURE_MAX=%d" % (S, S2, cap)):
            sequence_measure(torch.zeros((2, S), dtype=torch.int32, device=DEV), torch.zeros((2, S2), dtype=torch.int32, device=DEV))


def _one_hot(idx, C, dtype=torch.float32):
    """scores [N, C, 1, T] whose arg-max over C is idx [N, T]"""
    idx = torch.as_tensor(idx, dtype=torch.int64)
    return torch.nn.functional.one_hot(idx, C).permute(0, 2, 1).unsqueeze(2).to(dtype).contiguous()


def test_representer_and_measurer_on_long_sequences():
    """CTCRepresenter + SequenceRecognitionMeasurer end to end at T = 200: labels of up to 80 characters, predictions that emit 64
    symbols and more; the measurer's lists equal oracle.measure on the decoded ids"""
    from megreader_amd.charsets import EnglishCharset
    cs = EnglishCharset()
    rng = np.random.RandomState(31)
    T, N = 200, 8
    lens = [80, 80, 70, 64, 65, 63, 80, 5]
    texts = []
    for n in lens:
        ids = [int(rng.randint(2, 38))]
        while len(ids) < n:
            c = int(rng.randint(2, 38))
            if c != ids[-1]:
                ids.append(c)
        texts.append("".join(cs[i] for i in ids))
    labels = torch.from_numpy(np.stack([cs.string_to_label(t, max_size=80) for t in texts]))
    steps = np.zeros((N, T), np.int64)
    for r, t in enumerate(texts):
        ids = [cs.index(ch) for ch in t]
        if r == 1:
            ids[-1] = next(c for c in range(2, 38) if c not in ids[-2:])      # the 80th symbol wrong
        if r == 2:
            ids = _edited(rng, ids, 90, 2, 38)
        if r == 6:
            ids = ids[:64]
        seq = []
        for i in ids:                                    # symbol, then a blank or an unknown or nothing
            seq += [i] + [[0], [1], []][int(rng.randint(3))]
        steps[r, :len(seq)] = seq[:T]
    pred = _one_hot(steps, len(cs)).to(DEV)
    want_ids = greedy_decode(pred.cpu().numpy())
    out = CTCRepresenter(cs).represent({'label': labels}, pred)
    got_ids = torch.stack([o['pred_ids'] for o in out]).cpu().numpy()
    assert np.array_equal(got_ids, want_ids)
    emitted = (want_ids != 0).sum(axis=1).tolist()
    assert max(emitted) >= 80 and sum(e >= 64 for e in emitted) >= 5
    assert [o['label_string'] for o in out] == texts
    acc, eds = measure(labels.numpy(), want_ids)
    m = SequenceRecognitionMeasurer(cs).measure({'label': labels}, out)
    assert m['accuracy'] == acc and m['edit_distance'] == eds
    assert acc[0] is True and acc[1] is False and eds[1] == 1 - 1 / 80 and acc[3] and acc[4] and acc[5] and not acc[6]


# --------------------------------------------------------------------------------------------------------- decoders
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decode_1d_wide_alphabet_two_chunks(dtype):
    """C = 5360, T = 65 (a second chunk of one step): scores on a coarse grid that bf16 holds exactly, winners spread over the
    whole alphabet, exact ties above and below the winner (the lower index wins), repeats, blanks, unknowns"""
    g = torch.Generator().manual_seed(61)
    N, C, T = 3, 5360, 65
    p = (torch.rand(N, C, 1, T, generator=g) * 8).round() / 16           # <= 0.5, many ties below the winner's score
    win = torch.randint(0, C, (N, T), generator=g)
    win[0, :8] = torch.tensor([C - 1, C - 1, 0, C - 1, 1, C - 1, 2, 2])
    win[1, 60:65] = torch.tensor([4000, 4000, 1, 4000, 4000])            # a repeat across an unknown and the chunk boundary
    win[2, 62:65] = torch.tensor([77, 0, 77])                            # a blank between repeats at the boundary
    p.scatter_(1, win.view(N, 1, 1, T), 1.0)
    tie = torch.randint(0, C, (N, T), generator=g)                       # a second class with exactly the winner's score
    tie[:, ::3] = win[:, ::3]
    tie[0, :8], tie[1, 60:65], tie[2, 62:65] = win[0, :8], win[1, 60:65], win[2, 62:65]
    p.scatter_(1, tie.view(N, 1, 1, T), 1.0)
    p = p.to(dtype)
    want = greedy_decode(p.double().numpy())
    assert np.array_equal(p.double().numpy().argmax(axis=1)[:, 0, :], torch.minimum(win, tie).numpy())
    ids, ln = ctc_greedy_decode(p.to(DEV))
    assert np.array_equal(ids.cpu().numpy(), want)
    assert ln.cpu().tolist() == [int((r != 0).sum()) for r in want]


@pytest.mark.parametrize("N,C,T", [(5, 7, 130), (2, 38, 64)])
def test_decode_1d_other_blank_and_unknown(N, C, T):
    g = torch.Generator().manual_seed(N + T)
    p = torch.rand(N, C, 1, T, generator=g)
    p[:, :3] *= 1.6
    p = (p * 8).round() / 8
    want = greedy_decode(p.numpy(), blank=2, unknown=0)
    ids, ln = ctc_greedy_decode(p.to(DEV), blank=2, unknown=0)
    assert np.array_equal(ids.cpu().numpy(), want)
    assert ln.cpu().tolist() == [int((r != 2).sum()) for r in want]
    assert not np.array_equal(want, greedy_decode(p.numpy()))            # the two arguments matter on these inputs


def test_decode_empty_batch():
    ids, ln = ctc_greedy_decode(torch.zeros((0, 38, 1, 33), device=DEV))
    assert tuple(ids.shape) == (0, 33) and tuple(ln.shape) == (0,) and ids.dtype == ln.dtype == torch.int32
    ids, ln = ctc2d_greedy_decode(torch.zeros((0, 38, 4, 16), device=DEV), torch.zeros((0, 1, 4, 16), device=DEV))
    assert tuple(ids.shape) == (0, 16) and tuple(ln.shape) == (0,)


def _carry_cases(T):
    """arg-max rows [T] and the symbols they must decode to (blank 0, unknown 1): `previous` carried over 64-step chunks"""
    cases = []

    def case(assign, expect):
        row = np.zeros(T, np.int64)
        for sl, v in assign:
            row[sl] = v
        cases.append((row, expect))
    case([(63, 5), (slice(64, 128), 1), (128, 5)], [5])                  # unknowns do not reset `previous`, over a whole chunk
    case([(63, 5), (slice(64, 128), 1), (128, 6)], [5, 6])
    case([(slice(0, 64), 1), (64, 7), (65, 7), (67, 7)], [7, 7])         # an all-unknown first chunk: carry stays blank
    case([], [])                                                         # all blank
    case([(63, 5), (64, 5)], [5])                                        # a repeat straddling the chunk boundary
    case([(63, 5), (64, 0), (65, 5)], [5, 5])
    case([(slice(0, T), 1)], [])                                         # all unknown
    case([(slice(0, 64), 9), (slice(64, 128), 1), (slice(128, T), 9)], [9])
    case([(0, 4), (slice(1, 128), 1), (128, 0), (129, 4)], [4, 4])
    return cases


def test_decode_1d_carry_across_chunks():
    T = 130
    cases = _carry_cases(T)
    idx = np.stack([row for row, _ in cases])
    p = _one_hot(idx, 12)
    want = greedy_decode(p.numpy())
    ids, ln = ctc_greedy_decode(p.to(DEV))
    for r, (_, expect) in enumerate(cases):
        assert want[r].tolist() == expect + [0] * (T - len(expect)), r          # the oracle agrees with the listed expectation
        assert ids[r].cpu().tolist() == expect + [0] * (T - len(expect)), r
    assert ln.cpu().tolist() == [len(e) for _, e in cases]


def test_decode_2d_carry_across_chunks():
    W, H, C = 130, 3, 12
    cases = _carry_cases(W)
    idx = np.stack([row for row, _ in cases])
    N = len(cases)
    cl = torch.zeros(N, C, H, W)
    for r in range(N):
        for w in range(W):
            cl[r, idx[r, w], (w + r) % H, w] = 1.0                         # the winning row moves from column to column
    mk = torch.ones(N, 1, H, W)
    want = greedy_decode_2d(cl.numpy(), mk.numpy())
    ids, ln = ctc2d_greedy_decode(cl.to(DEV), mk.to(DEV))
    for r, (_, expect) in enumerate(cases):
        assert want[r].tolist() == expect + [0] * (W - len(expect)), r
        assert ids[r].cpu().tolist() == expect + [0] * (W - len(expect)), r
    assert ln.cpu().tolist() == [len(e) for _, e in cases]


def test_decode_2d_signed_scores_and_masks():
    """classify and mask of both signs on a coarse grid (exact products): columns whose row maxima are all negative, exact ties
    between rows (the first row wins) and between classes, zero masks"""
    g = torch.Generator().manual_seed(71)
    N, C, H, W = 3, 7, 4, 70
    cl = torch.randint(-8, 9, (N, C, H, W), generator=g).float() / 8
    mk = torch.randint(-4, 5, (N, 1, H, W), generator=g).float() / 4
    cl[:, :, :, 5] = -(torch.randint(1, 9, (N, C, H), generator=g).float() / 8)    # column 5: every product negative
    mk[:, :, :, 5] = torch.randint(1, 5, (N, 1, H), generator=g).float() / 4
    cl[:, :, :, 66] = cl[:, :, :, 5]                                               # and in the second chunk
    mk[:, :, :, 66] = mk[:, :, :, 5]
    cl[:, 3, 2, 9] = 0.75
    cl[:, :, 0, 9] = cl[:, :, 2, 9]                                                # column 9: rows 0 and 2 tie exactly
    mk[:, :, 0, 9] = mk[:, :, 2, 9] = 1.0
    cl[:, :, 1, 9] = -1.0
    cl[:, :, 3, 9] = -1.0
    mk[:, :, 1, 9] = mk[:, :, 3, 9] = 0.5
    cl[:, :, 1, 64] = cl[:, :, 3, 64] = 0.5                                        # column 64: a tie between rows 1 and 3, all classes
    mk[:, :, 1, 64] = mk[:, :, 3, 64] = 1.0
    mk[:, :, 0, 64] = mk[:, :, 2, 64] = 0.0
    heat = (cl * mk).numpy()
    assert (heat[:, :, :, 5] < 0).all() and (heat[:, :, :, 66] < 0).all()
    assert np.array_equal(heat[:, :, 0, 9], heat[:, :, 2, 9]) and (heat[:, :, 0, 9].max(axis=1) > -0.5).all()
    want = greedy_decode_2d(cl.numpy(), mk.numpy())
    ids, ln = ctc2d_greedy_decode(cl.to(DEV), mk.to(DEV))
    assert np.array_equal(ids.cpu().numpy(), want)
    assert ln.cpu().tolist() == [int((r != 0).sum()) for r in want]
    assert len(set(want.reshape(-1).tolist())) >= 5


def test_posterior_layouts_and_dtypes_read_alike_by_the_four_wrappers():
    """One posterior (N=3, C=5, T=7) through ctc_greedy_decode, ctc_beam_search_decode, ctc_forced_align and Lexicon.transcribe as
    [N, C, T], [N, C, 1, T], a transposed view (st != 1) and f64 / f16 copies: the same bits out every time.  Every value is a
    multiple of 1/64, exact in f16, so a copy holds the same numbers and a column's greatest value stays 22/64 clear of the next."""
    from megreader_amd.charsets import Charset
    from megreader_amd.ops.decode import ctc_beam_search_decode, ctc_forced_align
    from megreader_amd.ops.lexicon import Lexicon
    N, C, T = 3, 5, 7
    rng = np.random.RandomState(11)
    y = np.stack([np.stack([rng.permutation([34, 12, 9, 6, 3]) for _ in range(T)], axis=1) for _ in range(N)]).astype(np.float32) / 64
    pred = torch.from_numpy(y)                                                   # [N, C, T]
    assert pred.shape == (N, C, T) and torch.equal(pred.sum(dim=1), torch.ones(N, T))
    assert torch.equal(pred.half().float(), pred) and torch.equal(pred.double().float(), pred)
    top2 = pred.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) == 22 / 64
    pred = pred.to(DEV)
    transposed = pred.permute(0, 2, 1).contiguous().permute(0, 2, 1)             # [N, C, T] over an [N, T, C] base
    assert transposed.stride() == (T * C, 1, C) and not transposed.is_contiguous()
    forms = {'[N, C, T]': pred, '[N, C, 1, T]': pred.unsqueeze(2), 'transposed': transposed, 'f64': pred.double(),
             'f16': pred.half()}
    lexicon = Lexicon(["AB", "CAB", "B", "ACCA"], Charset("ABC"))
    assert len(lexicon.charset) == C
    targets = torch.tensor([[2, 3, 0], [4, 2, 3], [3, 0, 0]], dtype=torch.int32, device=DEV)
    lengths = torch.tensor([2, 3, 1], dtype=torch.int32, device=DEV)
    wrappers = {
        'greedy': lambda p: dict(zip(('ids', 'lengths'), ctc_greedy_decode(p))),
        'beam': lambda p: ctc_beam_search_decode(p, beam=4, nbest=2, top_classes=3),
        'align': lambda p: ctc_forced_align(p, targets, lengths),
        'transcribe': lambda p: lexicon.transcribe(p, all_scores=True),
    }
    errors = {'greedy': RuntimeError, 'beam': RuntimeError, 'align': RuntimeError, 'transcribe': ValueError}
    for name, run in wrappers.items():
        want = run(forms['[N, C, T]'])
        for form, p in forms.items():
            got = run(p)
            assert got.keys() == want.keys()
            for key in want:
                assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), (name, form, key)
        with pytest.raises(errors[name]):
            run(torch.full((N, C, 2, T), 0.2, device=DEV))
    # and they read something: the greedy path is the column maxima, the beam has two strings per row, every row aligns
    ids, _ = ctc_greedy_decode(pred)
    assert ids.shape == (N, T) and int(wrappers['beam'](pred)['count'].min()) == 2
    assert torch.isfinite(wrappers['align'](pred)['score']).all() and int(wrappers['transcribe'](pred)['index'].min()) >= 0
