"""mr_ctc_align (csrc/ctc_align.hip) and `ctc_forced_align` against the numpy restatement (tests/_ctc_align_ref.py).

The recursion is one f32 addition and one comparison per cell on a table of logs that is defined to the bit (the f32 nearest to the
f64 log), so the bar is EQUALITY of all six outputs with the float32 restatement, not a tolerance; `same` compares bit patterns.
The C entry point is called with every output pre-filled with garbage: equality also shows that everything was written.  The last
section holds the kernel's path to float64 truth by the rounding bound of the issue."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ctc_align_ref as R  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import ptr  # noqa: E402
from megreader_amd.ops.decode import ctc_forced_align  # noqa: E402

DEV = "cuda"
KEYS = ('score', 'pos', 'begin', 'end', 'sym_lp', 'peak')
GARBAGE_I, GARBAGE_F = 12345, 777.0


def dirichlet(seed, N, T, C, alpha=1.0):
    """f32 probabilities [N, T, C]."""
    return np.random.RandomState(seed).dirichlet(np.full(C, alpha), size=(N, T)).astype(np.float32)


def eval_layout(y, dtype=torch.float32):
    """y [N, T, C] numpy -> the eval head's [N, C, 1, T] device tensor (a class's T values contiguous)."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(y, (0, 2, 1)))).to(DEV).to(dtype).unsqueeze(2)


def random_targets(seed, N, S, C, lengths, blank=0, unknown=1):
    rng = np.random.RandomState(seed)
    letters = np.array([c for c in range(C) if c not in (blank, unknown)])
    targets = letters[rng.randint(0, len(letters), size=(N, S))].astype(np.int32)
    return targets, np.asarray(lengths, dtype=np.int32)


def raw_call(pred, targets, lengths, blank=0, unknown=1, log_probs=False, expect=0, override=()):
    """The C entry point with every output and the workspace pre-filled with garbage; `override` replaces arguments by name.
    Returns the outputs as numpy."""
    if pred.dim() == 4:
        pred = pred.select(2, 0)
    N, C, T = pred.shape
    targets = np.asarray(targets, dtype=np.int32)
    assert targets.ndim == 2 and targets.shape[0] == N
    S = targets.shape[1]
    tg = torch.from_numpy(np.ascontiguousarray(targets)).to(DEV) if S else None
    ln = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).to(DEV)
    out = {'score': torch.full((N,), GARBAGE_F, dtype=torch.float32, device=DEV),
           'pos': torch.full((N, T), GARBAGE_I, dtype=torch.int32, device=DEV),
           'begin': torch.full((N, S), GARBAGE_I, dtype=torch.int32, device=DEV),
           'end': torch.full((N, S), GARBAGE_I, dtype=torch.int32, device=DEV),
           'sym_lp': torch.full((N, S), GARBAGE_F, dtype=torch.float32, device=DEV),
           'peak': torch.full((N, S), GARBAGE_I, dtype=torch.int32, device=DEV)}
    nbytes = _lib.load().mr_ctc_align_ws_bytes(max(N, 1), max(1, min(T, 4096)), max(0, min(S, 256)))
    ws = torch.full((nbytes // 8 + 1,), -0x5454545454545455, dtype=torch.int64, device=DEV)
    sn, sc, st = pred.stride()
    a = dict(dtype={torch.float32: 0, torch.bfloat16: 1}[pred.dtype], pred=ptr(pred), sn=sn, sc=sc, st=st, N=N, C=C, T=T,
             log_probs=int(log_probs), blank=blank, unknown=unknown, targets=ptr(tg), S=S, target_len=ptr(ln),
             score=ptr(out['score']), pos=ptr(out['pos']), begin=ptr(out['begin']), end=ptr(out['end']),
             sym_lp=ptr(out['sym_lp']), peak=ptr(out['peak']), ws=ptr(ws), ws_bytes=ws.numel() * 8)
    a.update(dict(override))
    rc = _lib.load().mr_ctc_align(*[a[k] for k in ("dtype", "pred", "sn", "sc", "st", "N", "C", "T", "log_probs", "blank",
                                                   "unknown", "targets", "S", "target_len", "score", "pos", "begin", "end",
                                                   "sym_lp", "peak", "ws", "ws_bytes")], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.load().mr_last_error().decode())
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, name=""):
    """All six outputs equal bit for bit."""
    for key in KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, (name, key, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert len(bad) == 0, "%s %s: %d cells differ, first at %s: kernel %r, restatement %r" % (
            name, key, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def check(y, targets, lengths, blank=0, unknown=1, name="", alive=None):
    """Kernel (probabilities in the eval layout) == float32 restatement; `alive`: what the rows must be."""
    ref = R.align(R.log_table(y), targets, lengths, blank, unknown, np.float32)
    got = raw_call(eval_layout(y), targets, lengths, blank, unknown)
    same(got, ref, name)
    assert not np.isnan(got['score']).any() and not np.isnan(got['sym_lp']).any()
    if alive is not None:
        assert ref['alive'].tolist() == list(alive), (name, ref['alive'])
    return got, ref


# ---- small shapes and the rules of the target

def test_one_column():
    y = dirichlet(1, 2, 1, 5)
    got, _ = check(y, [[2, 3], [2, 3]], [0, 1], alive=[True, True])
    assert got['pos'].tolist() == [[0], [1]] and got['begin'][1].tolist() == [0, -1] and got['end'][1].tolist() == [1, -1]
    check(y, [[2, 3], [2, 3]], [2, 2], alive=[False, False])                   # two symbols, one column


def test_empty_string():
    y = dirichlet(2, 3, 5, 6)
    got, _ = check(y, np.zeros((3, 4), dtype=np.int32), [0, 0, 0], alive=[True] * 3)
    assert np.all(got['pos'] == 0) and np.all(got['begin'] == -1) and np.all(got['sym_lp'] == -np.inf)
    lp = R.log_table(y)
    assert np.allclose(got['score'], lp[:, :, 0].astype(np.float64).sum(axis=1), rtol=1e-6)
    got = raw_call(eval_layout(y), np.zeros((3, 0), dtype=np.int32), [0, 0, 0])            # S == 0: targets is not read
    assert np.all(got['pos'] == 0) and got['begin'].shape == (3, 0)


def test_as_many_symbols_as_columns():
    y = dirichlet(3, 2, 5, 6)
    got, _ = check(y, [[2, 3, 4, 2, 3], [5, 4, 5, 4, 5]], [5, 5], alive=[True, True])
    assert got['pos'].tolist() == [[1, 3, 5, 7, 9]] * 2


def test_repeats_need_their_blank():
    aab = [[2, 2, 3]]
    got, _ = check(dirichlet(4, 1, 4, 5), aab, [3], alive=[True])              # the exact fit: A - A B
    assert got['pos'].tolist() == [[1, 2, 3, 5]]
    check(dirichlet(4, 1, 3, 5), aab, [3], alive=[False])                      # one column short
    check(dirichlet(5, 1, 8, 5), [[2, 2, 2, 2, 3]], [5], alive=[True])         # 5 symbols and 3 blanks between the 2s
    check(dirichlet(5, 1, 7, 5), [[2, 2, 2, 2, 3]], [5], alive=[False])


def test_exact_zeros():
    y = dirichlet(6, 3, 5, 4)
    y[:, :, 3] = 0.0                                                           # class 3 is impossible everywhere
    y[0, 0, 0] = 0.0                                                           # row 0 must start on its symbol
    y[1, 2, :] = [0.0, 0.0, 1.0, 0.0]                                          # row 1: column 2 is class 2 for certain
    got, ref = check(y, [[2, 2], [2, 2], [3, 2]], [1, 1, 1], alive=[True, True, False])
    assert got['pos'][0, 0] == 1 and got['pos'][1, 2] == 1 and np.all(got['pos'][2] == -1)
    assert np.isfinite(got['score'][:2]).all() and got['score'][2] == -np.inf
    # reachable by shape, but every alignment crosses a zero
    y = dirichlet(7, 1, 4, 4)
    y[0, :, 2] = 0.0
    check(y, [[2, 3]], [2], alive=[False])


def test_uniform_posterior_is_decided_by_the_tie_rule():
    y = np.full((3, 6, 3), 1.0 / 3.0, dtype=np.float32)
    got, _ = check(y, [[1, 2], [1, 1], [2, 0]], [2, 2, 1], unknown=-1, alive=[True] * 3)
    assert got['pos'].tolist() == [[1, 3, 4, 4, 4, 4], [1, 2, 3, 4, 4, 4], [1, 2, 2, 2, 2, 2]]
    assert got['peak'].tolist() == [[0, 1], [0, 2], [0, -1]]


def test_two_classes():
    y = dirichlet(8, 2, 7, 2)
    check(y, [[1, 1, 1], [1, 1, 1]], [1, 3], blank=0, unknown=-1, alive=[True, True])
    check(y, [[0, 0, 0, 0], [0, 0, 0, 0]], [2, 4], blank=1, unknown=7, alive=[True, True])
    check(y, [[1, 1, 1], [1, 1, 1]], [1, 3], blank=0, unknown=1, alive=[False, False])     # the one symbol is `unknown`


def test_unalignable_targets():
    y = dirichlet(9, 8, 6, 5)
    targets = [[2, 0, 3], [2, 1, 3], [2, 5, 3], [2, -1, 3], [2, 3, 4], [2, 3, 4], [2, 3, 4], [0, 1, 9]]
    lengths = [3, 3, 3, 3, -1, 4, 3, 0]
    #          blank unknown >= C  < 0  -1  S+1  fine  K = 0: the bad ids lie past it
    got, _ = check(y, targets, lengths, alive=[False] * 6 + [True, True])
    assert np.all(got['pos'][:6] == -1) and np.all(got['score'][:6] == -np.inf) and np.all(got['peak'][:6] == -1)


# ---- long strings, long rows, wide alphabets

@pytest.mark.parametrize("alpha", [1.0, 0.2])
def test_both_sides_of_the_register_slots(alpha):
    """K = 63 fits one symbol per lane, 64 and 65 take a second slot (and 127 / 128 a third to fifth); one batch, S = 130."""
    lengths = [63, 64, 65, 127, 128, 130, 1, 0]
    N, T, C = len(lengths), 140, 12
    y = dirichlet(10, N, T, C, alpha)
    targets, lengths = random_targets(11, N, 130, C, lengths)
    for n in (3, 4, 5):                                                        # no repeats there: they have to fit 140 columns
        targets[n] = 2 + (np.arange(130) % 3)
    got, ref = check(y, targets, lengths, name="alpha %g" % alpha)
    assert ref['alive'].tolist() == [True, True, True, True, True, True, True, True]


def test_longest_string():
    N, T, C, K = 2, 600, 12, 256
    y = dirichlet(12, N, T, C, 0.5)
    targets, lengths = random_targets(13, N, K, C, [K, K - 1])
    check(y, targets, lengths, alive=[True, True])
    # 64..127 symbols and too many columns for the back-pointers to stay in LDS
    y = dirichlet(31, 2, 300, C, 0.5)
    targets, lengths = random_targets(32, 2, 100, C, [100, 64])
    check(y, targets, lengths, alive=[True, True])


def test_longest_row():
    N, T, C = 2, 4096, 6
    y = dirichlet(14, N, T, C)
    got, _ = check(y, [[2, 3, 2], [4, 4, 5]], [3, 3], alive=[True, True])
    assert (got['end'] - got['begin']).min() >= 1


def test_wide_alphabet():
    N, T, C = 3, 9, 6000
    y = dirichlet(15, N, T, C)
    targets = [[5999, 17, 3000, 64], [2, 2, 5998, 4097], [6000, 2, 2, 2]]
    check(y, targets, [4, 4, 4], alive=[True, True, False])


# ---- layouts, dtypes, logs

def test_layouts():
    N, T, C = 5, 11, 7
    y = dirichlet(16, N, T, C)
    targets, lengths = random_targets(17, N, 6, C, [0, 1, 3, 5, 6])
    want = R.align(R.log_table(y), targets, lengths, 0, 1, np.float32)
    same(raw_call(eval_layout(y), targets, lengths), want, "[N, C, 1, T]")
    tnc = torch.from_numpy(np.ascontiguousarray(np.transpose(y, (1, 0, 2)))).to(DEV)         # [T, N, C]: the CRNN's own order
    same(raw_call(tnc.permute(1, 2, 0), targets, lengths), want, "[T, N, C] viewed as [N, C, T]")
    big = torch.rand((2 * N, C + 3, 2 * T), device=DEV)
    view = big[1::2, 2:2 + C, ::2]
    view.copy_(eval_layout(y).select(2, 0))
    same(raw_call(view, targets, lengths), want, "a slice of a larger tensor")
    wrapped = ctc_forced_align(view.unsqueeze(2), torch.from_numpy(targets).to(DEV), torch.from_numpy(lengths).to(DEV))
    same({k: wrapped[k].cpu().numpy() for k in KEYS}, want, "ctc_forced_align")
    f64 = ctc_forced_align(eval_layout(y).double(), torch.from_numpy(targets).to(DEV), torch.from_numpy(lengths).to(DEV))
    same({k: f64[k].cpu().numpy() for k in KEYS}, want, "float64 input goes through float32")


def test_bfloat16_input():
    N, T, C = 4, 13, 9
    pred = eval_layout(dirichlet(18, N, T, C), torch.bfloat16)
    values = pred.float().select(2, 0).permute(0, 2, 1).cpu().numpy()                       # the same bf16 values, [N, T, C]
    targets, lengths = random_targets(19, N, 5, C, [5, 4, 2, 0])
    same(raw_call(pred, targets, lengths), R.align(R.log_table(values), targets, lengths, 0, 1, np.float32), "bf16")


def test_log_probs():
    N, T, C = 4, 13, 9
    y = dirichlet(20, N, T, C)
    y[0, 3, :] = [0, 0, 1, 0, 0, 0, 0, 0, 0]                                   # zeros: -inf logs
    targets, lengths = random_targets(21, N, 5, C, [5, 4, 2, 0])
    targets[0, :5] = [2, 3, 2, 4, 5]
    on_probs = raw_call(eval_layout(y), targets, lengths)
    on_logs = raw_call(eval_layout(R.log_table(y)), targets, lengths, log_probs=True)
    same(on_logs, on_probs, "log_probs")
    same(on_probs, R.align(R.log_table(y), targets, lengths, 0, 1, np.float32))


# ---- the call

def test_no_rows():
    got = raw_call(torch.empty((0, 5, 7), device=DEV), np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert got['pos'].shape == (0, 7)
    out = ctc_forced_align(torch.empty((0, 5, 1, 7), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV),
                           torch.zeros((0,), dtype=torch.int32, device=DEV))
    assert out['pos'].shape == (0, 7) and out['begin'].shape == (0, 3) and out['score'].shape == (0,)


def test_a_row_does_not_depend_on_its_batch():
    N, T, C = 3, 40, 10
    y = dirichlet(22, N, T, C)
    targets, lengths = random_targets(23, N, 12, C, [12, 7, 3])
    batch = raw_call(eval_layout(y), targets, lengths)
    for n in range(N):
        alone = raw_call(eval_layout(y[n:n + 1]), targets[n:n + 1], lengths[n:n + 1])
        order = [2, 0, 1, 0]
        moved = raw_call(eval_layout(y[order]), targets[order], lengths[order])
        wide = raw_call(eval_layout(y[n:n + 1]), np.pad(targets[n:n + 1], ((0, 0), (0, 100)), constant_values=1),
                        lengths[n:n + 1])                                      # another S: more slots, the same row
        for key in KEYS:
            assert np.array_equal(alone[key][0].view(np.int32), batch[key][n].view(np.int32)), (n, key)
            for at, src in enumerate(order):
                if src == n:
                    assert np.array_equal(moved[key][at].view(np.int32), batch[key][n].view(np.int32)), (n, key, at)
            width = batch[key].shape[1] if batch[key].ndim == 2 else 1
            assert np.array_equal(np.atleast_1d(wide[key][0])[:width].view(np.int32),
                                  np.atleast_1d(batch[key][n]).view(np.int32)), (n, key)


def test_capturable_in_a_graph():
    N, T, C = 6, 16, 37
    y = dirichlet(24, N, T, C, 0.3)
    pred, other = eval_layout(y), eval_layout(y[::-1].copy())
    targets, lengths = random_targets(25, N, 8, C, [8, 6, 4, 2, 1, 0])
    tg, ln = torch.from_numpy(targets).to(DEV), torch.from_numpy(lengths).to(DEV)
    eager = {k: v.clone() for k, v in ctc_forced_align(pred, tg, ln).items()}
    eager_other = {k: v.clone() for k, v in ctc_forced_align(other, tg, ln).items()}
    static = pred.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        found = ctc_forced_align(static, tg, ln)
    for source, want in ((other, eager_other), (pred, eager)):                 # new contents of the same tensor
        static.copy_(source)
        graph.replay()
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(found[key].view(torch.int32), want[key].view(torch.int32)), key
    assert not torch.equal(eager['pos'], eager_other['pos'])


def untouched(got):
    return all(np.all(got[k] == (GARBAGE_F if got[k].dtype == np.float32 else GARBAGE_I)) for k in KEYS)


def test_argument_errors_write_nothing():
    y = dirichlet(26, 2, 6, 5)
    pred = eval_layout(y)
    targets, lengths = random_targets(27, 2, 3, 5, [3, 2])
    arg, dtype_err = 1, 2
    lib = _lib.load()
    for override in (dict(S=257), dict(S=-1), dict(T=0), dict(T=4097), dict(C=1), dict(blank=5), dict(blank=-1), dict(N=-1),
                     dict(ws=0), dict(ws_bytes=8), dict(ws_bytes=lib.mr_ctc_align_ws_bytes(2, 6, 3) - 1)):
        assert untouched(raw_call(pred, targets, lengths, expect=arg, override=override.items())), override
        assert "mr_ctc_align" in lib.mr_last_error().decode()
    ws = torch.empty(1024, dtype=torch.int64, device=DEV)
    assert untouched(raw_call(pred, targets, lengths, expect=arg, override=dict(ws=ws.data_ptr() + 4, ws_bytes=4096).items()))
    assert untouched(raw_call(pred, targets, lengths, expect=dtype_err, override=dict(dtype=2).items()))
    same(raw_call(pred, targets, lengths), R.align(R.log_table(y), targets, lengths, 0, 1, np.float32))   # and then it works

    tg, ln = torch.from_numpy(targets).to(DEV), torch.from_numpy(lengths).to(DEV)
    for bad in (lambda: ctc_forced_align(pred, tg, ln, blank=5),
                lambda: ctc_forced_align(pred, tg, ln, blank=-1),
                lambda: ctc_forced_align(pred[:, :1], tg, ln),
                lambda: ctc_forced_align(pred, tg[:1], ln),
                lambda: ctc_forced_align(pred, tg, ln[:1]),
                lambda: ctc_forced_align(pred, torch.zeros((2, 257), dtype=torch.int32, device=DEV), ln),
                lambda: ctc_forced_align(torch.ones((2, 5, 4097), device=DEV), tg, ln),
                lambda: ctc_forced_align(pred[..., :0], tg, ln)):
        with pytest.raises(ValueError, match="ctc_forced_align"):
            bad()


# ---- against float64

def test_against_float64_truth():
    """N = 64 random Dirichlet rows, C = 12, T = 20, K <= 8.  bound = T * 2^-24 * sum_t |lp[t, path_t]|: T additions, each rounding
    at most half an ulp (2^-24 relative) of a partial sum that is at most the sum of the magnitudes.  The kernel's path, evaluated
    in float64 over the f32 table, scores within `bound` of the f32 `score`; it lies within 2 * bound of the float64 optimum (the
    f32 optimum beats the f32 value of the f64-best path, and both are within bound of their f64 values); and where the float64
    margin exceeds 4 * bound the path IS the float64 path.  The seed is chosen so that this holds on every row."""
    N, C, T, S = 64, 12, 20, 8
    y = dirichlet(28, N, T, C)
    rng = np.random.RandomState(29)
    lengths = rng.randint(0, S + 1, size=N)
    targets, lengths = random_targets(30, N, S, C, lengths)
    lp = R.log_table(y)
    got = raw_call(eval_layout(y), targets, lengths)
    truth = R.align(lp, targets, lengths, 0, 1, np.float64, margin=True)
    clear = 0
    for n in range(N):
        assert truth['alive'][n] and np.isfinite(got['score'][n])
        path = R.path_of(got['pos'][n], targets[n], 0)
        terms = np.array([lp[n, t, c] for t, c in enumerate(path)], dtype=np.float64)
        bound = T * 2.0 ** -24 * np.abs(terms).sum()
        value = terms[0]
        for v in terms[1:]:
            value = value + v
        print("row %2d K %d: |f64(path) - score| %.3g, f64 optimum - f64(path) %.3g, bound %.3g, margin %.3g"
              % (n, lengths[n], abs(value - float(got['score'][n])), float(truth['score'][n]) - value, bound,
                 truth['margin'][n]))
        assert abs(value - float(got['score'][n])) <= bound, n
        assert 0.0 <= float(truth['score'][n]) - value + 1e-15 and float(truth['score'][n]) - value <= 2 * bound, n
        if truth['margin'][n] > 4 * bound:
            clear += 1
            assert np.array_equal(got['pos'][n], truth['pos'][n]), n
    assert clear == N
