"""mr_ctc_beam_search (csrc/ctc_beam.hip) and `ctc_beam_search_decode` against enumeration of every path and against the numpy
restatement (tests/_ctc_beam_ref.py).

Tolerance: none is fixed.  Each case runs the restatement in float64 and in float32 on the f32 table of logs the kernel is defined
on; e32 is the largest |score32 - score64| over the rows where both return the same strings, and the kernel gets tol = 8 * e32 (its
exp / log differ from numpy's; e32 itself is rounding at the magnitude of the scores).  A row is CLEAR when its float64 margin --
the smallest gap at any decision of the row: the B-th against the (B+1)-th total, the Kc-th symbol against the best one left out,
two consecutive returned scores -- exceeds 2 tol.  On clear rows strings, order, lengths and count equal the float64 restatement
exactly and the scores are within tol.  On every row: scores descend, no NaN, slots past count are exactly (0, -inf, blanks), a
score is at most the float64 log-probability of its string over ALL alignments + tol, and within tol of the restatement's score for
that string whenever the restatement returned it too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ctc_beam_ref as B  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.ops.decode import ctc_beam_search_decode  # noqa: E402

DEV = "cuda"
KEYS = ('ids', 'lengths', 'scores', 'count')


def eval_layout(y, dtype=torch.float32):
    """y [N, T, C] numpy -> the eval head's [N, C, 1, T] device tensor (a class's T values contiguous)."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(y, (0, 2, 1)))).to(DEV).to(dtype).unsqueeze(2)


def host(out, keys=KEYS):
    return {k: out[k].cpu().numpy() for k in keys}


def strings(out, n, scores=('scores',)):
    """[(tuple of ids, score)] of row n as returned; with the model's `scores`, (tuple of ids, score, ctc_score, lm_score)."""
    return [(tuple(int(s) for s in out['ids'][n, k, :out['lengths'][n, k]]),) + tuple(float(out[key][n, k]) for key in scores)
            for k in range(int(out['count'][n]))]


def raw_call(pred, beam, nbest, top, blank=0, unknown=1, log_probs=False, expect=0, override=()):
    """The C entry point with every output and the workspace pre-filled with garbage; `override` replaces arguments by name.
    Returns (return code, outputs as numpy)."""
    if pred.dim() == 4:
        pred = pred.select(2, 0)
    N, C, T = pred.shape
    K = max(1, min(nbest, 64))
    ids = torch.full((N, K, T), 12345, dtype=torch.int32, device=DEV)
    lengths = torch.full((N, K), 12345, dtype=torch.int32, device=DEV)
    scores = torch.full((N, K), 777.0, dtype=torch.float32, device=DEV)
    count = torch.full((N,), 12345, dtype=torch.int32, device=DEV)
    nbytes = _lib.load().mr_ctc_beam_ws_bytes(max(N, 1), T, max(1, min(beam, 64)), max(1, min(top, 64)))
    ws = torch.full((nbytes // 8 + 1,), -0x5454545454545455, dtype=torch.int64, device=DEV)
    sn, sc, st = pred.stride()
    a = dict(dtype={torch.float32: 0, torch.bfloat16: 1}[pred.dtype], pred=ptr(pred), sn=sn, sc=sc, st=st, N=N, C=C, T=T,
             log_probs=int(log_probs), blank=blank, unknown=unknown, beam=beam, nbest=nbest, top=top, ids=ptr(ids),
             lengths=ptr(lengths), scores=ptr(scores), count=ptr(count), ws=ptr(ws), ws_bytes=ws.numel() * 8)
    a.update(dict(override))
    fn = _lib.load().mr_ctc_beam_search
    rc = fn(*[a[k] for k in ("dtype", "pred", "sn", "sc", "st", "N", "C", "T", "log_probs", "blank", "unknown", "beam", "nbest",
                             "top", "ids", "lengths", "scores", "count", "ws", "ws_bytes")], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.load().mr_last_error().decode())
    return rc, host(dict(ids=ids, lengths=lengths, scores=scores, count=count))


class Reference(object):
    """The two restatements of one case, computed once: lp [N, T, C], the f32 table of logs."""

    def __init__(self, lp, beam, nbest, top, blank=0, unknown=1):
        self.lp, self.args, self.blank, self.unknown = lp, (beam, nbest, top), blank, unknown
        self.r64 = B.decode(lp, beam, nbest, top, blank, unknown, np.float64)
        self.r32 = B.decode(lp, beam, nbest, top, blank, unknown, np.float32)
        self.e32 = 0.0
        for a, b in zip(self.r64, self.r32):
            if [p for p, _ in a['hyps']] == [p for p, _ in b['hyps']]:
                self.e32 = max([self.e32] + [abs(float(s32) - float(s64)) for (_, s64), (_, s32) in zip(a['hyps'], b['hyps'])])
        self.tol = 8.0 * self.e32
        self.clear = [r['margin'] > 2 * self.tol for r in self.r64]


def compare(out, ref, name="", need_clear=None, truth=None):
    """Every assertion of the module docstring; `truth`: per row {string: float64 log-probability} from enumeration, which then
    replaces the restatement as what the scores are held to (and must list exactly the strings returned).  Returns worst / e32."""
    lp, (beam, nbest, top), blank = ref.lp, ref.args, ref.blank
    N, T = lp.shape[:2]
    tol, worst = ref.tol, 0.0
    assert out['ids'].shape == (N, nbest, T) and out['scores'].shape == (N, nbest) and out['count'].shape == (N,)
    assert not np.isnan(out['scores']).any()
    for n in range(N):
        got, want = strings(out, n), ref.r64[n]['hyps']
        k = len(got)
        assert 0 <= k <= nbest
        assert np.all(out['lengths'][n, k:] == 0) and np.all(out['scores'][n, k:] == -np.inf), n
        assert np.all(out['ids'][n, k:] == blank), n
        for j in range(k):
            assert np.all(out['ids'][n, j, out['lengths'][n, j]:] == blank), (n, j)
            assert np.isfinite(got[j][1]), (n, j)
        scores = [s for _, s in got]
        assert scores == sorted(scores, reverse=True), (n, scores)
        assert len({p for p, _ in got}) == k, "a string twice in row %d: %r" % (n, got)
        theirs = dict(want)
        for p, s in got:
            assert blank not in p and ref.unknown not in p
            bound = truth[n][p] if truth is not None else B.true_score(lp[n], p, blank, ref.unknown)
            assert s <= bound + tol, (n, p, s, bound, tol)
            if p in theirs:
                err = abs(s - float(theirs[p]))
                worst = max(worst, err)
                assert err <= tol, "row %d %r: |kernel - float64| = %.3g, tol = %.3g (e32 = %.3g)" % (n, p, err, tol, ref.e32)
        if truth is not None:
            assert {p for p, _ in got} == set(truth[n]), n
            for p, s in got:
                err = abs(s - truth[n][p])
                worst = max(worst, err)
                assert err <= tol, "row %d %r: |kernel - enumeration| = %.3g, tol = %.3g" % (n, p, err, tol)
        if ref.clear[n]:
            assert [p for p, _ in got] == [p for p, _ in want], (n, got, want)
            assert k == len(want)
    ratio = worst / ref.e32 if ref.e32 > 0 else 0.0
    print("%s: N=%d T=%d C=%d B=%d K=%d Kc=%d e32=%.3g tol=%.3g worst=%.3g (%.2f e32), %d of %d rows clear"
          % (name, N, T, lp.shape[2], beam, nbest, top, ref.e32, tol, worst, ratio, sum(ref.clear), N))
    if need_clear is not None:
        assert sum(ref.clear) >= need_clear, "only %d of %d rows are clear" % (sum(ref.clear), N)
    return ratio


def run(y, beam, nbest, top, blank=0, unknown=1, name="", need_clear=None, dtype=torch.float32, truth=None):
    """y: f32 [N, T, C] probabilities.  Decode on the device, restate, compare; returns (outputs, reference)."""
    pred = eval_layout(y, dtype)
    seen = pred.float().cpu().numpy()[:, :, 0, :].transpose(0, 2, 1)              # what the kernel reads (bf16: rounded)
    out = host(ctc_beam_search_decode(pred, beam=beam, nbest=nbest, top_classes=top, blank=blank, unknown=unknown))
    ref = Reference(B.logs(seen), beam, nbest, top, blank, unknown)
    compare(out, ref, name, need_clear, truth)
    return out, ref


# ---- exhaustive: against enumeration, no restatement of the algorithm in what the scores are held to

@pytest.mark.parametrize("C,T,unknown", [(3, 5, -1), (3, 6, -1), (4, 3, -1), (4, 4, -1), (5, 3, -1), (4, 4, 1)])
def test_exhaustive_equals_enumeration(C, T, unknown):
    y = B.posterior(np.random.RandomState(C * 16 + T), 32, T, C, sharp=1.5)
    # the paths of the table the kernel is defined on: probabilities exp(lp) of the f32 logs
    truth = [B.enumerate_strings(np.exp(B.logs(row).astype(np.float64)), 0, unknown) for row in y]
    assert max(len(t) for t in truth) <= 64
    out, ref = run(y, 64, 64, 64, unknown=unknown, name="exhaustive C=%d T=%d" % (C, T), truth=truth)
    assert [int(c) for c in out['count']] == [len(t) for t in truth]


# ---- pruned: the table of the issue

PRUNED = {"english-8": (64, 24, 37, 8, 8, 2.0), "english-all": (64, 24, 37, 8, 37, 2.0), "printable": (32, 26, 96, 16, 12, 3.0),
          "wide": (16, 8, 6000, 4, 16, 3.0)}


@pytest.mark.parametrize("kind", sorted(PRUNED))
def test_pruned_against_restatement(kind):
    N, T, C, beam, top, sharp = PRUNED[kind]
    y = B.posterior(np.random.RandomState(len(kind)), N, T, C, sharp)
    run(y, beam, beam, top, name=kind, need_clear=-(-3 * N // 4))


def test_pruned_wide_bf16():
    N, T, C, beam, top, sharp = PRUNED["wide"]
    # bf16 keeps 8 bits of a probability: bit-equal neighbours at the Kc-th place are common and make a row's margin 0.  The seed
    # is one whose batch has 14 of 16 rows clear (of the seeds 30..35 most have 11 or 12)
    y = B.posterior(np.random.RandomState(31), N, T, C, sharp)
    run(y, beam, beam, top, name="wide bf16", need_clear=-(-3 * N // 4), dtype=torch.bfloat16)


def test_alphabet_wider_than_the_staged_column():
    """Above 8 192 classes the column kernel keeps no copy of the column's logs and takes them again from the posterior."""
    y = B.posterior(np.random.RandomState(8), 4, 5, 8200, 3.0)
    y[0, 2, 8199] = 0.5                                    # the last class, in the tail past the last full wave of classes
    out, _ = run(y, 4, 4, 16, name="C=8200", need_clear=3)
    assert 8199 in out['ids'][0]


def test_maximum_candidates():
    y = B.posterior(np.random.RandomState(7), 8, 26, 96, 2.0)
    run(y, 64, 64, 64, name="64 x 64")


def test_reentry_beside_a_live_child_is_merged():
    """A prefix leaves the beam, its child stays, the prefix is made again: its next extension by the child's symbol IS the child.
    A decoder that tells sameness by fresh node ids returns the child twice (or splits its mass) on these rows."""
    y = B.posterior(np.random.RandomState(0), 200, 12, 5, 1.0)
    out, ref = run(y, 4, 4, 3, name="re-entry")
    hit = [n for n, r in enumerate(ref.r64) if r['reentries'] > 0 and ref.clear[n]]
    print("re-entry beside a live child on clear rows", hit)
    assert len(hit) >= 2


# ---- edges

def test_one_column():
    run(B.posterior(np.random.RandomState(11), 8, 1, 7, 1.0), 4, 4, 16, name="T=1")


def test_beam_of_one():
    out, _ = run(B.posterior(np.random.RandomState(12), 8, 12, 9, 2.0), 1, 1, 16, name="B=1")
    assert np.all(out['count'] == 1)


def test_nbest_below_and_at_the_beam():
    y = B.posterior(np.random.RandomState(13), 8, 12, 9, 2.0)
    few, _ = run(y, 8, 3, 16, name="K=3 of B=8")
    full, _ = run(y, 8, 8, 16, name="K=8 of B=8")
    for key in ('ids', 'lengths', 'scores'):
        assert np.array_equal(few[key].view(np.int32), full[key][:, :3].view(np.int32)), key
    assert np.array_equal(few['count'], np.minimum(full['count'], 3))


def test_no_rows_and_one_row():
    empty = ctc_beam_search_decode(torch.zeros((0, 7, 1, 5), device=DEV), beam=4, nbest=2)
    assert [tuple(empty[k].shape) for k in KEYS] == [(0, 2, 5), (0, 2), (0, 2), (0,)]
    raw_call(torch.zeros((0, 7, 5), device=DEV), 4, 2, 16, override=dict(ws=0, ws_bytes=0))     # MR_OK: no launch, no workspace
    run(B.posterior(np.random.RandomState(14), 1, 9, 7, 1.5), 4, 4, 16, name="N=1")


def test_blank_last_and_unknown_in_and_out_of_range():
    y = B.posterior(np.random.RandomState(15), 8, 10, 6, 1.5)
    run(y, 6, 6, 16, blank=5, unknown=0, name="blank=C-1 unknown=0")
    run(y, 6, 6, 16, blank=5, unknown=-1, name="blank=C-1 no unknown")
    run(y, 6, 6, 16, blank=0, unknown=99, name="unknown=99")
    run(y, 6, 6, 16, blank=2, unknown=3, name="blank=2 unknown=3")


def test_one_symbol_left():
    out, _ = run(B.posterior(np.random.RandomState(16), 8, 7, 3, 1.0), 8, 8, 16, name="C=3")
    assert set(np.unique(out['ids'])) <= {0, 2}


def test_exact_zeros():
    rng = np.random.RandomState(17)
    y = B.posterior(rng, 12, 10, 8, 1.5)
    y[rng.rand(*y.shape) < 0.5] = 0.0                      # half the table, whole columns of some rows among them
    y[0, 3, :] = 0.0
    y[1, :, 0] = 0.0                                       # a row that may never rest on a blank
    out, ref = run(y, 6, 6, 16, name="zeros")
    assert out['count'][0] == 0


def test_a_column_on_unknown_kills_the_row():
    y = B.posterior(np.random.RandomState(18), 4, 9, 6, 1.5)
    y[2, 4, :] = 0.0
    y[2, 4, 1] = 1.0
    out, _ = run(y, 4, 4, 16, name="unknown column")
    assert out['count'].tolist()[2] == 0 and np.all(out['count'][[0, 1, 3]] > 0)
    assert np.all(out['ids'][2] == 0) and np.all(out['lengths'][2] == 0) and np.all(out['scores'][2] == -np.inf)


def test_only_the_empty_string_survives():
    y = np.zeros((3, 6, 5), dtype=np.float32)
    y[:, :, 0] = 1.0
    y[1] = B.posterior(np.random.RandomState(19), 1, 6, 5, 1.0)[0]
    out, _ = run(y, 4, 4, 16, name="blank only")
    for n in (0, 2):
        assert out['count'][n] == 1 and out['lengths'][n, 0] == 0 and out['scores'][n, 0] == 0.0
    assert out['count'][1] == 4


# ---- layouts

def test_layouts_and_logs_give_the_same_bits():
    y = B.posterior(np.random.RandomState(20), 10, 14, 11, 2.0)
    y[3, 5, 4] = 0.0
    args = dict(beam=6, nbest=4, top_classes=5)
    base = host(ctc_beam_search_decode(eval_layout(y), **args))
    compare(base, Reference(B.logs(y), 6, 4, 5), "layout base")
    ntc = torch.from_numpy(y).to(DEV)                                              # [N, T, C]: the class stride is 1
    views = {"[N, C, T]": eval_layout(y).select(2, 0), "transposed": ntc.permute(0, 2, 1),
             "sliced": torch.from_numpy(np.repeat(y, 2, axis=0)).to(DEV).permute(0, 2, 1)[::2],
             "float64": eval_layout(y).double()}
    assert not views["transposed"].is_contiguous() and not views["sliced"].is_contiguous()
    for name, pred in views.items():
        got = host(ctc_beam_search_decode(pred, **args))
        for key in KEYS:
            assert np.array_equal(got[key].view(np.int32), base[key].view(np.int32)), (name, key)
    logs = torch.from_numpy(B.logs(y)).to(DEV).permute(0, 2, 1)                     # rounded as the header says, -inf included
    got = host(ctc_beam_search_decode(logs, log_probs=True, **args))
    for key in KEYS:
        assert np.array_equal(got[key].view(np.int32), base[key].view(np.int32)), ("logs", key)


# ---- invariance

def test_deterministic_row_independent_and_every_output_written():
    y = B.posterior(np.random.RandomState(21), 9, 16, 37, 2.0)
    pred = eval_layout(y)
    one = host(ctc_beam_search_decode(pred, beam=8, nbest=5, top_classes=8))
    two = host(ctc_beam_search_decode(pred, beam=8, nbest=5, top_classes=8))
    _, raw = raw_call(pred, 8, 5, 8)                                               # outputs and workspace start as garbage
    for key in KEYS:
        assert np.array_equal(one[key].view(np.int32), two[key].view(np.int32)), key
        assert np.array_equal(one[key].view(np.int32), raw[key].view(np.int32)), key
    for n in (0, 4, 8):
        alone = host(ctc_beam_search_decode(pred[n:n + 1], beam=8, nbest=5, top_classes=8))
        for key in KEYS:
            assert np.array_equal(alone[key][0].view(np.int32), one[key][n].view(np.int32)), (n, key)


def test_capturable_in_a_graph():
    y = B.posterior(np.random.RandomState(22), 6, 16, 37, 2.0)
    pred, other = eval_layout(y), eval_layout(y[::-1].copy())
    args = dict(beam=8, nbest=3, top_classes=8)
    eager = {k: v.clone() for k, v in ctc_beam_search_decode(pred, **args).items()}          # the call outside
    eager_other = {k: v.clone() for k, v in ctc_beam_search_decode(other, **args).items()}
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


# ---- C ABI

def test_bad_arguments_are_refused_and_nothing_is_written():
    pred = eval_layout(B.posterior(np.random.RandomState(23), 3, 6, 5, 1.0)).select(2, 0)
    cap = _lib._DEFINES["MR_SEQ_MEASURE_MAX"]
    need = _lib.load().mr_ctc_beam_ws_bytes(3, 6, 4, 3)
    refused = [dict(T=0), dict(T=cap + 1), dict(C=1), dict(blank=5), dict(blank=-1), dict(beam=0), dict(beam=65), dict(nbest=0),
               dict(nbest=5), dict(top=0), dict(top=65), dict(ws=0), dict(ws_bytes=need - 1), dict(N=-1)]
    for override in refused:
        _, out = raw_call(pred, 4, 4, 3, expect=1, override=override)
        assert np.all(out['ids'] == 12345) and np.all(out['lengths'] == 12345) and np.all(out['count'] == 12345), override
        assert np.all(out['scores'] == 777.0), override
    _, out = raw_call(pred, 4, 4, 3, expect=2, override=dict(dtype=2))
    assert np.all(out['count'] == 12345)
    with pytest.raises(RuntimeError, match="mr_ctc_beam_search: beam=65"):
        call("mr_ctc_beam_search", 0, ptr(pred), 30, 6, 1, 3, 5, 6, 0, 0, 1, 65, 1, 3, 0, 0, 0, 0, 0, 0)
    raw_call(pred, 4, 4, 3, override=dict(ws_bytes=need))                          # exactly what the query says is enough
