"""The attention beam search: mr_attn_beam_step alone at the C ABI (ops.decode.attention_beam_step) against the restatement of
tests/_attn_ref.py, the whole search (`AttentionDecoder.read`, `_beam_decode`) on the analytically known decoder of
tests/test_attention_eval_gpu.py (restated here) and on a random small one against exhaustive enumeration, and `read` inside a
captured graph.  Scores carry the bar of tests/test_ctc_beam_gpu.py: the kernel's largest error against float64 may be at most
8 x the float32 restatement's own."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_ref as ref  # noqa: E402
import megreader_amd as mr  # noqa: E402
from megreader_amd.decoders import AttentionDecoder  # noqa: E402
from megreader_amd.decoders import attention_decoder as ad  # noqa: E402
from megreader_amd.nn import functional as Fn  # noqa: E402
from megreader_amd.ops.decode import attention_beam_step, attention_beam_trace  # noqa: E402

DEV = "cuda"
BLANK = 0
MARGIN = 1e-4


@pytest.fixture(autouse=True)
def _reset():
    yield
    mr.set_compute_dtype(torch.bfloat16)
    Fn.LSTM_STATUS = None


# ---- one step ----

def step_inputs(N, B, C, seed, dtype=torch.float32, H=24):
    """logits [N * B, C], hprime [N * B, H], score / finished / length [N, B] entering a step s > 0: live slots with scores spread
    over 30 units, every fourth one finished."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(N * B, C, generator=g) * 3.0).to(dtype)
    hprime = torch.randn(N * B, H, generator=g).to(dtype)
    score = -30.0 * torch.rand(N, B, generator=g)
    finished = (torch.arange(N * B).view(N, B) % 4 == 3).to(torch.int32)
    length = torch.randint(0, 3, (N, B), generator=g).to(torch.int32)
    return logits, hprime, score, finished, length


def run_step(logits, hprime, score, finished, length, s, S=8):
    """The kernel on copies of the state: dict(parent, word [N, B], score, finished, length, feed, h_next)."""
    N, B = score.shape
    on = lambda t: t.clone().to(DEV)                                      # noqa: E731
    st = dict(score=on(score), finished=on(finished), length=on(length))
    parent = torch.full((S, N, B), -7, dtype=torch.int32, device=DEV)
    word = torch.full((S, N, B), -7, dtype=torch.int32, device=DEV)
    feed = torch.full((N, B), -7, dtype=torch.int64, device=DEV)
    hp = on(hprime)
    h_next = torch.zeros_like(hp)
    attention_beam_step(on(logits), hp, h_next, st["score"], st["finished"], st["length"], parent, word, feed, s, BLANK)
    torch.cuda.synchronize()
    other = [i for i in range(S) if i != s]
    assert bool((parent[other] == -7).all()) and bool((word[other] == -7).all())      # only step s's plane is written
    out = {k: v.cpu() for k, v in st.items()}
    out.update(parent=parent[s].cpu(), word=word[s].cpu(), feed=feed.cpu(), h_next=h_next.cpu())
    return out


def check_step(logits, hprime, score, finished, length, s, margin=MARGIN):
    """Parents and words exact, scores within the bar, the gather bit for bit; every image's margin asserted first."""
    N, B = score.shape
    C = logits.shape[1]
    got = run_step(logits, hprime, score, finished, length, s)
    lg = logits.double().numpy().reshape(N, B, C)
    e32 = ek = 0.0
    for n in range(N):
        args = (lg[n], score[n].double().numpy(), finished[n].numpy().astype(bool), length[n].numpy(), s, BLANK)
        f64, f32 = ref.beam_step(*args), ref.beam_step(*args, dtype=np.float32)
        vals = np.array(f64["values"])
        live = int((vals[:B] > -np.inf).sum())
        if margin:
            gaps = vals[:live] - vals[1:live + 1]
            assert live > 0 and float(gaps.min()) >= margin, (n, float(gaps.min()))     # no row is let off
        for key in ("parent", "word", "finished", "length"):
            assert np.array_equal(got[key][n].numpy(), f64[key]), (key, n, got[key][n], f64[key])
        assert np.array_equal(got["feed"][n].numpy(), f64["word"])
        assert np.array_equal(np.isneginf(got["score"][n].numpy()), np.isneginf(f64["score"]))
        ok = f64["score"] > -np.inf
        e32 = max(e32, float(np.abs(f32["score"][ok].astype(np.float64) - f64["score"][ok]).max()))
        ek = max(ek, float(np.abs(got["score"][n].double().numpy()[ok] - f64["score"][ok]).max()))
        rows = n * B + torch.from_numpy(f64["parent"]).long()
        assert torch.equal(got["h_next"][n * B:(n + 1) * B], hprime[rows])
    print("B=%d C=%d: score error kernel %.3e, f32 restatement %.3e, ratio %.2f" % (B, C, ek, e32, ek / e32 if e32 else 0.0))
    assert ek <= 8.0 * e32, (ek, e32)
    return got


# seeds found on the host with tests/_attn_ref.py: the float64 margins of every image hold (asserted in check_step)
STEP_SEEDS = {(1, 3): 1, (1, 38): 1, (1, 300): 1, (4, 3): 2, (4, 38): 1, (4, 300): 1, (64, 3): 1, (64, 38): 1, (64, 300): 2}


@pytest.mark.parametrize("B", [1, 4, 64])
@pytest.mark.parametrize("C", [3, 38, 300])
def test_one_step_against_the_restatement(B, C):
    check_step(*step_inputs(3, B, C, STEP_SEEDS[(B, C)]), s=3)


def test_one_step_bf16_and_rows_that_are_no_16_byte_pieces():
    check_step(*step_inputs(3, 4, 38, 1, dtype=torch.bfloat16, H=5), s=2)


def test_step_zero_starts_from_slot_zero_whatever_the_state_holds():
    logits, hprime, score, finished, length = step_inputs(3, 4, 38, 1)
    got = check_step(logits, hprime, score + 100.0, torch.ones_like(finished), length + 9, s=0)
    assert bool((got["parent"] == 0).all()) and bool((got["score"] <= 0).all())


def test_ties_go_to_the_smaller_index():
    """Slots 1 and 2 are one hypothesis twice (bit-equal logits and scores), and classes 1 and 2 of slot 0 have one logit: among
    bit-equal candidates the smaller b * C + c comes first."""
    N, B, C = 2, 4, 3
    logits = torch.tensor([[0.0, -1.5, -1.5], [0.25, -2.0, -0.75], [0.25, -2.0, -0.75], [3.0, 0.0, 1.0]]).repeat(N, 1)
    score = torch.tensor([[-0.5, -1.0, -1.0, -40.0]]).repeat(N, 1)
    zeros = torch.zeros(N, B, dtype=torch.int32)
    got = check_step(logits, torch.randn(N * B, 8), score, zeros, zeros + 2, s=2, margin=0.0)
    for n in range(N):
        picked = list(zip(got["parent"][n].tolist(), got["word"][n].tolist()))
        assert picked == [(0, 0), (1, 0), (2, 0), (0, 1)], picked                 # (1, 0) before its copy (2, 0)
    # ... and with four dead slots behind them there is room for every pair: -0.87, -1.39 x 2, -2.37 x 2, -2.39 x 2, -3.64 x 2
    dead = torch.full((N, 4), float("-inf"))
    wide = check_step(torch.cat([logits.view(N, B, C), torch.zeros(N, 4, C)], 1).reshape(N * 8, C), torch.randn(N * 8, 8),
                      torch.cat([score, dead], 1), torch.zeros(N, 8, dtype=torch.int32), torch.zeros(N, 8, dtype=torch.int32),
                      s=1, margin=0.0)
    for n in range(N):
        picked = list(zip(wide["parent"][n].tolist(), wide["word"][n].tolist()))
        assert picked == [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (1, 2), (2, 2), (1, 1)], picked


def test_finished_and_dead_slots():
    """A finished hypothesis offers its blank at its own score and nothing else; a dead slot offers nothing; with fewer candidates
    than slots the last slots are dead."""
    N, B, C = 2, 4, 3
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(N * B, C, generator=g)
    logits[0] = torch.tensor([2.0, 0.0, -4.0])           # slot 0 of image 0 offers -1.13, -3.13 and -7.13
    ninf = float("-inf")
    score = torch.tensor([[-1.0, -0.2, ninf, -3.0], [ninf, -2.0, ninf, ninf]])
    finished = torch.tensor([[0, 1, 0, 1], [0, 1, 0, 0]], dtype=torch.int32)
    length = torch.tensor([[2, 1, 0, 0], [0, 2, 0, 0]], dtype=torch.int32)
    got = check_step(logits, torch.randn(N * B, 16, generator=g), score, finished, length, s=2, margin=1e-3)
    assert list(zip(got["parent"][0].tolist(), got["word"][0].tolist())) == [(1, BLANK), (0, 0), (3, BLANK), (0, 1)]
    assert got["score"][0, 0] == torch.tensor(-0.2) and got["score"][0, 2] == -3.0        # their own scores, unchanged
    # (0, 0) is slot 0's blank: it ends there with the s = 2 symbols it had; (0, 1) goes on with a third
    assert got["length"][0].tolist() == [1, 2, 0, 3] and got["finished"][0].tolist() == [1, 1, 1, 0]
    # image 1: one finished hypothesis and nothing else -> one live slot, three dead ones
    assert got["score"][1].tolist() == [-2.0, ninf, ninf, ninf] and got["finished"][1].tolist() == [1, 0, 0, 0]
    assert got["length"][1].tolist() == [2, 0, 0, 0] and got["word"][1].tolist() == [BLANK] * 4


def test_bad_arguments_are_refused():
    logits, hprime, score, finished, length = (t.to(DEV) for t in step_inputs(2, 4, 5, 1))
    parent = torch.zeros((3, 2, 4), dtype=torch.int32, device=DEV)
    feed = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="step 3 of S=3"):
        attention_beam_step(logits, hprime, torch.empty_like(hprime), score, finished, length, parent, parent.clone(), feed, 3, BLANK)
    with pytest.raises(RuntimeError, match="h_next == hprime"):
        attention_beam_step(logits, hprime, hprime, score, finished, length, parent, parent.clone(), feed, 1, BLANK)
    with pytest.raises(RuntimeError, match="blank=5"):
        attention_beam_step(logits, hprime, torch.empty_like(hprime), score, finished, length, parent, parent.clone(), feed, 1, 5)
    with pytest.raises(RuntimeError, match="nbest=5"):
        attention_beam_trace(parent, parent.clone(), score, finished, length, 5, BLANK)


# ---- the whole search ----

H = 512


def _permutation_decoder(pi):
    """tests/test_attention_eval_gpu.py's decoder, restated: the next word is pi(last word), whatever the image -- the word's +-1
    pattern P[c] passes through the n gate (h' = tanh(4 P[c]), z = sigmoid(-30) = 0) and the output layer's row pi(c) is P[c]: the
    own-class logit is ~512 against |x| < ~100 elsewhere, so every step's probability is 1 to float32."""
    torch.manual_seed(3)
    dec = AttentionDecoder(in_channels=256)
    cell = dec.decoder
    C = len(dec.charset)
    g = torch.Generator().manual_seed(8)
    P = (torch.randint(0, 2, (C, H), generator=g) * 2 - 1).float()
    with torch.no_grad():
        cell.word_linear.weight.copy_(P.t())
        cell.word_linear.bias.zero_()
        cell.rnn.weight_ih.zero_()
        cell.rnn.weight_ih[2 * H:, :H] = 4 * torch.eye(H)
        cell.rnn.weight_hh.zero_()
        cell.rnn.bias_hh.zero_()
        cell.rnn.bias_ih.zero_()
        cell.rnn.bias_ih[H:2 * H] = -30
        cell.out.weight.copy_(P[torch.argsort(torch.tensor(pi))])
        cell.out.bias.zero_()
    return dec.to(DEV).eval()


CYCLE = [0, 5, 9, 3, 20, 11, 37]          # pi^7(blank) = blank: the string is 5 9 3 20 11 37, then the blank


def _pi(C):
    pi = list(range(C))
    for a, b in zip(CYCLE, CYCLE[1:] + CYCLE[:1]):
        pi[a] = b
    return pi


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_known_decoder_beams_1_4_8(dtype):
    mr.set_compute_dtype(dtype)
    N, S = 3, 32
    dec = _permutation_decoder(_pi(38))
    feat = torch.randn(N, 256, 16, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    want = CYCLE[1:]
    with torch.no_grad():
        pred = dec(feat, train=False).cpu()
    for beam in (1, 4, 8):
        nbest = min(beam, 3)
        out = {k: v.cpu() for k, v in dec.read(feat, beam=beam, nbest=nbest, attention=(beam == 4)).items()}
        assert out["ids"].shape == (N, nbest, S) and out["ids"].dtype == torch.int32
        for n in range(N):
            assert out["lengths"][n, 0] == len(want) and out["ids"][n, 0, :6].tolist() == want
            # blank from the end of the string on, on every path: the one-launch kernel's cycle starts again behind the blank
            assert bool((out["ids"][n, 0, 6:] == BLANK).all()) and abs(float(out["scores"][n, 0])) < 1e-3
            assert out["count"][n] == nbest
            assert bool((out["scores"][n, 1:] <= out["scores"][n, :-1]).all()) and bool(torch.isfinite(out["scores"][n]).all())
            assert bool((out["sym_lp"][n, :7].abs() < 1e-3).all())
        assert out["moments"].shape == (N, S, 4) and bool(torch.isfinite(out["moments"]).all())
        if beam == 1:           # forward's eval prediction up to the first blank
            assert torch.equal(out["ids"][:, 0, :7], pred[:, :7])
        if beam == 4:
            assert out["att"].shape == (N, S, dec.height, dec.max_size)
            assert bool(((out["att"].sum((2, 3)) - 1).abs() < 1e-5).all())


def _small_decoder(N, T, Hd, Ep, C, seed, dtype):
    g = np.random.default_rng(seed)
    p = dict(cat_w=g.normal(size=(4 * Hd, Hd)) * 0.5, cat_b=g.normal(size=4 * Hd) * 0.1, eproj=g.normal(size=(N, T, Hd)),
             enc=g.normal(size=(N, T, Ep)), v=g.normal(size=Hd), ic_w=g.normal(size=(3 * Hd, Ep)) * 0.4,
             G=g.normal(size=(C, 3 * Hd)), out_w=g.normal(size=(C, Hd)) * 1.5, out_b=g.normal(size=C) * 0.3)
    t = {k: torch.from_numpy(a).to(dtype) for k, a in p.items()}
    p = {k: a.double().numpy() for k, a in t.items()}                    # the restatements see the rounded values
    t = {k: a.to(DEV) for k, a in t.items()}
    f = lambda a: a.float()                                              # noqa: E731
    cat = ad._SeqLinear([f(t["cat_w"][:Hd]), f(t["cat_w"][Hd:])], [None, f(t["cat_b"][Hd:])], Hd, dtype)
    ic = ad._SeqLinear(f(t["ic_w"]), None, Ep, dtype)
    out = ad._SeqLinear(f(t["out_w"]), f(t["out_b"]), Hd, dtype)
    p["cat_b"][:Hd] = 0.0                                                # (the attention half has no bias in the stack)
    return p, t, cat, ic, out


SMALL_SEED = 1          # found on the host: every image's 15 strings are 1e-3 apart in float64 (asserted below)


def test_random_small_decoder_against_enumeration():
    """f32, H = 4 (one 16-byte vector: the least K of mr_gemm_nt), C = 3, S = 3, beam 32 >= 27: nothing is pruned, so the beam
    returns every string with its exact probability."""
    N, T, Hd, Ep, C, S, B = 2, 5, 4, 4, 3, 3, 32
    dtype = torch.float32
    p, t, cat, ic, out = _small_decoder(N, T, Hd, Ep, C, SMALL_SEED, dtype)
    got = ad._beam_decode(t["enc"].contiguous(), t["eproj"].contiguous(), t["v"], cat, ic, t["G"].contiguous(), out, BLANK, S,
                          beam=B, nbest=B)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    _, _, s32, _ = ref.beam_search(p, S, BLANK, B, B, dtype=np.float32)
    e32 = ek = 0.0
    for n in range(N):
        want = ref.enumerate_strings(p, n, S, BLANK)
        lps = np.array([w[2] for w in want])
        assert len(want) == 15 and float((lps[:-1] - lps[1:]).min()) >= 1e-3
        assert got["count"][n] == 15
        for j, (string, ended, lp) in enumerate(want):
            k = int(got["lengths"][n, j])
            assert tuple(got["ids"][n, j, :k]) == string and bool((got["ids"][n, j, k:] == BLANK).all()), (n, j)
        e32 = max(e32, float(np.abs(s32[n, :15].astype(np.float64) - lps).max()))
        ek = max(ek, float(np.abs(got["scores"][n, :15].astype(np.float64) - lps).max()))
        assert np.all(np.isneginf(got["scores"][n, 15:])) and np.all(got["lengths"][n, 15:] == 0)
    print("small decoder: score error kernel %.3e, f32 restatement %.3e, ratio %.2f" % (ek, e32, ek / e32))
    assert ek <= 8.0 * e32, (ek, e32)
    # the states of the first hypothesis are the float64 decoder's along its words
    h, feed = np.zeros((N, Hd)), np.full(N, BLANK)
    for s in range(S):
        h, _, _, _ = ref.decoder_step(p, h, feed)
        assert np.abs(got["states"][s + 1] - h).max() < 1e-4
        feed = got["ids"][:, 0, s].astype(np.int64)
    assert got["path"].shape == (N, B, S + 1) and np.all(got["path"][:, :15, 0] == 0)
    assert np.array_equal(got["path"][:, :, S], np.where(np.arange(B) < 15, np.arange(B), 0)[None].repeat(N, 0))


def test_read_replays_from_a_captured_graph():
    """Nothing in `read` looks at the device: greedy (the persistent launch and its stored states) and a beam of 2 replay from one
    graph each and give the other input's result."""
    mr.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(5)
    dec = AttentionDecoder(in_channels=256).to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    static = torch.randn(4, 256, 16, 64, generator=g).to(DEV)
    first = static.clone()
    other = (torch.randn(4, 256, 16, 64, generator=g) * 1.3).to(DEV)
    for beam in (1, 2):
        static.copy_(first)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dec.read(static, beam=beam, nbest=beam)                      # eager warm-up: weight images, code objects
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = dec.read(static, beam=beam, nbest=beam)
        static.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        eager = dec.read(other, beam=beam, nbest=beam)
        assert set(replayed) == {'ids', 'lengths', 'scores', 'count', 'sym_lp', 'moments'}
        for k in replayed:
            assert torch.equal(replayed[k], eager[k]), (beam, k)
        assert bool(torch.isfinite(replayed['scores']).all())
