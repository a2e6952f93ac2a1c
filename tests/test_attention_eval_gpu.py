"""Eval (greedy decode) of decoders.AttentionDecoder: the one-launch path (`_greedy_decode`: mr_decode_greedy_fwd + one trim)
against an analytically known decoder, against the per-step loop and fp32, in chunks of 64 rows, and inside a captured graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd.decoders import AttentionDecoder  # noqa: E402
from megreader_amd.decoders import attention_decoder as ad  # noqa: E402
from megreader_amd.nn import functional as Fn  # noqa: E402

DEV = "cuda"
H = 512


@pytest.fixture(autouse=True)
def _reset():
    yield
    mr.set_compute_dtype(torch.bfloat16)
    Fn.LSTM_STATUS = None


def _permutation_decoder(pi):
    """A decoder whose next word is pi(last word), whatever the image: the word's +-1 pattern P[c] passes through the n gate
    (h' = tanh(4 P[c]), z = sigmoid(-30) = 0, nothing from the context or the old state) and the output layer's row pi(c) is
    P[c]: own-class logit ~ 512 against |x| < ~100 elsewhere, so no rounding of bf16 or fp32 can change a word."""
    torch.manual_seed(3)
    dec = AttentionDecoder(in_channels=256)
    cell = dec.decoder
    C = len(dec.charset)
    g = torch.Generator().manual_seed(8)
    P = (torch.randint(0, 2, (C, H), generator=g) * 2 - 1).float()
    with torch.no_grad():
        assert torch.equal(cell.embedding.weight, torch.eye(C))
        cell.word_linear.weight.copy_(P.t())
        cell.word_linear.bias.zero_()
        cell.rnn.weight_ih.zero_()
        cell.rnn.weight_ih[2 * H:, :H] = 4 * torch.eye(H)
        cell.rnn.weight_hh.zero_()
        cell.rnn.bias_hh.zero_()
        cell.rnn.bias_ih.zero_()
        cell.rnn.bias_ih[H:2 * H] = -30
        cell.out.weight.copy_(P[torch.argsort(torch.tensor(pi))])        # row pi(c) = P[c]
        cell.out.bias.zero_()
    return dec.to(DEV).eval()


def _expected(pi, blank, N, S):
    """The reference loop on that decoder: pi^(s+1)(blank) until every row emitted blank, blank behind."""
    row, w, stopped = [], blank, False
    for s in range(S):
        w = pi[w]
        row.append(blank if stopped else w)
        stopped = stopped or w == blank
    return torch.tensor([row] * N, dtype=torch.int32)


def _pi_returning(C, cycle):
    pi = list(range(C))
    for a, b in zip(cycle, cycle[1:] + cycle[:1]):
        pi[a] = b
    return pi


@pytest.mark.parametrize("which", ["returns to blank at step 6", "never returns"])
def test_known_permutation_decoder(which, monkeypatch):
    C, N, S = 38, 6, 32
    if which == "never returns":
        pi = [(c + 1) % C for c in range(C)]                 # 38 > 32 steps: no early stop
    else:
        pi = _pi_returning(C, [0, 5, 9, 3, 20, 11, 37])      # pi^7(blank) = blank: step 6 emits blank everywhere, 25 steps are cut
    want = _expected(pi, 0, N, S)
    assert (which == "never returns") == bool((want != 0).all())
    feat = torch.randn(N, 256, 16, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    dec = _permutation_decoder(pi)
    assert int(dec.charset.blank) == 0

    def run():
        with torch.no_grad():
            p = dec(feat, train=False)
        assert p.dtype == torch.int32 and p.shape == (N, S)
        return p.cpu()

    # bf16, one launch
    mr.set_compute_dtype(torch.bfloat16)
    Fn.LSTM_STATUS = status = []
    got = run()
    assert len(status) == 1 and int(status[0].view(torch.int32).item()) == 0          # one launch, no hand-off timed out
    assert torch.equal(got, want)
    # bf16, the per-step loop
    monkeypatch.setattr(ad, "PERSIST_EVAL", False)
    Fn.LSTM_STATUS = status = []
    got = run()
    assert status == []
    assert torch.equal(got, want)
    monkeypatch.setattr(ad, "PERSIST_EVAL", True)
    # fp32 (always the per-step loop)
    mr.set_compute_dtype(torch.float32)
    Fn.LSTM_STATUS = status = []
    got = run()
    assert status == []
    assert torch.equal(got, want)


def _random_decode_inputs(N, T=32, Ep=552, C=38, seed=2, same_from=64):
    """Random weights and sequences; the rows from `same_from` on are copies of one another, so they emit the same words."""
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16

    def dev(t, dt=bf):
        return t.to(dt).to(DEV).contiguous()
    enc = torch.randn(N, T, Ep, generator=g)
    eproj = torch.randn(N, T, H, generator=g) * 0.7
    enc[same_from:] = enc[same_from]
    eproj[same_from:] = eproj[same_from]
    enc, eproj = dev(enc), dev(eproj)
    v = dev(torch.randn(H, generator=g) * H ** -0.5 * 4, torch.float32)
    w_ah = dev(torch.randn(H, H, generator=g) * H ** -0.5, torch.float32)
    w_hh = dev(torch.randn(3 * H, H, generator=g) * H ** -0.5, torch.float32)
    b_hh = dev(torch.randn(3 * H, generator=g) * 0.1, torch.float32)
    w_ic = dev(torch.randn(3 * H, Ep, generator=g) * Ep ** -0.5, torch.float32)
    w_out = dev(torch.randn(C, H, generator=g) * H ** -0.5 * 3, torch.float32)
    b_out = torch.randn(C, generator=g) * 0.2
    b_out[0] += 1.5                  # blank is a frequent word
    b_out = dev(b_out, torch.float32)
    G = dev(torch.randn(C, 3 * H, generator=g) * 0.5)
    cat = ad._SeqLinear([w_ah, w_hh], [None, b_hh], H, bf)
    ic = ad._SeqLinear(w_ic, None, Ep, bf)
    out = ad._SeqLinear(w_out, b_out, H, bf)
    return enc, eproj, v, cat, ic, G, out


def test_batches_beyond_64_rows_run_in_chunks_with_one_trim():
    N, S, blank = 70, 32, 0
    enc, eproj, v, cat, ic, G, out = _random_decode_inputs(N)
    Fn.LSTM_STATUS = status = []
    got = ad._greedy_decode(enc, eproj, v, cat, ic, G, out, blank, S)
    torch.cuda.synchronize()
    assert len(status) == 2 and all(int(w.view(torch.int32).item()) == 0 for w in status)
    assert got.dtype == torch.int32 and got.shape == (N, S)
    Fn.LSTM_STATUS = None
    parts = [ad._greedy_decode(enc[a:b].contiguous(), eproj[a:b].contiguous(), v, cat, ic, G, out, blank, S, trim=False)
             for a, b in ((0, 64), (64, 70))]
    whole = torch.cat(parts, 0)
    assert int(whole.min()) >= 0 and int(whole.max()) < 38
    want = whole.clone()
    hit = (want == blank).all(0).nonzero()
    if hit.numel():
        want[:, int(hit[0]) + 1:] = blank
    assert torch.equal(got, want)
    alone, batch = (parts[1] == blank).all(0), (whole == blank).all(0)
    print("all-blank steps: batch %d, rows 64..69 alone %d" % (int(batch.sum()), int(alone.sum())))


def test_eval_forward_is_capturable():
    """No host synchronisation on the one-launch path: a whole eval forward (encoder + decode) replays from a graph."""
    mr.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(5)
    dec = AttentionDecoder(in_channels=256).to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    static = torch.randn(4, 256, 16, 64, generator=g).to(DEV)
    other = (torch.randn(4, 256, 16, 64, generator=g) * 1.3).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            dec(static, train=False)                         # eager warm-up: weight images, code objects
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = dec(static, train=False)
        static.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        eager = dec(other, train=False)
    assert replayed.dtype == torch.int32 and replayed.shape == (4, 32)
    assert torch.equal(replayed, eager)
