"""Eval (greedy) decode of the attention head on the GPU: the one-launch path (decoders/attention_decoder.py: _greedy_decode =
mr_decode_greedy_fwd + mr_decode_greedy_trim, with the word table built in front of it) against the per-step eval loop, which is
restated here launch for launch as AttentionDecoder.forward runs it (embedding gather, five _SeqLinear GEMMs, _AttnStepFn,
_GruGatesFn, mr_nll_step_fwd, a clone, a column write and bool((am == blank).all()) per step).
  python tools/microbench_decode_eval.py [--out FILE]
Shapes (N, T, Ep, S, C) = (32, 64, 552, 32, 38) and (16, 64, 552, 32, 38), bf16; the blank's output bias is -10, so no step stops
the loop early (checked).  Every figure is the median over ROUNDS rounds of REPS calls with the smallest and the largest round
behind it (the spread); the versions alternate round by round in one process after 3 warm-up calls each.  Two clocks per round:
device events around the calls, and the host clock from the first call to the end of a final synchronise (the per-step loop holds
a host synchronisation per step, so its device-event time and its wall time are both of interest)."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from megreader_amd._lib import call, dtype_code, load, ptr, vec_of  # noqa: E402
from megreader_amd.decoders import attention_decoder as ad  # noqa: E402

ROUNDS, REPS = 7, 20
SHAPES = [(32, 64, 552, 32, 38), (16, 64, 552, 32, 38)]
DEV = "cuda"
H = 512
BF = torch.bfloat16
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def one_round(fn, reps=REPS):
    """(us per call by device events, us per call by the host clock up to the end of a synchronise)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return e0.elapsed_time(e1) / reps * 1e3, (t1 - t0) / reps * 1e6


def rounds(*fns):
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            e, w = one_round(fn)
            ev[i].append(e)
            wall[i].append(w)
    return ev, wall


def fmt(us):
    return "%8.1f us (min %.1f, max %.1f)" % (statistics.median(us), min(us), max(us))


class Problem(object):
    """A decoder cell with its default initialisation (blank's output bias -10) and a random encoder sequence."""

    def __init__(self, N, T, Ep, S, C, seed=0):
        torch.manual_seed(seed)
        self.N, self.T, self.Ep, self.S, self.C, self.blank = N, T, Ep, S, C, 0
        self.E = Ep - 7                                  # 545 = 512 channels + 33 position columns, padded to 552
        self.cell = ad.AttentionRNNCell(H, self.E - H, C).to(DEV)
        with torch.no_grad():
            self.cell.out.bias[self.blank] = -10.0
        g = torch.Generator().manual_seed(seed + 1)
        enc = torch.randn(N, T, Ep, generator=g)
        enc[:, :, self.E:] = 0
        self.enc = enc.to(BF).to(DEV).contiguous()
        cell, E = self.cell, self.E
        Wa = cell.attn.attn.weight
        self.Cp = ad._ceil_to(C, vec_of(BF))
        self.lin_e = ad._SeqLinear(Wa[:, H:H + E], cell.attn.attn.bias, Ep, BF)
        self.lin_iw = ad._SeqLinear(cell.rnn.weight_ih[:, :H], cell.rnn.bias_ih, H, BF)
        self.lin_word = ad._SeqLinear(cell.word_linear.weight, cell.word_linear.bias, self.Cp, BF)
        self.lin_h = ad._SeqLinear(Wa[:, :H], None, H, BF)
        self.lin_ic = ad._SeqLinear(cell.rnn.weight_ih[:, H:H + E], None, Ep, BF)
        self.lin_hh = ad._SeqLinear(cell.rnn.weight_hh, cell.rnn.bias_hh, H, BF)
        self.lin_out = ad._SeqLinear(cell.out.weight, cell.out.bias, H, BF)
        self.cat = ad._SeqLinear([Wa[:, :H], cell.rnn.weight_hh], [None, cell.rnn.bias_hh], H, BF)
        with torch.no_grad():
            self.eproj = self.lin_e(self.enc.view(N * T, Ep))[:, :H].reshape(N, T, H).contiguous()

    def one_launch(self):
        """what the eval branch of AttentionDecoder.forward runs behind eproj on the one-launch path"""
        cell = self.cell
        with torch.no_grad():
            rows = ad._EmbedRowsFn.apply(torch.arange(self.C, device=DEV), cell.embedding.weight, self.Cp, BF)
            G = self.lin_iw(self.lin_word(rows))
            return ad._greedy_decode(self.enc, self.eproj, cell.attn.v, self.cat, self.lin_ic, G, self.lin_out, self.blank, self.S)

    def per_step(self):
        """... and on the per-step path (the loop of AttentionDecoder.forward, restated)"""
        cell, N, C, S = self.cell, self.N, self.C, self.S
        att_state = {'dtype': BF}
        hidden = torch.zeros((N, H), dtype=BF, device=DEV)
        word_idx = torch.full((N,), self.blank, dtype=torch.int64, device=DEV)
        pred = torch.full((N, S), self.blank, dtype=torch.int32, device=DEV)
        probs = torch.empty((N, C), dtype=torch.float32, device=DEV)
        am = torch.empty((N,), dtype=torch.int64, device=DEV)
        with torch.no_grad():
            for t in range(S):
                word = self.lin_word(ad._EmbedRowsFn.apply(word_idx, cell.embedding.weight, self.Cp, BF))
                w, context = ad._AttnStepFn.apply(self.lin_h(hidden), self.eproj, self.enc, cell.attn.v, att_state, t == 0)
                hidden = ad._GruGatesFn.apply(self.lin_iw(word), self.lin_ic(context), self.lin_hh(hidden), hidden, BF)
                logits = self.lin_out(hidden)
                call("mr_nll_step_fwd", dtype_code(BF), ptr(logits), logits.stride(0), 0, 0, 0, ptr(probs), 0, ptr(am), N, C, 0, 1)
                word_idx = am.clone()
                pred[:, t] = am
                if bool((am == self.blank).all()):
                    break
        return pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_decode_eval.py measures on the GPU; there is none")
    load()
    say("%s, %d rounds of %d calls per figure; eval decode, bf16, H = 512" % (torch.cuda.get_device_name(0), ROUNDS, REPS))
    verdict = []
    for N, T, Ep, S, C in SHAPES:
        p = Problem(N, T, Ep, S, C)
        assert ad._greedy_persist_ok(BF, N, T, H, Ep, C), "the one-launch path does not take this shape on this device"
        a_pred, b_pred = p.one_launch(), p.per_step()
        torch.cuda.synchronize()
        assert not bool((b_pred == p.blank).all(0).any()) and not bool((a_pred == p.blank).all(0).any()), "a step stopped the loop"
        same = int((a_pred == b_pred).sum())
        # the one-launch path replayed from a graph (it holds no host synchronisation; the per-step loop cannot be captured)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            p.one_launch()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            p.one_launch()
        ev, wall = rounds(p.one_launch, p.per_step, graph.replay)
        say("(N, T, Ep, S, C) = (%d, %d, %d, %d, %d): words identical at %d of %d positions" % (N, T, Ep, S, C, same, N * S))
        for name, i in (("one launch (word table + decode + trim), eager", 0), ("per-step loop, eager", 1),
                        ("one launch, replayed from a graph", 2)):
            say("  %-48s events %s | wall incl. synchronise %s" % (name, fmt(ev[i]), fmt(wall[i])))
        say("  per-step / one launch: events x%.1f, wall x%.1f" %
            (statistics.median(ev[1]) / statistics.median(ev[0]), statistics.median(wall[1]) / statistics.median(wall[0])))
        verdict.append(max(ev[0]) < min(ev[1]) and max(wall[0]) < min(wall[1]))
    say("the one-launch path is faster than the per-step loop beyond the spread at both shapes, by both clocks: %s" % all(verdict))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
