#!/usr/bin/env python
"""Time `AttentionDecoder.read` -- scored greedy decoding and the beam search -- against yardsticks that are not the code under
test: the eval `forward` of the same decoder on the same tensors (greedy decoding without scores: one persistent launch and a
trim) and its per-step loop (MEGREADER_DECODE_PERSIST=0: the launches of a step with a host synchronisation each).  Times are
device events in this process after warm-up; the candidates are measured alternately, `--repeats` times each, and every repeat is
printed (the spread is the noise).

    python tools/bench_attention_read.py          # prints one line per case and one JSON line at the end

Workload (seeded: nothing is downloaded): a randomly initialised AttentionDecoder(in_channels=256) in bf16 -- 38 classes, 32 steps,
H = 512, a 1 x 32 feature grid -- on features [N, 256, 16, 64], N = 32 and 256 crops.  `forward` and `read` both run the encoder
and the image-independent operand preparation; that part is timed on its own ('encode') and subtracted where a line says 'decode'.
The replay read is also timed alone on the states of one greedy decode: its share of the scored greedy call, and the rate of its
S * N * T * H tanh evaluations.  Last, the beam's selection launch (`mr_attn_beam_step`) alone on 64 images of seeded logits, at
beams 8 and 64 and C = 38, 300 and 6 000: its B rounds are serial, so this is where a wide beam over a wide alphabet pays."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_lexicon import timed  # noqa: E402
import megreader_amd as mr  # noqa: E402
from megreader_amd.decoders import AttentionDecoder  # noqa: E402
from megreader_amd.decoders import attention_decoder as ad  # noqa: E402
from megreader_amd.ops.decode import attention_beam_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--crops", type=int, nargs="*", default=[32, 256])
    ap.add_argument("--beams", type=int, nargs="*", default=[1, 4, 8])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_read.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    mr.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(2026)
    dec = AttentionDecoder(in_channels=256).to(dev).eval()
    S, Hd, T, C = dec.max_size, dec.inner_channels, dec.height * dec.max_size, len(dec.charset)
    blank = int(dec.charset.blank)
    results = []
    for N in args.crops:
        feat = torch.randn(N, 256, 16, 64, generator=torch.Generator().manual_seed(N)).to(dev)

        def encode():
            with torch.no_grad():
                enc, E, dtype, eproj, lin_iw, lin_word = dec._encoded(feat)
                return (enc, eproj) + dec._loop_operands(lin_iw, lin_word, E, enc.shape[2], dtype, dev)

        def forward(persist):
            ad.PERSIST_EVAL = persist
            try:
                with torch.no_grad():
                    return dec(feat, train=False)
            finally:
                ad.PERSIST_EVAL = True

        def read(beam, persist=True):
            ad.PERSIST_EVAL = persist
            try:
                return dec.read(feat, beam=beam, nbest=beam)
            finally:
                ad.PERSIST_EVAL = True

        enc, eproj, G, cat, ic, out = encode()
        v = dec.decoder.attn.v
        pred, H_all = ad._greedy_decode(enc, eproj, v, cat, ic, G, out, blank, S, trim=False, states=True)
        # the same words from the one-launch path and from the per-step kernels, wherever the logits are not nearly tied
        steps = read(1, persist=False)['ids'][:, 0]
        same = float((steps == read(1)['ids'][:, 0]).float().mean())
        candidates = {
            'encode_ms': encode,
            'forward_persistent_ms': lambda: forward(True),
            'forward_per_step_ms': lambda: forward(False),
            'read_greedy_ms': lambda: read(1),
            'greedy_launch_ms': lambda: ad._greedy_decode(enc, eproj, v, cat, ic, G, out, blank, S),
            'replay_read_ms': lambda: ad._replay_read(H_all, pred, eproj, v, cat, out, blank, dec.height, dec.max_size),
        }
        for b in args.beams:
            candidates['read_beam%d_per_step_ms' % b] = (lambda b=b: read(b, persist=False))
        runs = {k: [] for k in candidates}
        for _ in range(args.repeats):                                          # alternately: the machine is shared
            for k, fn in candidates.items():
                runs[k].append(timed(fn, args.warmup, args.iters)[0])
        best = {k: min(x) for k, x in runs.items()}
        tanhs = S * N * T * Hd
        case = dict(N=N, S=S, T=T, H=Hd, C=C, words_equal_per_step_vs_persistent=round(same, 4),
                    replay_share_of_read_greedy=round(best['replay_read_ms'] / best['read_greedy_ms'], 3),
                    replay_tanh_per_second=round(tanhs / (best['replay_read_ms'] * 1e-3)),
                    decode_forward_persistent_ms=round(best['forward_persistent_ms'] - best['encode_ms'], 4),
                    decode_forward_per_step_ms=round(best['forward_per_step_ms'] - best['encode_ms'], 4),
                    decode_read_greedy_ms=round(best['read_greedy_ms'] - best['encode_ms'], 4),
                    **{'decode_' + k: round(best[k] - best['encode_ms'], 4) for k in best if k.startswith('read_beam')},
                    **{k: round(x, 4) for k, x in best.items()}, **{k + "_runs": [round(y, 4) for y in x] for k, x in runs.items()})
        print("N=%-3d encode %.3f ms | forward: persistent %.3f, per-step loop %.3f | read greedy %.3f (greedy launch + trim alone "
              "%.3f, replay read alone %.3f = %.0f %% of the call, %.2e tanh/s) | read on the per-step kernels: %s | words equal %.4f"
              "\n      runs: %s"
              % (N, best['encode_ms'], best['forward_persistent_ms'], best['forward_per_step_ms'], best['read_greedy_ms'],
                 best['greedy_launch_ms'], best['replay_read_ms'], 100 * case['replay_share_of_read_greedy'],
                 case['replay_tanh_per_second'],
                 ", ".join("beam %d %.3f" % (b, best['read_beam%d_per_step_ms' % b]) for b in args.beams), same,
                 {k: [round(y, 3) for y in x] for k, x in runs.items()}), flush=True)
        results.append(case)
    # the selection launch alone: B serial rounds, the owner of each round's maximum rescanning its candidates from global memory
    selection = []
    for B, Cs in ((8, 38), (64, 38), (64, 300), (64, 6000)):
        N = 64
        g = torch.Generator().manual_seed(B + Cs)
        logits = (torch.randn(N * B, Cs, generator=g) * 3.0).to(torch.bfloat16).to(dev)
        hprime = torch.randn(N * B, Hd, generator=g).to(torch.bfloat16).to(dev)
        h_next = torch.empty_like(hprime)
        start = (-30.0 * torch.rand(N, B, generator=g)).to(dev)
        score = start.clone()
        finished, length = (torch.zeros((N, B), dtype=torch.int32, device=dev) for _ in range(2))
        parent, word = (torch.zeros((2, N, B), dtype=torch.int32, device=dev) for _ in range(2))
        feed = torch.zeros((N, B), dtype=torch.int64, device=dev)

        def step():
            score.copy_(start)                                                 # (the launch rewrites its state in place)
            finished.zero_()
            attention_beam_step(logits, hprime, h_next, score, finished, length, parent, word, feed, 1, blank)

        def reset_only():
            score.copy_(start)
            finished.zero_()

        ms = [timed(step, args.warmup, 200)[0] - timed(reset_only, args.warmup, 200)[0] for _ in range(args.repeats)]
        selection.append(dict(N=N, beam=B, C=Cs, H=Hd, beam_step_ms=round(min(ms), 4), beam_step_ms_runs=[round(x, 4) for x in ms]))
        print("mr_attn_beam_step alone, %d images, beam %-2d, C = %-4d: %.4f ms   runs: %s"
              % (N, B, Cs, min(ms), [round(x, 4) for x in ms]), flush=True)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), cases=results, selection=selection)))


if __name__ == "__main__":
    main()
