#!/usr/bin/env python
"""Time `ctc_forced_align` (mr_ctc_align) on recognition batches against a yardstick that is not the code under test: the same
batched Viterbi recursion and back-trace written out of torch tensor operations (T steps of `maximum` / `where`, the back-trace by
`gather`), run on the same tensors.  Both must give the same paths on every row.  Times are device events in this process after
warm-up; the two are measured alternately, `--repeats` times each, and every repeat is printed (the spread is the noise).

    python tools/bench_ctc_align.py               # prints one line per case and one JSON line at the end

Workload (seeded: nothing is downloaded): posteriors [N, C, 1, T], the softmax of noise plus a path that spells a random string
with a blank between its symbols; the string is what is aligned.  Cases: 256 rows x 32 columns, 8 symbols, C = 37 and C = 6 000;
256 rows x 129 columns, 25 symbols, C = 37.  To see where a call's time goes the kernel is also timed on the logs of the same
posterior (log_probs=True: no f64 log per cell) and through the C entry point with outputs and workspace allocated once (no
allocator, no Python wrapper)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_lexicon import timed  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.ops.decode import ctc_forced_align  # noqa: E402

CASES = [(256, 32, 8, 37), (256, 32, 8, 6000), (256, 129, 25, 37)]       # rows, columns, symbols, classes


def make_case(rng, N, T, K, C, sharp):
    """(pred f32 [N, C, 1, T], targets i32 [N, K], lengths i32 [N]) on the host; classes 0 / 1 are blank / unknown."""
    logits = rng.randn(N, T, C).astype(np.float32)
    targets = rng.randint(2, C, size=(N, K)).astype(np.int32)
    for n in range(N):
        path = np.zeros(T, dtype=np.int64)
        path[1:2 * K:2] = targets[n]
        logits[n, np.arange(T), path] += sharp
    y = torch.softmax(torch.from_numpy(logits), dim=-1)
    return y.permute(0, 2, 1).contiguous().unsqueeze(2), torch.from_numpy(targets), torch.full((N,), K, dtype=torch.int32)


def torch_viterbi(pred, targets, lengths, blank=0, log_probs=False):
    """(score f32 [N], pos i64 [N, T]) by tensor operations: the recursion of include/megreader_hip.h (mr_ctc_align) with its tie
    rule, every row at once, one column per step.  Targets must be alignable (this is a yardstick, not an entry point)."""
    pred = pred.select(2, 0)
    N, C, T = pred.shape
    S = targets.shape[1]
    P = 2 * S + 1
    dev = pred.device
    ninf = float("-inf")
    ext = torch.full((N, P), blank, dtype=torch.long, device=dev)
    ext[:, 1::2] = targets.long()
    lp = pred if log_probs else pred.double().log().float()
    emit = lp.gather(1, ext[:, :, None].expand(N, P, T))                       # [N, P, T]
    live = torch.arange(P, device=dev)[None, :] < (2 * lengths.long() + 1)[:, None]
    emit = torch.where(live[:, :, None], emit, torch.full_like(emit, ninf))
    hop = torch.zeros((N, P), dtype=torch.bool, device=dev)
    if S > 1:
        hop[:, 3::2] = ext[:, 3::2] != ext[:, 1:-2:2]
    d = torch.full((N, P), ninf, device=dev)
    d[:, :2] = emit[:, :2, 0]
    back = torch.empty((T, N, P), dtype=torch.long, device=dev)
    back[0] = 0
    pad = torch.full((N, 2), ninf, device=dev)
    for t in range(1, T):
        shifted = torch.cat([pad, d], dim=1)
        b, c = shifted[:, 1:P + 1], torch.where(hop, shifted[:, :P], pad[:, :1])
        take_b = b > d
        best = torch.where(take_b, b, d)
        take_c = c > best
        best = torch.where(take_c, c, best)
        back[t] = torch.where(take_c, 2, take_b.long())
        d = emit[:, :, t] + best
    last = (2 * lengths.long())[:, None]
    d_blank, d_symbol = d.gather(1, last), d.gather(1, (last - 1).clamp(min=0))
    s = torch.where((last == 0) | (d_blank >= d_symbol), last, last - 1)
    score = d.gather(1, s)[:, 0]
    pos = torch.empty((N, T), dtype=torch.long, device=dev)
    for t in range(T - 1, -1, -1):
        pos[:, t] = s[:, 0]
        s = s - back[t].gather(1, s)
    return score, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sharp", type=float, default=4.0, help="what the spelled path is raised by (logits of unit noise)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--yardstick-iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_align.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    results = []
    for N, T, K, C in CASES:
        rng = np.random.RandomState(2026 + C + T)
        pred, targets, lengths = (x.to(dev) for x in make_case(rng, N, T, K, C, args.sharp))
        logs = pred.double().log().float()
        out = ctc_forced_align(pred, targets, lengths)
        score, pos = torch_viterbi(pred, targets, lengths)
        assert bool(torch.isfinite(out['score']).all())
        assert torch.equal(out['pos'].long(), pos), "N=%d T=%d K=%d C=%d: the paths differ" % (N, T, K, C)
        assert torch.equal(out['score'], score), "N=%d T=%d K=%d C=%d: the scores differ" % (N, T, K, C)
        on_logs = ctc_forced_align(logs, targets, lengths, log_probs=True)
        assert torch.equal(on_logs['pos'], out['pos'])
        # the C entry point alone: outputs and workspace allocated once
        ws = torch.empty(_lib.load().mr_ctc_align_ws_bytes(N, T, K) // 8 + 1, dtype=torch.int64, device=dev)
        row = pred.select(2, 0)
        sn, sc, st = row.stride()

        def entry():
            call("mr_ctc_align", 0, ptr(row), sn, sc, st, N, C, T, 0, 0, 1, ptr(targets), K, ptr(lengths), ptr(out['score']),
                 ptr(out['pos']), ptr(out['begin']), ptr(out['end']), ptr(out['sym_lp']), ptr(out['peak']), ptr(ws),
                 ws.numel() * 8)

        runs = {'align_ms': [], 'entry_ms': [], 'align_on_logs_ms': [], 'torch_viterbi_ms': []}
        for _ in range(args.repeats):                                          # alternately: the machine is shared
            runs['align_ms'].append(timed(lambda: ctc_forced_align(pred, targets, lengths), args.warmup, args.iters)[0])
            runs['torch_viterbi_ms'].append(timed(lambda: torch_viterbi(pred, targets, lengths), 2, args.yardstick_iters)[0])
            runs['entry_ms'].append(timed(entry, args.warmup, args.iters)[0])
            runs['align_on_logs_ms'].append(timed(lambda: ctc_forced_align(logs, targets, lengths, log_probs=True),
                                                  args.warmup, args.iters)[0])
        best = {k: min(v) for k, v in runs.items()}
        case = dict(rows=N, columns=T, symbols=K, classes=C, paths_equal=True,
                    ratio_to_torch=round(best['torch_viterbi_ms'] / best['align_ms'], 1),
                    **{k: round(best[k], 4) for k in runs}, **{k + "_runs": [round(x, 4) for x in v] for k, v in runs.items()})
        print("N=%d T=%-3d K=%-2d C=%-5d ctc_forced_align %.4f ms (entry point alone %.4f, on logs %.4f)   torch Viterbi %.3f ms "
              "(x%.1f)   equal paths and scores on %d rows   runs: %s"
              % (N, T, K, C, best['align_ms'], best['entry_ms'], best['align_on_logs_ms'], best['torch_viterbi_ms'],
                 case['ratio_to_torch'], N, {k: [round(x, 4) for x in v] for k, v in runs.items()}), flush=True)
        results.append(case)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), cases=results)))


if __name__ == "__main__":
    main()
