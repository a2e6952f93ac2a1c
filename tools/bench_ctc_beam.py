#!/usr/bin/env python
"""Time `ctc_beam_search_decode` (mr_ctc_beam_search) on recognition batches, against two things that are not the code under test:
`ctc_greedy_decode` on the same tensor -- the floor: one read of the posterior -- and the float64 numpy restatement
(tests/_ctc_beam_ref.py) on the host for a sample of rows, EXTRAPOLATED per row to the batch and labelled as such.  Device times
are device events in this process after warm-up; the host time is a host clock.

    python tools/bench_ctc_beam.py                # prints one line per case and one JSON line at the end

Workload (seeded: nothing is downloaded): 256 posteriors [N, C, 1, 32], the softmax of noise plus a path that spells a random
string of 3..12 symbols with a blank between them, over C = 37, 96 and 6 000 classes; beams of 1, 8 and 32 hypotheses over the 16
best symbols of a column, one string returned.  Per case the tool also counts, from the results of the timed calls, the rows whose
most probable string is not the greedy one, and holds the sampled rows to the restatement with the tolerance of
tests/test_ctc_beam_gpu.py (8 x e32 on the rows whose float64 margin is clear).  The two launches of a call (columns, then rows)
are not timed apart here: `rocprofv3 --kernel-trace --stats -- python tools/bench_ctc_beam.py` names them."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_lexicon import timed  # noqa: E402
from megreader_amd.ops.decode import ctc_beam_search_decode, ctc_greedy_decode  # noqa: E402


def make_posteriors(rng, N, T, C, sharp):
    """f32 [N, C, 1, T] (the eval head's layout), the f32 [N, T, C] numpy copy of it and the strings the rows spell (class ids)."""
    logits = rng.randn(N, T, C).astype(np.float32)
    texts = []
    for n in range(N):
        text = rng.randint(2, C, size=int(rng.randint(3, 13)))
        path = np.zeros(T, dtype=np.int64)
        path[1:2 * len(text):2] = text                                   # a blank between the symbols, blanks after them
        logits[n, np.arange(T), path] += sharp
        texts.append(text.tolist())
    y = torch.softmax(torch.from_numpy(logits), dim=-1)
    return y.permute(0, 2, 1).contiguous().unsqueeze(2), y.numpy(), texts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--columns", type=int, default=32)
    ap.add_argument("--classes", type=int, nargs="+", default=[37, 96, 6000])
    ap.add_argument("--beams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--top-classes", type=int, default=16)
    ap.add_argument("--sharp", type=float, default=4.0, help="what the spelled path is raised by (logits of unit noise)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sample", type=int, default=8, help="rows restated on the host per case")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_beam.py measures on the GPU; there is none")
    import _ctc_beam_ref as B
    dev = torch.device("cuda")
    N, T, top = args.rows, args.columns, args.top_classes
    results = []
    for C in args.classes:
        rng = np.random.RandomState(2025 + C)
        pred, y, _ = make_posteriors(rng, N, T, C, args.sharp)
        pred = pred.to(dev)
        lp = B.logs(y[:args.sample])
        ms_greedy, (g_ids, g_len) = timed(lambda: ctc_greedy_decode(pred), args.warmup, args.iters)
        for beam in args.beams:
            ms_beam, out = timed(lambda: ctc_beam_search_decode(pred, beam=beam, nbest=1, top_classes=top), args.warmup,
                                 args.iters)
            ids, lengths = out['ids'][:, 0], out['lengths'][:, 0]
            differs = int(((lengths != g_len) | (ids != g_ids).any(dim=1)).sum())     # both are blank padded
            t0 = time.perf_counter()
            r64 = B.decode(lp, beam, 1, top, dtype=np.float64)
            host_ms_per_row = (time.perf_counter() - t0) * 1e3 / len(lp)
            r32 = B.decode(lp, beam, 1, top, dtype=np.float32)
            e32 = max([0.0] + [abs(float(a['hyps'][0][1]) - float(b['hyps'][0][1])) for a, b in zip(r64, r32)
                               if a['hyps'] and b['hyps'] and a['hyps'][0][0] == b['hyps'][0][0]])
            ids_h, len_h, score_h = ids.cpu().numpy(), lengths.cpu().numpy(), out['scores'][:, 0].cpu().numpy()
            worst, clear = 0.0, 0
            for n, r in enumerate(r64):
                if r['margin'] > 16 * e32 and r['hyps']:
                    clear += 1
                    assert tuple(ids_h[n, :len_h[n]].tolist()) == r['hyps'][0][0], (C, beam, n)
                    worst = max(worst, abs(float(score_h[n]) - float(r['hyps'][0][1])))
            assert worst <= 8 * e32, "C=%d beam=%d: |kernel - float64| = %.3g, tolerance %.3g" % (C, beam, worst, 8 * e32)
            row = dict(classes=C, rows=N, columns=T, beam=beam, top_classes=top, beam_ms=round(ms_beam, 4),
                       greedy_ms=round(ms_greedy, 4), ratio_to_greedy=round(ms_beam / ms_greedy, 1),
                       host_restatement_ms_extrapolated=round(host_ms_per_row * N, 1), host_rows_timed=len(lp),
                       rows_differing_from_greedy=differs, sample_clear_rows=clear,
                       sample_error_in_e32=round(worst / e32, 2) if e32 > 0 else 0.0)
            print("C=%-5d B=%-3d beam search %.4f ms   greedy %.4f ms (x%.1f)   host float64 restatement %.0f ms (extrapolated "
                  "from %d rows)   top-1 differs from greedy on %d of %d rows   sample: %d clear rows within %.2f e32"
                  % (C, beam, ms_beam, ms_greedy, ms_beam / ms_greedy, host_ms_per_row * N, len(lp), differs, N, clear,
                     row['sample_error_in_e32']), flush=True)
            results.append(row)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), cases=results)))


if __name__ == "__main__":
    main()
