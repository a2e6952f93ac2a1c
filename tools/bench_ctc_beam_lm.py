#!/usr/bin/env python
"""Time `ctc_beam_search_decode(lm=...)` (mr_ctc_beam_search_lm) on recognition batches against the same call with lm=None
(mr_ctc_beam_search) on the same tensor: what the model lookups of the row stage cost.  The two calls launch the same column
kernel, so their difference is the row stage's alone; it is printed per column.  Device times are device events in this process
after warm-up, the two calls timed in turn within one process.

    python tools/bench_ctc_beam_lm.py             # prints one line per case and one JSON line at the end

Workload (seeded: nothing is downloaded): 256 posteriors [N, C, 1, 32], the softmax of noise plus a path that spells a random
string of 3..12 symbols with a blank between them (tools/bench_ctc_beam.py's), over C = 37 and 6 000 classes; beams of 1, 8 and 32
hypotheses over the 16 best symbols of a column, one string returned; character models of order 3 and 5 trained on the strings the
rows spell (`CharNgramLM.train`), so that the extensions along a row's path find long n-grams and the others back off to the
unigrams.  Per case the tool also holds a sample of rows to the float64 restatement (tests/_ctc_beam_ref.py, with a model) with the tolerance
of tests/test_ctc_beam_lm_gpu.py.  The two kernels of a call are not timed apart here:
`rocprofv3 --kernel-trace --stats -- python tools/bench_ctc_beam_lm.py --iters 20` names them."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_ctc_beam import make_posteriors  # noqa: E402
from bench_lexicon import timed  # noqa: E402
from megreader_amd.charsets import Charset  # noqa: E402
from megreader_amd.ops.decode import ctc_beam_search_decode  # noqa: E402
from megreader_amd.ops.language_model import CharNgramLM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--columns", type=int, default=32)
    ap.add_argument("--classes", type=int, nargs="+", default=[37, 6000])
    ap.add_argument("--beams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--orders", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--top-classes", type=int, default=16)
    ap.add_argument("--sharp", type=float, default=4.0, help="what the spelled path is raised by (logits of unit noise)")
    ap.add_argument("--lm-weight", type=float, default=0.8)
    ap.add_argument("--lm-bonus", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sample", type=int, default=4, help="rows restated on the host per case")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_beam_lm.py measures on the GPU; there is none")
    import _ctc_beam_ref as B
    import _ngram_lm_ref as R
    dev = torch.device("cuda")
    N, T, top = args.rows, args.columns, args.top_classes
    weights = (args.lm_weight, args.lm_bonus, True)
    results = []
    for C in args.classes:
        rng = np.random.RandomState(2025 + C)
        pred, y, texts = make_posteriors(rng, N, T, C, args.sharp)
        pred = pred.to(dev)
        lp = B.logs(y[:args.sample])
        charset = Charset([chr(0x4e00 + i) for i in range(C - 2)], case_sensitive=True)
        words = ["".join(charset[c] for c in text) for text in texts]
        for order in args.orders:
            lm = CharNgramLM.train(words, charset, order=order)
            image = lm.image(C)
            model = R.DictLM(lm.ngrams, lm.order, lm.eligible(C))
            for beam in args.beams:
                kw = dict(beam=beam, nbest=1, top_classes=top)
                ms_plain, _ = timed(lambda: ctc_beam_search_decode(pred, **kw), args.warmup, args.iters)
                ms_lm, out = timed(lambda: ctc_beam_search_decode(pred, lm=lm, lm_weight=weights[0], lm_bonus=weights[1], **kw),
                                   args.warmup, args.iters)
                r64 = B.decode(lp, beam, 1, top, 0, 1, np.float64, model, *weights)
                r32 = B.decode(lp, beam, 1, top, 0, 1, np.float32, model, *weights)
                e32 = max([0.0] + [abs(float(a['hyps'][0][1]) - float(b['hyps'][0][1])) for a, b in zip(r64, r32)
                                   if a['hyps'] and b['hyps'] and a['hyps'][0][0] == b['hyps'][0][0]])
                ids_h, len_h = out['ids'][:, 0].cpu().numpy(), out['lengths'][:, 0].cpu().numpy()
                score_h = out['scores'][:, 0].cpu().numpy()
                worst, clear = 0.0, 0
                for n, r in enumerate(r64):
                    if r['margin'] > 16 * e32 and r['hyps']:
                        clear += 1
                        assert tuple(ids_h[n, :len_h[n]].tolist()) == r['hyps'][0][0], (C, order, beam, n)
                        worst = max(worst, abs(float(score_h[n]) - float(r['hyps'][0][1])))
                assert worst <= 8 * e32, "C=%d order=%d beam=%d: |kernel - float64| = %.3g, tolerance %.3g" \
                    % (C, order, beam, worst, 8 * e32)
                spelled = sum(tuple(ids_h[n, :len_h[n]].tolist()) == tuple(texts[n]) for n in range(N))
                row = dict(classes=C, rows=N, columns=T, beam=beam, top_classes=top, order=order, states=image['states'],
                           slots=image['slots'], max_probe=image['max_probe'], lm_ms=round(ms_lm, 4), plain_ms=round(ms_plain, 4),
                           ratio=round(ms_lm / ms_plain, 2), added_us_per_column=round((ms_lm - ms_plain) * 1e3 / T, 2),
                           rows_spelled=spelled, sample_clear_rows=clear,
                           sample_error_in_e32=round(worst / e32, 2) if e32 > 0 else 0.0)
                print("C=%-5d order %d (%d states, %d slots, max_probe %d) B=%-3d with the model %.4f ms   without %.4f ms (x%.2f)"
                      "   the row stage gains %.2f us per column   %d of %d rows read as spelled   sample: %d clear rows within "
                      "%.2f e32" % (C, order, image['states'], image['slots'], image['max_probe'], beam, ms_lm, ms_plain,
                                    ms_lm / ms_plain, row['added_us_per_column'], spelled, N, clear, row['sample_error_in_e32']),
                      flush=True)
                results.append(row)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), cases=results)))


if __name__ == "__main__":
    main()
