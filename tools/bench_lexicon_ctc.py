#!/usr/bin/env python
"""Time `Lexicon.transcribe` (mr_lexicon_transcribe) on the lexicon sizes the recognition benchmarks use, against the only way to
get the same scores from stock operators: `torch.nn.functional.ctc_loss(reduction='none')` on the same GPU over the expanded list
of (row, word) pairs -- the row's log-probabilities replicated once per pair -- in chunks that fit memory, plus an arg-max.  Both
are timed with device events in this process, after warm-up, and their results are asserted equal within the tolerance of
tests/test_lexicon_ctc_gpu.py: 8 x e32, e32 the largest difference between the float32 and the float64 numpy restatement
(tests/_lexicon_ctc_ref.py) on a sample of the workload.

    python tools/bench_lexicon_ctc.py             # prints one line per case and one JSON line at the end

Workload (seeded: nothing is downloaded): N = 256 posteriors [N, 38, 1, 32] of EnglishCharset, the softmax of noise plus a path
that spells a lexicon word with two symbols changed (even rows) or a random string (odd rows); words of 3..15 symbols.  Cases: 256
per-row lexicons of 50 words (`Lexicon.grouped`) and 1 000 shared words, every word scored; 90 000 words within 2 and within 3
edits of the greedy string, and 90 000 words all scored.  For the two bounded cases the yardstick is handed the candidate pairs
(it has no distance filter of its own) and is charged for their ctc_loss and arg-max only."""
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
from bench_lexicon import ALPHABET, make_words, timed  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.ops.lexicon import Lexicon  # noqa: E402


def make_posteriors(rng, charset, words, N, T, sharp=6.0):
    """f32 [N, C, 1, T] (the eval head's layout) and the f32 [N, T, C] numpy copy of it."""
    C = len(charset)
    letters = list(ALPHABET)
    logits = rng.randn(N, T, C)
    for n in range(N):
        if n % 2 == 0:
            text = list(words[int(rng.randint(len(words)))])
            for _ in range(2):
                text[int(rng.randint(len(text)))] = letters[int(rng.randint(36))]
        else:
            text = [letters[int(rng.randint(36))] for _ in range(int(rng.randint(3, 16)))]
        path = [0] * T
        path[1:2 * len(text):2] = [charset.index(ch) for ch in text]        # a blank between the symbols, blanks after them
        logits[n, np.arange(T), path] += sharp
    y = torch.softmax(torch.from_numpy(logits.astype(np.float32)), dim=-1)
    return y.permute(0, 2, 1).contiguous().unsqueeze(2), y.numpy()


def ctc_scores(logp, rows, wordmat, lens, words):
    """-ctc_loss of the pairs (rows[i], words[i]): logp f32 [T, N, C] log-probabilities, replicated once per pair."""
    T = logp.shape[0]
    loss = torch.nn.functional.ctc_loss(logp[:, rows, :], wordmat[words], torch.full_like(rows, T), lens[words], blank=0,
                                        reduction='none')
    return -loss


def yardstick_all(logp, wordmat, lens, spans, chunk_pairs):
    """(index i64 [N], score f32 [N]) over every word of the span (None: the whole lexicon), lowest index among equal scores."""
    N, L = logp.shape[1], wordmat.shape[0]
    dev = logp.device
    best = torch.full((N,), -float('inf'), device=dev)
    index = torch.full((N,), -1, dtype=torch.long, device=dev)
    rows_all = torch.arange(N, device=dev)
    if spans is not None:
        per = L // N
        words = torch.arange(L, device=dev)
        s = ctc_scores(logp, rows_all.repeat_interleave(per), wordmat, lens, words).view(N, per)
        best, k = s.max(dim=1)
        return torch.where(torch.isfinite(best), k + rows_all * per, index), best
    step = max(1, chunk_pairs // N)
    for c0 in range(0, L, step):
        c1 = min(L, c0 + step)
        words = torch.arange(c0, c1, device=dev).repeat(N)
        s = ctc_scores(logp, rows_all.repeat_interleave(c1 - c0), wordmat, lens, words).view(N, c1 - c0)
        top, k = s.max(dim=1)                                              # the first maximum of the chunk
        better = top > best                                                # strict: an earlier chunk keeps a tie
        best = torch.where(better, top, best)
        index = torch.where(better, k + c0, index)
    return index, best


def yardstick_pairs(logp, wordmat, lens, rows, words, chunk_pairs):
    """The same over a given list of candidate pairs sorted by (row, word)."""
    N = logp.shape[1]
    dev = logp.device
    scores = torch.cat([ctc_scores(logp, rows[c0:c0 + chunk_pairs], wordmat, lens, words[c0:c0 + chunk_pairs])
                        for c0 in range(0, max(1, len(rows)), chunk_pairs)]) if len(rows) else torch.zeros(0, device=dev)
    best = torch.full((N,), -float('inf'), device=dev).scatter_reduce(0, rows, scores, 'amax')
    at = torch.where(scores == best[rows], words, torch.full_like(words, wordmat.shape[0]))
    index = torch.full((N,), wordmat.shape[0], dtype=torch.long, device=dev).scatter_reduce(0, rows, at, 'amin')
    return torch.where(torch.isfinite(best), index, torch.full_like(index, -1)), best


def run_case(name, lexicon, spans, delta, pred, tol, args, results):
    dev = pred.device
    N = pred.shape[0]
    lens_np = np.diff(lexicon.off).astype(np.int64)
    mat = np.zeros((len(lexicon), max(1, int(lens_np.max()))), dtype=np.int64)
    mat[np.arange(mat.shape[1])[None, :] < lens_np[:, None]] = lexicon.sym
    wordmat, lens = torch.from_numpy(mat).to(dev), torch.from_numpy(lens_np).to(dev)
    d_spans = None if spans is None else spans.to(dev)
    logp = pred.select(2, 0).permute(2, 0, 1).log().contiguous()           # [T, N, C]: what ctc_loss takes
    ms_new, found = timed(lambda: lexicon.transcribe(pred, d_spans, max_distance=delta), args.warmup, args.iters)
    candidates = int(found['candidates'].sum())
    if delta is None:
        ms_old, (index, score) = timed(lambda: yardstick_all(logp, wordmat, lens, d_spans, args.chunk_pairs), 1,
                                       args.yardstick_iters)
    else:
        table = lexicon.transcribe(pred, d_spans, max_distance=delta, all_scores=True)['scores']
        rows, words = torch.nonzero(torch.isfinite(table), as_tuple=True)  # (3..15 symbols always fit 32 columns: finite = candidate)
        assert len(rows) == candidates
        del table
        ms_old, (index, score) = timed(lambda: yardstick_pairs(logp, wordmat, lens, rows, words, args.chunk_pairs), 1,
                                       args.yardstick_iters)
    got_i, got_s = found['index'].long(), found['score']
    assert torch.equal(got_i < 0, index < 0), name
    hit = got_i >= 0
    worst = float((got_s[hit] - score[hit]).abs().max()) if hit.any() else 0.0
    same = int((got_i == index).sum())
    row = dict(case=name, rows=N, words=len(lexicon), max_distance=delta, candidates=candidates,
               transcribe_ms=round(ms_new, 4), ctc_loss_ms=round(ms_old, 3), ratio=round(ms_old / ms_new, 1),
               pairs_per_s=float("%.4g" % (candidates / (ms_new * 1e-3))), max_score_difference=float("%.3g" % worst),
               rows_same_word=same)
    print("%-16s %9d candidates   transcribe %.4f ms   ctc_loss pairs + arg-max %.3f ms   x%.1f   |score diff| <= %.2g, %d of %d "
          "rows the same word" % (name, candidates, ms_new, ms_old, ms_old / ms_new, worst, same, N), flush=True)
    assert worst <= tol, "%s: scores differ by %.3g, tolerance %.3g" % (name, worst, tol)
    assert same >= N - N // 10, "%s: only %d of %d rows agree on the word" % (name, same, N)   # the rest: a top-two gap within rounding
    results.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--full", type=int, default=90000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--yardstick-iters", type=int, default=1)
    ap.add_argument("--chunk-pairs", type=int, default=1 << 16, help="pairs per ctc_loss call (4.9 KB of log-probabilities each)")
    ap.add_argument("--sample", type=int, default=500, help="words of the full lexicon compared with the numpy restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lexicon_ctc.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    charset = EnglishCharset()
    rng = np.random.RandomState(2025)
    full_words = make_words(rng, args.full)
    pred, y = make_posteriors(rng, charset, full_words, args.rows, 32)
    pred = pred.to(dev)

    import _lexicon_ctc_ref as Q
    pick = sorted(rng.choice(len(full_words), size=min(args.sample, len(full_words)), replace=False).tolist())
    sample = Lexicon([full_words[i] for i in pick], charset)
    words = [sample.sym[sample.off[l]:sample.off[l + 1]].tolist() for l in range(len(sample))]
    S64 = Q.score_table(Q.log_probs(y, np.float64), words)
    S32 = Q.score_table(Q.log_probs(y, np.float32), words, dtype=np.float32)
    e32 = float(np.abs(S32.astype(np.float64) - S64).max())
    tol = 8.0 * e32
    got = sample.transcribe(pred, all_scores=True)['scores'].cpu().numpy().astype(np.float64)
    worst = float(np.abs(got - S64).max())
    assert worst <= tol, "sample of %d words: |kernel - float64| = %.3g, tolerance %.3g" % (len(pick), worst, tol)
    print("%d x %d sample: e32 = %.3g, |kernel - float64 restatement| <= %.3g (%.2f e32)" %
          (args.rows, len(pick), e32, worst, worst / e32), flush=True)

    results = []
    groups = [[full_words[int(i)] for i in rng.randint(len(full_words), size=50)] for _ in range(args.rows)]
    grouped, spans = Lexicon.grouped(groups, charset)
    run_case("per_row_50", grouped, spans, None, pred, tol, args, results)
    run_case("set_1000", Lexicon(full_words[:1000], charset), None, None, pred, tol, args, results)
    full = Lexicon(full_words, charset)
    run_case("full_%d_d2" % args.full, full, None, 2, pred, tol, args, results)
    run_case("full_%d_d3" % args.full, full, None, 3, pred, tol, args, results)
    run_case("full_%d_all" % args.full, full, None, None, pred, tol, args, results)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), e32=e32, sample_checked=[args.rows, len(pick)],
                          sample_error_in_e32=round(worst / e32, 2), cases=results)))


if __name__ == "__main__":
    main()
