#!/usr/bin/env python
"""Time `ctc2d_marginal` (mr_ctc2d_marginal) on the eval output of a 2D-CTC head against a yardstick that is not the code under
test: `(classify * mask).sum(2)` in torch on the same tensors.  The two must agree to float32 rounding (the kernel's order of
summation is fixed, torch's is its own).  Times are device events in this process after warm-up; the two are measured alternately,
`--repeats` times each, and every repeat is printed (the spread is the noise).

    python tools/bench_ctc2d_read.py              # prints one line per case and one JSON line at the end

Workload (seeded: nothing is downloaded): classify [N, C, 8, 32], the softmax over the classes of noise, and mask [N, 1, 8, 32], the
softmax over the heights; N = 256, C = 38 (the BASELINE head) and N = 64, C = 6 000 (the wide alphabet), each in the two layouts
that occur: "nhwc", the project's own head (an NHWC buffer viewed as NCHW), and "nchw", a contiguous tensor.  Bytes moved are what
the algorithm needs -- classify and the mask read once, the marginal written once -- and the share of HBM bandwidth is those bytes
over the time, against the 8.0 TB/s of the MI355X's data sheet (about 6.3 TB/s is what a plain copy achieves).  The small head is
10 MB: its time is the launch, not the memory.  `ctc2d_char_rows` is timed on the same heads with 8 symbols per row, aligned by
`ctc_forced_align` to the marginal."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_lexicon import timed  # noqa: E402
from megreader_amd.ops.decode import ctc2d_char_rows, ctc2d_marginal, ctc_forced_align  # noqa: E402

CASES = [(256, 38, 8, 32), (64, 6000, 8, 32)]                                 # N, C, H, W
HBM_PEAK = 8.0e12                                                              # bytes per second, the data sheet's
SYMBOLS = 8


def make_head(gen, N, C, H, W, layout, dev):
    """(classify [N, C, H, W], mask [N, 1, H, W]) f32 on the device; the path b s0 b s1 .. of `SYMBOLS` symbols is raised so that
    the marginal aligns to it."""
    targets = torch.randint(2, C, (N, SYMBOLS), generator=gen, device=dev, dtype=torch.int64)
    logits = torch.randn((N, H, W, C), generator=gen, device=dev)
    path = torch.zeros((N, W), dtype=torch.int64, device=dev)
    path[:, 1:2 * SYMBOLS:2] = targets
    logits.scatter_add_(3, path[:, None, :, None].expand(N, H, W, 1), torch.full((N, H, W, 1), 4.0, device=dev))
    classify = torch.softmax(logits, dim=3).permute(0, 3, 1, 2)                # the NHWC buffer viewed as NCHW
    mask = torch.softmax(torch.randn((N, 1, H, W), generator=gen, device=dev), dim=2)
    if layout == "nchw":
        classify = classify.contiguous()
    assert classify.stride(1 if layout == "nhwc" else 3) == 1
    return classify, mask, targets.to(torch.int32), torch.full((N,), SYMBOLS, dtype=torch.int32, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc2d_read.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    results = []
    for N, C, H, W in CASES:
        for layout in ("nhwc", "nchw"):
            gen = torch.Generator(device=dev)
            gen.manual_seed(2026 + C)
            classify, mask, targets, lengths = make_head(gen, N, C, H, W, layout, dev)
            yardstick = lambda: (classify * mask).sum(2)                      # noqa: E731
            post = ctc2d_marginal(classify, mask)
            worst = float((post - yardstick()).abs().max())
            assert worst <= 1e-6, "N=%d C=%d %s: the marginal differs from torch by %.3g" % (N, C, layout, worst)
            align = ctc_forced_align(post, targets, lengths)
            assert bool(torch.isfinite(align['score']).all())
            rows = ctc2d_char_rows(classify, mask, targets, lengths, align)
            assert int(rows['rows'].min()) >= 0 and int(rows['row_lo'].min()) >= 0
            runs = {'marginal_ms': [], 'marginal_log_ms': [], 'torch_ms': [], 'char_rows_ms': []}
            for _ in range(args.repeats):                                      # alternately: the machine is shared
                runs['marginal_ms'].append(timed(lambda: ctc2d_marginal(classify, mask), args.warmup, args.iters)[0])
                runs['torch_ms'].append(timed(yardstick, args.warmup, args.iters)[0])
                runs['marginal_log_ms'].append(timed(lambda: ctc2d_marginal(classify, mask, log=True), args.warmup, args.iters)[0])
                runs['char_rows_ms'].append(timed(lambda: ctc2d_char_rows(classify, mask, targets, lengths, align),
                                                  args.warmup, args.iters)[0])
            best = {k: min(v) for k, v in runs.items()}
            moved = 4 * (N * C * H * W + N * H * W + N * C * W)               # classify and mask read once, the marginal written
            rate = moved / (best['marginal_ms'] * 1e-3)
            case = dict(N=N, C=C, H=H, W=W, layout=layout, max_abs_difference_to_torch=worst, bytes_moved=moved,
                        bytes_per_second=round(rate), share_of_hbm_peak=round(rate / HBM_PEAK, 4),
                        ratio_to_torch=round(best['torch_ms'] / best['marginal_ms'], 2),
                        **{k: round(best[k], 4) for k in runs}, **{k + "_runs": [round(x, 4) for x in v] for k, v in runs.items()})
            print("N=%-3d C=%-4d H=%d W=%d %s  ctc2d_marginal %.4f ms (with log %.4f)   torch (classify * mask).sum(2) %.4f ms (x%.2f)"
                  "   %.1f MB moved, %.0f GB/s = %.1f %% of the HBM peak   ctc2d_char_rows (%d symbols) %.4f ms   runs: %s"
                  % (N, C, H, W, layout, best['marginal_ms'], best['marginal_log_ms'], best['torch_ms'], case['ratio_to_torch'],
                     moved / 1e6, rate / 1e9, 100 * rate / HBM_PEAK, SYMBOLS, best['char_rows_ms'],
                     {k: [round(x, 4) for x in v] for k, v in runs.items()}), flush=True)
            results.append(case)
            del classify, mask, post
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), cases=results)))


if __name__ == "__main__":
    main()
