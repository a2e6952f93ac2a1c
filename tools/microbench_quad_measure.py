"""Time of one `QuadMeasurer.measure` call (megreader_amd/structure/quad_measurer.py: host padding, five H2D copies,
mr_quad_iou + mr_quad_match, one D2H copy, the per-image dicts) at a validation batch of the DB detector's size:
N = 16 images, 16 ground truths and 100 detections each (max_candidates), the random quads of tests/_quad_eval_ref.py.
  python tools/microbench_quad_measure.py [--out FILE]
Median of 20 calls after 3 warm-up calls, each call between two device synchronisations, host clock; the two launches
alone by device events; and the float64 Python restatement of the tests on the same input beside it (one call).  The
reference's shapely path cannot be timed where shapely is not installed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _quad_eval_ref as R  # noqa: E402
from megreader_amd.ops.detection_measure import quad_measure  # noqa: E402
from megreader_amd.structure import QuadMeasurer  # noqa: E402

N, G, D, WARMUP, CALLS = 16, 16, 100, 3, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    images = [R.random_image(500 + n, G, D) for n in range(N)]
    batch = {'polygons': [np.array(g) for g, _, _ in images], 'ignore_tags': [np.array(i) for _, i, _ in images]}
    output = ([d for _, _, d in images],)
    measurer = QuadMeasurer()
    times = []
    for k in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = measurer.measure(batch, output)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times = times[WARMUP:]
    # the two launches alone, inputs already on the device
    gt = torch.tensor(np.array([g for g, _, _ in images]), device="cuda")
    det = torch.tensor(np.array([d for _, _, d in images]), device="cuda")
    ign = torch.tensor(np.array([i for _, i, _ in images]), dtype=torch.int32, device="cuda")
    gc = torch.full((N,), G, dtype=torch.int32, device="cuda")
    dc = torch.full((N,), D, dtype=torch.int32, device="cuda")
    kernel = []
    for k in range(WARMUP + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        quad_measure(gt, gc, ign, det, dc)
        e1.record()
        torch.cuda.synchronize()
        kernel.append(e0.elapsed_time(e1) * 1e3)
    kernel = kernel[WARMUP:]
    t0 = time.perf_counter()
    want = [R.evaluate_image(*im) for im in images]
    helper_ms = (time.perf_counter() - t0) * 1e3
    same = all(g[key] == w[key] for g, w in zip(got, want)
               for key in ('pairs', 'gtCare', 'detCare', 'detMatched', 'gtDontCare', 'detDontCare'))
    lines = [
        "%s; QuadMeasurer.measure, N = %d images x %d ground truths x %d detections (%d pairs)"
        % (torch.cuda.get_device_name(0), N, G, D, N * G * D),
        "  measure(), synchronised at both ends: median of %d calls %.3f ms (min %.3f, max %.3f)"
        % (CALLS, statistics.median(times), min(times), max(times)),
        "  mr_quad_iou + mr_quad_match alone, device events: median %.1f us (min %.1f, max %.1f)"
        % (statistics.median(kernel), min(kernel), max(kernel)),
        "  float64 Python restatement (tests/_quad_eval_ref.py) on the same input, one call: %.1f ms" % helper_ms,
        "  counts, pairs and don't-care lists equal to the restatement's: %s; matched %d, don't-care detections %d"
        % (same, sum(w['detMatched'] for w in want), sum(len(w['detDontCare']) for w in want)),
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
