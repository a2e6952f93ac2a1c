"""Time of one `PolygonMeasurer.measure` call (megreader_amd/structure/polygon_measurer.py: host padding, seven H2D copies,
mr_poly_iou + mr_quad_match, one D2H copy, the per-image dicts) and of the two launches alone at a validation batch of curved
text: N = 16 images, 100 ground truths and 100 detections each, every word the outline of a ribbon on an arc
(tests/_poly_eval_ref.py `random_ribbon`) scattered over a 2048 x 2048 photo, the detections the ground truths with jittered
vertices.  Two vertex counts: 14 (CTW1500's annotations) and 36 (a full ribbon outline).
  python tools/bench_polygon_measure.py [--out FILE]
Beside them, on the same words: `quad_measure` on each word's axis-aligned box (the path quads take, and the yardstick of what the
extra vertices cost), the float64 Python restatement on the host (one call), and the share of
the N * G * D pairs whose boxes overlap -- the only ones that are clipped.  Median of 20 calls after 3 warm-up calls; measure()
between two device synchronisations by the host clock, the launches by device events."""
import argparse
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _poly_eval_ref as P  # noqa: E402
from megreader_amd.ops.detection_measure import polygon_measure, quad_measure  # noqa: E402
from megreader_amd.structure import PolygonMeasurer  # noqa: E402

N, G, D, WARMUP, CALLS = 16, 100, 100, 3, 20
KEYS = ('pairs', 'gtCare', 'detCare', 'detMatched', 'gtDontCare', 'detDontCare')


def words(seed, rulings):
    """(gts, ignores, dets) of one image: G ribbon outlines of 2 * rulings points and their jittered copies."""
    rng = random.Random(seed)
    gts, dets = [], []
    for _ in range(G):
        gts.append(P.random_ribbon(rng, rng.uniform(150, 1898), rng.uniform(150, 1898), rng.uniform(30, 100), rulings))
    for g in rng.sample(range(G), D):
        cx, cy = sum(v[0] for v in gts[g]) / len(gts[g]), sum(v[1] for v in gts[g]) / len(gts[g])
        size = max(math.hypot(v[0] - cx, v[1] - cy) for v in gts[g])
        while True:
            jitter = rng.uniform(0.0, 0.08) * size
            q = [(x + rng.uniform(-jitter, jitter), y + rng.uniform(-jitter, jitter)) for x, y in gts[g]]
            if P.poly_valid(q):
                break
        dets.append(q)
    return gts, [rng.random() < 0.1 for _ in gts], dets


def boxes_of(polys):
    a = np.array(polys)                                                   # [K, V, 2]
    lo, hi = a.min(axis=1), a.max(axis=1)
    return np.stack([lo, np.stack([hi[:, 0], lo[:, 1]], 1), hi, np.stack([lo[:, 0], hi[:, 1]], 1)], axis=1)


def timed(fn):
    """(median, min, max) in microseconds of CALLS calls of fn() by device events, after WARMUP calls."""
    times = []
    for _ in range(WARMUP + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times = times[WARMUP:]
    return statistics.median(times), min(times), max(times)


def bench(rulings):
    images = [words(700 + n, rulings) for n in range(N)]
    V = 2 * rulings
    # per image a list of float64 arrays [V, 2], as a data loader and `outlines_of` give them
    batch = {'polygons': [[np.array(q) for q in g] for g, _, _ in images], 'ignore_tags': [np.array(i) for _, i, _ in images]}
    output = ([[np.array(q) for q in d] for _, _, d in images],)
    measurer = PolygonMeasurer()
    times = []
    for _ in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = measurer.measure(batch, output)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times = times[WARMUP:]
    gt = torch.tensor(np.array([g for g, _, _ in images]), device="cuda")
    det = torch.tensor(np.array([d for _, _, d in images]), device="cuda")
    ign = torch.tensor(np.array([i for _, i, _ in images]), dtype=torch.int32, device="cuda")
    gv = torch.full((N, G), V, dtype=torch.int32, device="cuda")
    dv = torch.full((N, D), V, dtype=torch.int32, device="cuda")
    gc = torch.full((N,), G, dtype=torch.int32, device="cuda")
    dc = torch.full((N,), D, dtype=torch.int32, device="cuda")
    poly_us = timed(lambda: polygon_measure(gt, gv, gc, ign, det, dv, dc))
    gbox = torch.tensor(np.array([boxes_of(g) for g, _, _ in images]), device="cuda")
    dbox = torch.tensor(np.array([boxes_of(d) for _, _, d in images]), device="cuda")
    quad_us = timed(lambda: quad_measure(gbox, gc, ign, dbox, dc))
    # the pairs whose boxes overlap: what mr_poly_iou clips
    glo, ghi = gbox.cpu().numpy()[:, :, 0], gbox.cpu().numpy()[:, :, 2]
    dlo, dhi = dbox.cpu().numpy()[:, :, 0], dbox.cpu().numpy()[:, :, 2]
    live = ((glo[:, :, None, :] <= dhi[:, None, :, :]) & (dlo[:, None, :, :] <= ghi[:, :, None, :])).all(axis=3)
    t0 = time.perf_counter()
    want = [P.evaluate_image(*im) for im in images]
    helper_s = time.perf_counter() - t0
    same = all(g[key] == w[key] for g, w in zip(got, want) for key in KEYS)
    return [
        "  %d vertices per polygon (ribbons of %d rulings)" % (V, rulings),
        "    PolygonMeasurer.measure(), synchronised at both ends: median of %d calls %.3f ms (min %.3f, max %.3f)"
        % (CALLS, statistics.median(times), min(times), max(times)),
        "    mr_poly_iou + mr_quad_match alone, device events: median %.1f us (min %.1f, max %.1f)" % poly_us,
        "    mr_quad_iou + mr_quad_match on the same words' boxes: median %.1f us (min %.1f, max %.1f)" % quad_us,
        "    pairs whose boxes overlap (clipped): %d of %d = %.2f %%" % (live.sum(), live.size, 100.0 * live.sum() / live.size),
        "    float64 Python restatement (tests/_poly_eval_ref.py) on the same input, one call: %.1f s" % helper_s,
        "    counts, pairs and don't-care lists equal to the restatement's: %s; matched %d of %d in the batch"
        % (same, sum(g['detMatched'] for g in got), sum(g['gtCare'] for g in got)),
    ], same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = ["%s; N = %d images x %d ground truths x %d detections (%d pairs)" % (torch.cuda.get_device_name(0), N, G, D, N * G * D)]
    ok = True
    for rulings in (7, 18):
        part, same = bench(rulings)
        lines += part
        ok = ok and same
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
