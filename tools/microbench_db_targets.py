"""Time of one `mr_db_targets` call (csrc/db_targets.hip: the prep kernel and the fused map kernel) at the DB detector's
training size: 640 x 640 images, N = 16 with 12, 64 and 256 quads per image, and N = 2 with 12 quads per image (the batch
and the density of bench.py's DB workload, synthetic.detection_batch).
  python tools/microbench_db_targets.py [--out FILE]
The quads are the rectangles of synthetic.detection_batch (40..200 x 12..48) turned by up to 30 degrees; one in ten is
pre-tagged ignore.  Inputs are on the device.  Per configuration: 5 warm-up calls, then 7 windows of 50 back-to-back calls
between two device events; the figure is the median window / 50 (min and max beside it).  Beside the device time, the host
time of the numpy float64 restatement of the tests (tests/_db_targets_ref.py) for ONE image -- the restatement, not the
reference's cv2 / pyclipper / shapely path, which cannot run where those libraries are not installed."""
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
import _db_targets_ref as R  # noqa: E402
from megreader_amd._lib import call, load, ptr  # noqa: E402

S, WARMUP, WINDOWS, CALLS = 640, 5, 7, 50


def quads(rng, n, g):
    w, h = rng.uniform(40, 200, (n, g)), rng.uniform(12, 48, (n, g))
    cx, cy = rng.uniform(0, S, (n, g)), rng.uniform(0, S, (n, g))
    th = rng.uniform(-np.pi / 6, np.pi / 6, (n, g))
    c, s = np.cos(th), np.sin(th)
    pts = np.empty((n, g, 4, 2))
    for k, (sx, sy) in enumerate(((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5))):
        pts[:, :, k, 0] = cx + c * sx * w - s * sy * h
        pts[:, :, k, 1] = cy + s * sx * w + c * sy * h
    return pts, (rng.rand(n, g) < 0.1).astype(np.int32)


def time_config(n, g, lines):
    dev = torch.device("cuda")
    polys, tags = quads(np.random.RandomState(1000 + g), n, g)
    d_polys, d_tags = torch.from_numpy(polys).to(dev), torch.from_numpy(tags).to(dev)
    d_count = torch.full((n,), g, dtype=torch.int32, device=dev)
    records = torch.empty((n * g * load().mr_sizeof_db_record(),), dtype=torch.uint8, device=dev)
    ignore = torch.empty((n, g), dtype=torch.int32, device=dev)
    dist = torch.empty((n, g), dtype=torch.float64, device=dev)
    maps = [torch.empty((n, S, S), dtype=torch.float32, device=dev) for _ in range(4)]

    def once():
        call("mr_db_targets", ptr(d_polys), ptr(d_count), ptr(d_tags), n, g, S, S, 8.0, 0.4, 0.3, 0.7, ptr(records), ptr(ignore),
             ptr(dist), ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(maps[3]))

    for _ in range(WARMUP):
        once()
    per_call = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(CALLS):
            once()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    t0 = time.perf_counter()
    ref = R.db_targets_ref(polys[:1], [g], tags[:1], S, S)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = [m[0].cpu().numpy() for m in maps]
    skip = ref['skip']
    same = (np.array_equal(ignore[0].cpu().numpy(), ref['ignore_out'][0])
            and all(((a == b[0].reshape(a.shape)) | s[0]).all() for a, b, s in
                    ((got[0], ref['gt'], skip['gt']), (got[1], ref['mask'], skip['mask']), (got[3], ref['thresh_mask'], skip['thresh_mask'])))
            and float(np.abs(got[2] - ref['thresh_map'][0]).max()) <= 2e-7)
    med = statistics.median(per_call)
    lines.append("  N = %2d x %3d quads: median %.1f us per call (min %.1f, max %.1f) = %.1f us per image; kept %d of %d in image 0; "
                 "restatement, one image on the host: %.1f ms; image 0 equal to the restatement: %s"
                 % (n, g, med, min(per_call), max(per_call), med / n, int((ref['ignore_out'][0] == 0).sum()), g, host_ms, same))
    return med, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = ["%s; mr_db_targets at %d x %d, median of %d windows of %d calls, device events" % (torch.cuda.get_device_name(0), S, S, WINDOWS, CALLS)]
    ok = True
    for n, g in ((16, 12), (16, 64), (16, 256), (2, 12)):
        _, same = time_config(n, g, lines)
        ok = ok and same
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
