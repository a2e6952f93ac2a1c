"""Time of `SegDetectorRepresenter.represent` on the host-geometry path (two host synchronisations with Python geometry between
them) against `device_geometry=True` (`mr_db_boxes`, one copy), in the same process and on the same inputs.
  python tools/microbench_db_post.py [--out FILE]
Shapes: oracle.db_post.synthetic_maps(3, N=4, H=576, W=1024, regions=60) -- TextReader's det_size -- and (3, N=2, 640 x 640,
regions=60).  Per shape:
  (a) / (b) wall clock (time.perf_counter) around the whole `represent` call, device idle on entry, including every copy and the
      list building: 3 warm-up calls each, then 25 calls of the two paths ALTERNATING; median, min, max;
  (c) `boxes_on_device` alone between two device events: 5 warm-up calls, 7 windows of 20 back-to-back calls, median window / 20;
and whether the two paths returned identical lists, the number of components and of boxes."""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from megreader_amd.structure import SegDetectorRepresenter  # noqa: E402
from oracle import db_post as O  # noqa: E402

CASES = [(4, 576, 1024), (2, 640, 640)]
CALLS, WARM = 25, 3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = [torch.cuda.get_device_name(0)]
    ok = True
    for N, H, W in CASES:
        maps = O.synthetic_maps(3, N=N, H=H, W=W, regions=60)
        pred = {'binary': torch.from_numpy(maps).cuda().unsqueeze(1)}
        batch = {'image': None, 'shape': [(720, 1280)] * N}
        host = SegDetectorRepresenter(resize=True)
        dev = SegDetectorRepresenter(resize=True, device_geometry=True)
        for _ in range(WARM):
            host.represent(batch, pred)
            dev.represent(batch, pred)
        t_host, t_dev = [], []
        for _ in range(CALLS):
            ms, a = wall(lambda: host.represent(batch, pred)[0])
            t_host.append(ms)
            ms, b = wall(lambda: dev.represent(batch, pred)[0])
            t_dev.append(ms)
        same = a == b
        ok = ok and same
        for _ in range(5):
            found = dev.boxes_on_device(pred['binary'], None, batch['shape'])
        per_call = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(20):
                found = dev.boxes_on_device(pred['binary'], None, batch['shape'])
            e1.record()
            torch.cuda.synchronize()
            per_call.append(e0.elapsed_time(e1) / 20)
        lines.append("N = %d, %d x %d: %s components, %s boxes per image; identical lists: %s"
                     % (N, H, W, found['components'].tolist(), [len(x) for x in b], same))
        lines.append("  (a) represent, host geometry:        median %.3f ms (min %.3f, max %.3f) of %d calls, wall clock"
                     % (statistics.median(t_host), min(t_host), max(t_host), CALLS))
        lines.append("  (b) represent, device_geometry=True: median %.3f ms (min %.3f, max %.3f) of %d calls, wall clock"
                     % (statistics.median(t_dev), min(t_dev), max(t_dev), CALLS))
        lines.append("  (c) boxes_on_device alone:           median %.3f ms per call (min %.3f, max %.3f) of 7 windows of 20, "
                     "device events" % (statistics.median(per_call), min(per_call), max(per_call)))
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
