"""Time of `QuadCropper.crop` (data/quad_crop.py over csrc/image_sample.hip) for 256 crops at 32 x 128 out of ONE resident
720 x 1280 photo, next to the two-pass numpy restatement of the reference's `ImageCropper.crop` on the host for the same crops.
  python tools/microbench_quad_crop.py [--out FILE]
Three figures.  (a) the whole call -- planning on the host, one staging copy of the tables, the launch -- between two device
events with a synchronisation in front, so host time in which the device waits is counted: 3 warm-up calls, then the median of 9
single calls.  (b) the launch alone, tables already on the device: 5 warm-up launches, then 7 windows of 50 back-to-back launches
between two device events; the figure is the median window / 50.  (c) `two_pass_ref` of tests/_quad_crop_ref.py, one crop after
the other, wall clock of one pass over all crops (it is pure numpy: this is the restated arithmetic, not cv2's speed).
Beside them: whether crop 0 equals the kernel's numpy restatement bit for bit, and the deviation of the fused pass from the
two-pass chain over all crops (max and mean, normalised units) on the random photo and on a smooth one."""
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
import _quad_crop_ref as R  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.data import QuadCropper  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402

CANVAS, SRC, M = (32, 128), (720, 1280), 256


def boxes(rng):
    out = []
    for _ in range(M):
        a, b, t = rng.uniform(60, 300), rng.uniform(20, 60), np.radians(rng.uniform(-30, 30))
        c, s = np.cos(t), np.sin(t)
        base = np.array([[-a / 2, -b / 2], [a / 2, -b / 2], [a / 2, b / 2], [-a / 2, b / 2]])
        out.append(base @ np.array([[c, s], [-s, c]]) + [rng.uniform(100, 1180), rng.uniform(80, 640)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    photo = rng.randint(0, 256, SRC + (3,)).astype(np.uint8)
    quads = boxes(rng)
    resident = torch.from_numpy(photo).cuda()
    cropper = QuadCropper(image_size=CANVAS)
    lines = ["%s; %d crops at %d x %d from one resident %d x %d photo" % (torch.cuda.get_device_name(0), M, CANVAS[0], CANVAS[1],
                                                                         SRC[1], SRC[0])]
    # (a) the whole call
    whole = []
    for k in range(3 + 9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = cropper.crop([resident], [quads])
        e1.record()
        torch.cuda.synchronize()
        if k >= 3:
            whole.append(e0.elapsed_time(e1))
    lines.append("  (a) QuadCropper.crop, plan + tables + launch: median %.2f ms per call (min %.2f, max %.2f) of 9"
                 % (statistics.median(whole), min(whole), max(whole)))
    # (b) the launch alone
    staged, layout = cropper.pack([resident], [quads])
    kept = cropper.upload(staged, layout)
    dbuf = kept['_keepalive'][0]
    image = torch.empty((M, 3) + CANVAS, dtype=torch.float32, device="cuda")

    def once():
        call("mr_quad_crop", ptr(dbuf), dbuf.data_ptr() + layout.table_off, layout.I, dbuf.data_ptr() + layout.desc_off, M,
             CANVAS[0], CANVAS[1], RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(image))

    for _ in range(5):
        once()
    per_call = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            once()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / 50)
    lines.append("  (b) mr_quad_crop alone: median %.1f us per launch (min %.1f, max %.1f) of 7 windows of 50 = %.3f us per crop"
                 % (statistics.median(per_call), min(per_call), max(per_call), statistics.median(per_call) / M))
    # (c) the two-pass restatement on the host, and the deviation
    got = out['image'].cpu().numpy()
    t0 = time.perf_counter()
    two = [R.two_pass_ref(photo, plan, 'resize') for plan in layout.plans]
    host_s = time.perf_counter() - t0
    lines.append("  (c) two-pass numpy restatement on the host, %d crops: %.1f ms (wall clock, one pass)" % (M, host_s * 1e3))
    dev = np.abs(got - np.stack(two))
    lines.append("  fused pass against the two-pass chain over all crops (random pixels): max %.4f mean %.4f (normalised units)"
                 % (dev.max(), dev.mean()))
    # the same on a smooth photo (a few sinusoids, periods of 40 to 300 pixels): noise is the worst case for a second resampling
    yy, xx = np.mgrid[0:SRC[0], 0:SRC[1]].astype(np.float64)
    wave = 127.5 + 60 * np.sin(xx / 47.0) * np.cos(yy / 31.0) + 40 * np.sin((xx + 2 * yy) / 9.0) + 27 * np.cos(yy / 6.5)
    smooth = np.repeat(np.clip(np.rint(wave), 0, 255).astype(np.uint8)[..., None], 3, axis=2)
    fused = cropper.crop([smooth], [quads])['image'].cpu().numpy()
    dev = np.abs(fused - np.stack([R.two_pass_ref(smooth, plan, 'resize') for plan in layout.plans]))
    lines.append("  fused pass against the two-pass chain over all crops (smooth photo): max %.4f mean %.4f (normalised units)"
                 % (dev.max(), dev.mean()))
    same = np.array_equal(got[0].view(np.uint32), R.quad_crop_ref(photo, layout.plans[0]).view(np.uint32))
    lines.append("  crop 0 equal to the restatement bit for bit: %s" % same)
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
