"""Time of one `mr_warp_normalize` call (csrc/image_sample.hip) at the DB detector's training size: a 640 x 640 canvas from
1280 x 720 photos, N = 2 (the batch of bench.py's DB workload) and N = 16, for plans at scale 0.5, 1 and 3 with +-10 degrees
and a flip, and for the identity plan (640 x 640 sources) next to `mr_resize_normalize` at identity on the same canvas.
  python tools/microbench_db_augment.py [--out FILE]
The crop of every plan is 640 x 640 of the resized photo (all of it where it is smaller), placed in its middle.  Inputs are on
the device: the figure is the kernel alone, without the plan (host) and the copy.  Per configuration: 5 warm-up calls, then 7
windows of 50 back-to-back calls between two device events; the figure is the median window / 50 (min and max beside it).
Beside it: the bytes of the uploaded windows against the whole photos, and whether image 0 equals the numpy restatement of
the tests (tests/_db_augment_ref.py) bit for bit."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _db_augment_ref as R  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.data import DetectionAugmenter, WarpDesc  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN, ImgDesc  # noqa: E402

S, SRC, WARMUP, WINDOWS, CALLS = 640, (720, 1280), 5, 7, 50


def timed(once):
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
    return statistics.median(per_call), min(per_call), max(per_call)


def middle(resized, side=S):
    nh, nw = resized
    cw, ch = min(side, nw), min(side, nh)
    return (nw - cw) // 2, (nh - ch) // 2, cw, ch


def upload(images, plans):
    """The windows back to back (16-byte aligned) and their descriptors, on the device."""
    descs = (WarpDesc * len(plans))()
    off = 0
    for d, plan in zip(descs, plans):
        plan.fill(d, off)
        off += (plan.window[2] * plan.window[3] * 3 + 15) // 16 * 16
    host = np.zeros(max(off, 16), dtype=np.uint8)
    for d, plan, im in zip(descs, plans, images):
        x, y, w, h = plan.window
        host[d.offset:d.offset + h * w * 3] = im[y:y + h, x:x + w].reshape(-1)
    dev = torch.device("cuda")
    return torch.from_numpy(host).to(dev), torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev), off


def time_warp(name, n, shape, params, lines):
    rng = np.random.RandomState(n)
    images = [rng.randint(0, 256, shape + (3,)).astype(np.uint8) for _ in range(n)]
    aug = DetectionAugmenter(size=(S, S))
    plans = []
    for i in range(n):
        flip, angle, scale = params[i % len(params)]
        resized = DetectionAugmenter.stages(shape, flip, angle, scale)[2]
        plans.append(aug.plan(shape, flip=flip, angle=angle, scale=scale, crop=middle(resized)))
    d_src, d_desc, nbytes = upload(images, plans)
    out = torch.empty((n, 3, S, S), dtype=torch.float32, device="cuda")

    def once():
        call("mr_warp_normalize", ptr(d_src), ptr(d_desc), n, S, S, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(out))

    med, lo, hi = timed(once)
    same = np.array_equal(out[0].cpu().numpy().view(np.uint32), R.warp_normalize_ref(images[0], plans[0])['image'].view(np.uint32))
    lines.append("  %-34s N = %2d: median %.1f us per call (min %.1f, max %.1f) = %.1f us per image; windows %.2f MB of %.2f MB; "
                 "image 0 equal to the restatement: %s" % (name, n, med, lo, hi, med / n, nbytes / 1e6,
                                                           n * shape[0] * shape[1] * 3 / 1e6, same))
    return med, same, images


def time_resize(n, images, lines):
    descs = (ImgDesc * n)()
    for i, d in enumerate(descs):
        d.offset, d.h, d.w, d.pitch, d.dst_w, d.scale_x, d.scale_y = i * S * S * 3, S, S, S * 3, S, 1.0, 1.0
    dev = torch.device("cuda")
    d_src = torch.from_numpy(np.stack(images).reshape(-1)).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)

    def once():
        call("mr_resize_normalize", ptr(d_src), ptr(d_desc), n, S, S, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(out))

    med, lo, hi = timed(once)
    lines.append("  %-34s N = %2d: median %.1f us per call (min %.1f, max %.1f) = %.1f us per image"
                 % ("mr_resize_normalize at identity", n, med, lo, hi, med / n))
    return med, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert ctypes.sizeof(WarpDesc) == 128
    lines = ["%s; mr_warp_normalize onto %d x %d from %d x %d photos, median of %d windows of %d calls, device events"
             % (torch.cuda.get_device_name(0), S, S, SRC[1], SRC[0], WINDOWS, CALLS)]
    ok = True
    for n in (2, 16):
        for name, params in (("scale 0.5, +-10 deg, flip", [(True, 10.0, 0.5), (False, -10.0, 0.5)]),
                             ("scale 1, +-10 deg, flip", [(True, 10.0, 1.0), (False, -10.0, 1.0)]),
                             ("scale 3, +-10 deg, flip", [(True, 10.0, 3.0), (False, -10.0, 3.0)])):
            _, same, _ = time_warp(name, n, SRC, params, lines)
            ok = ok and same
        warp, same, images = time_warp("identity plan (640 x 640 sources)", n, (S, S), [(False, 0.0, 1.0)], lines)
        resize, _ = time_resize(n, images, lines)
        lines.append("  identity plan / mr_resize_normalize at identity, N = %d: %.2f" % (n, warp / resize))
        ok = ok and same
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
