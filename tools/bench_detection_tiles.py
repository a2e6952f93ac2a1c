"""Times of tiled multi-scale detection (data/detection_tiles.py over csrc/det_tiles.hip) for ONE resident 2160 x 3840 photo with
tiles of 576 x 1024 and a halo of 64, in two plans: scales=('fit', 0.5), and scales=(1.0,) within max_canvas=(2176, 3840).
  python tools/bench_detection_tiles.py [--out FILE]
Per plan, all between device events, warm (as tools/microbench_quad_crop.py does):
  (a) mr_tile_sample alone, tables already on the device: 5 warm-up launches, then 7 windows of 20 back-to-back launches; the
      figure is the median window / 20, with the bytes the pass must move (the uint8 photo once per level, plus every f32
      tile element written) and their rate as a share of the 8.0 TB/s HBM peak;
  (b) mr_tile_stitch alone, f32 maps, likewise: every map element of every level read once, every fused pixel written once;
  (c) `DetectionTiler.detect` as a whole with a pointwise stub detector (sigmoid of channel 0): plan, staging of the tables,
      sample, the stub in chunks of 8 tiles, stitch -- 3 warm-up calls, then the median of 9 single calls with a
      synchronisation in front;
  (d) the yardstick: the same fused map composed from torch operations on the same resident tensors -- per level the whole-canvas
      resize (mr_resize_normalize, one launch), the stub on it, `F.interpolate(mode='bilinear', align_corners=False)` onto the
      base level and `torch.maximum` -- which is also what slicing tiles out of the whole canvas and pasting their cores back
      amounts to for a pointwise detector.  Median of 9 single calls.  Its result is compared with (c): exactly equal for the
      one-level plan, and the largest difference for the two-level plan (F.interpolate rounds differently from mr_tile_stitch).
Bytes are counted from shapes; cache hits on the re-read overlap make the achieved DRAM traffic smaller than a per-tile count
would say, so the share of peak is that of the least traffic, not of what the lanes request."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from megreader_amd._lib import call, dtype_code, ptr  # noqa: E402
from megreader_amd.data import DetectionTiler, DevicePipeline  # noqa: E402
from megreader_amd.data.detection_tiles import FUSE_CODES  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.data.quad_crop import CropImage  # noqa: E402

SRC, TILE, HALO = (2160, 3840), (576, 1024), (64, 64)
HBM_PEAK = 8.0e12
PLANS = [("scales=('fit', 0.5)", dict(scales=('fit', 0.5))), ("scales=(1.0,), max_canvas=(2176, 3840)",
                                                               dict(scales=(1.0,), max_canvas=(2176, 3840)))]


def stub(x):
    return torch.sigmoid(x[:, :1])


def on_device(table):
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()


def windows(once, n=20, warm=5, reps=7):
    """Median, min, max microseconds per launch over `reps` windows of `n` back-to-back launches."""
    for _ in range(warm):
        once()
    per = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            once()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / n)
    return statistics.median(per), min(per), max(per)


def singles(once, warm=3, reps=9):
    """Median, min, max milliseconds of single calls with a synchronisation in front; the last result."""
    times, out = [], None
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = once()
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            times.append(e0.elapsed_time(e1))
    return (statistics.median(times), min(times), max(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_detection_tiles.py measures on the GPU; there is none")
    photo = np.random.RandomState(0).randint(0, 256, SRC + (3,)).astype(np.uint8)
    resident = torch.from_numpy(photo).cuda()
    lines = ["%s; one resident %d x %d photo, tiles %d x %d, halo %d" % (torch.cuda.get_device_name(0), SRC[1], SRC[0], TILE[1],
                                                                        TILE[0], HALO[0])]
    ok = True
    for name, kw in PLANS:
        tiler = DetectionTiler(tile=TILE, halo=HALO, **kw)
        plan = tiler.plan([SRC])
        th, tw = TILE
        canvases = [lv.canvas for lv in plan.levels[0]]
        lines.append("%s: %d tiles, canvases %s, fused map %d x %d" % (name, plan.T, canvases, plan.sizes[0][1], plan.sizes[0][0]))
        # (a) the sampling launch alone
        table = (CropImage * 1)()
        table[0].offset, table[0].pitch, table[0].h, table[0].w = 0, SRC[1] * 3, SRC[0], SRC[1]
        table_d, descs_d = on_device(table), on_device(plan.tile_descs())
        tiles = torch.empty((plan.T, 3, th, tw), dtype=torch.float32, device="cuda")
        t = windows(lambda: call("mr_tile_sample", ptr(resident), ptr(table_d), 1, ptr(descs_d), plan.T, th, tw, RGB_MEAN[0],
                                 RGB_MEAN[1], RGB_MEAN[2], ptr(tiles)))
        moved = len(canvases) * photo.nbytes + tiles.numel() * 4
        lines.append("  (a) mr_tile_sample alone: median %.1f us per launch (min %.1f, max %.1f) of 7 windows of 20; %.1f MB at "
                     "least = %.2f TB/s = %.0f %% of the HBM peak" % (t + (moved / 1e6, moved / t[0] / 1e6, 100 * moved / (t[0] * 1e-6) / HBM_PEAK)))
        # (b) the stitching launch alone
        maps = stub(tiles).contiguous()
        levels, photos, max_pixels = plan.stitch_tables()
        levels_d, photos_d = on_device(levels), on_device(photos)
        fused = torch.empty((plan.total,), dtype=torch.float32, device="cuda")
        t = windows(lambda: call("mr_tile_stitch", dtype_code(maps.dtype), ptr(maps), plan.T, th, tw, HALO[0], HALO[1], ptr(levels_d),
                                 len(levels), ptr(photos_d), 1, max_pixels, FUSE_CODES['max'], ptr(fused), plan.total))
        moved = sum(h * w for h, w in canvases) * 4 + plan.total * 4
        lines.append("  (b) mr_tile_stitch alone: median %.1f us per launch (min %.1f, max %.1f) of 7 windows of 20; %.1f MB at "
                     "least = %.2f TB/s = %.0f %% of the HBM peak" % (t + (moved / 1e6, moved / t[0] / 1e6, 100 * moved / (t[0] * 1e-6) / HBM_PEAK)))
        # (c) detect as a whole
        t, got = singles(lambda: tiler.detect(stub, [resident], batch=8)[0])
        lines.append("  (c) DetectionTiler.detect, pointwise stub, chunks of 8: median %.2f ms per call (min %.2f, max %.2f) of 9" % t)
        # (d) the same map from torch operations on whole canvases
        wholes = []                                  # per level: the photo and its descriptor on the device, and the canvas
        for canvas in canvases:
            pipe = DevicePipeline(image_size=canvas, mode='resize')
            staged, layout = pipe.pack([photo], [''])
            wholes.append((pipe.upload(staged, layout)['_keepalive'], layout[1], canvas))

        def yardstick():
            out = None
            for dbuf, desc_off, canvas in wholes:
                whole = torch.empty((1, 3) + canvas, dtype=torch.float32, device="cuda")
                call("mr_resize_normalize", ptr(dbuf), dbuf.data_ptr() + desc_off, 1, canvas[0], canvas[1], RGB_MEAN[0],
                     RGB_MEAN[1], RGB_MEAN[2], ptr(whole))
                level = stub(whole)
                if canvas != plan.sizes[0]:
                    level = torch.nn.functional.interpolate(level, size=plan.sizes[0], mode='bilinear', align_corners=False)
                out = level if out is None else torch.maximum(out, level)
            return out
        t, want = singles(yardstick)
        lines.append("  (d) the same map from torch operations on whole canvases: median %.2f ms per call (min %.2f, max %.2f) of 9" % t)
        diff = (got - want).abs().max().item()
        lines.append("      largest difference between (c) and (d): %.3g" % diff)
        if len(canvases) == 1:
            ok = ok and diff == 0.0
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
