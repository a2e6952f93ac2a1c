"""Times of curved reading: the two device stages behind `TextReader(curved=True)` against the stages they stand beside, and the
reader as a whole.
  python tools/bench_curved_read.py [--out FILE]
All between device events, warm (as tools/bench_detection_tiles.py does): 5 warm-up launches, then 7 windows of 20 back-to-back
launches, the figure is the median window / 20.
  (a) mr_db_boxes alone (the yardstick) and mr_db_boxes + mr_db_ribbons on the same maps: N = 4 maps of 576 x 1024 with 48 painted
      components each (arches, tilted bars, short bars), K = 100, S = 8; the difference is what the ribbons cost;
  (b) mr_quad_crop (the yardstick) and mr_strip_crop for 256 crops onto 32 x 128 from four resident 576 x 1024 photos: the same
      boxes as two-knot strips, and 12-knot arches of the same size.  Both kernels write the same bytes and read the same taps, so
      a large gap would point at the per-column work not being hoisted;
  (c) `TextReader.read` of the four photos with a pointwise stub detector and a stub recogniser, curved=False and curved=True:
      3 warm-up calls, then the median of 9 single calls with a synchronisation in front."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from megreader_amd import TextReader  # noqa: E402
from megreader_amd._lib import call, load, ptr  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.data.quad_crop import CropDesc, CropImage, plan_crop  # noqa: E402
from megreader_amd.data.strip_crop import StripDesc, plan_strip  # noqa: E402
from megreader_amd.structure import Ribbon, SegDetectorRepresenter  # noqa: E402

N, H, W, K, S = 4, 576, 1024, 100, 8


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
        per.append(e0.elapsed_time(e1) * 1000.0 / n)
    return {'median_us': statistics.median(per), 'min_us': min(per), 'max_us': max(per)}


def single_calls(once, warm=3, reps=9):
    for _ in range(warm):
        once()
    per = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        once()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1))
    return {'median_ms': statistics.median(per), 'min_ms': min(per), 'max_ms': max(per)}


def arch(centre, radius, half, span, knots):
    angles = np.radians(np.linspace(-span / 2.0, span / 2.0, knots))
    top = [(centre[0] + (radius + half) * math.sin(a), centre[1] - (radius + half) * math.cos(a)) for a in angles]
    bot = [(centre[0] + (radius - half) * math.sin(a), centre[1] - (radius - half) * math.cos(a)) for a in angles]
    return Ribbon(top, bot)


def scene(seed):
    """A 576 x 1024 mask of 48 components on an 8 x 6 grid of 128 x 96 cells: arches, tilted bars and short bars in turn."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    mask = np.zeros((H, W), bool)
    for k in range(48):
        cx, cy = 64.0 + 128.0 * (k % 8), 48.0 + 96.0 * (k // 8)
        if k % 3 == 0:
            dx, dy = xx - cx, yy - (cy + 50.0)
            r = np.sqrt(dx * dx + dy * dy)
            mask |= (np.abs(r - 70.0) <= 6.0) & (np.abs(np.degrees(np.arctan2(dx, -dy))) <= 40.0)
        else:
            t = math.radians(float(g.uniform(-20.0, 20.0)))
            u = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
            v = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
            mask |= (np.abs(u) <= (50.0 if k % 3 == 1 else 16.0)) & (np.abs(v) <= 7.0)
    return mask


def on_device(table):
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()


def bench_ribbons(masks):
    maps = torch.from_numpy(np.stack(masks).astype(np.float32) * np.float32(0.9)).cuda()
    nbytes, rbytes = ctypes.c_longlong(0), ctypes.c_longlong(0)
    assert load().mr_db_boxes_ws_bytes(N, H, W, K, ctypes.byref(nbytes)) == 0
    assert load().mr_db_ribbons_ws_bytes(N, K, ctypes.byref(rbytes)) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    rws = torch.empty(rbytes.value, dtype=torch.uint8, device="cuda")
    boxes = torch.empty((N, K, 4, 2), dtype=torch.float64, device="cuda")
    scores = torch.empty((N, K), dtype=torch.float32, device="cuda")
    count, comps = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
    ribbons = torch.empty((N, K, 18, 2, 2), dtype=torch.float64, device="cuda")
    knots, why = torch.empty((N, K), dtype=torch.int32, device="cuda"), torch.empty((N, K), dtype=torch.int32, device="cuda")
    dest = torch.tensor([(W, H)] * N, dtype=torch.int32, device="cuda")

    def run_boxes():
        call("mr_db_boxes", ptr(maps), ptr(maps), 0.3, ptr(dest), N, H, W, K, 0.2, 3.0, ptr(ws), ptr(boxes), ptr(scores),
             ptr(count), ptr(comps), 0, 0, 0)

    def run_both():
        run_boxes()
        call("mr_db_ribbons", ptr(dest), N, H, W, K, S, 1.5, ptr(ws), ptr(rws), ptr(ribbons), ptr(knots), ptr(why))

    def run_ribbons():
        call("mr_db_ribbons", ptr(dest), N, H, W, K, S, 1.5, ptr(ws), ptr(rws), ptr(ribbons), ptr(knots), ptr(why))

    out = {'mr_db_boxes': windows(run_boxes), 'mr_db_boxes + mr_db_ribbons': windows(run_both)}
    run_boxes()
    out['mr_db_ribbons on a finished workspace'] = windows(run_ribbons)
    torch.cuda.synchronize()
    out['components'], out['boxes'] = comps.tolist(), count.tolist()
    out['ribbons'] = [int((knots[n, :int(count[n])] > 0).sum()) for n in range(N)]
    return out


def bench_crops(photos):
    M, canvas = 256, (32, 128)
    table = (CropImage * N)()
    flat = torch.cat([p.reshape(-1) for p in photos])
    for i in range(N):
        table[i].offset, table[i].pitch, table[i].h, table[i].w = i * H * W * 3, W * 3, H, W
    quads, arches = [], []
    for m in range(M):
        cx, cy = 80.0 + (m % 16) * 56.0, 60.0 + (m // 16 % 16) * 30.0
        quads.append([[cx - 60.0, cy - 12.0], [cx + 60.0, cy - 12.0], [cx + 60.0, cy + 12.0], [cx - 60.0, cy + 12.0]])
        arches.append(arch((cx, cy + 70.0), 70.0, 12.0, 100.0, 12))
    qd, sd2, sd12 = (CropDesc * M)(), (StripDesc * M)(), (StripDesc * M)()
    for m in range(M):
        plan_crop((H, W), quads[m], canvas, 'resize').fill(qd[m], m % N)
        plan_strip((H, W), Ribbon.from_box(quads[m]), canvas, 'resize').fill(sd2[m], m % N)
        plan_strip((H, W), arches[m], canvas, 'resize').fill(sd12[m], m % N)
    d_table, d_q, d_s2, d_s12 = on_device(table), on_device(qd), on_device(sd2), on_device(sd12)
    a = torch.empty((M, 3) + canvas, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)

    def crop(name, desc, dst):
        return lambda: call(name, ptr(flat), ptr(d_table), N, ptr(desc), M, canvas[0], canvas[1], RGB_MEAN[0], RGB_MEAN[1],
                            RGB_MEAN[2], ptr(dst))
    out = {'mr_quad_crop, 256 boxes': windows(crop("mr_quad_crop", d_q, a)),
           'mr_strip_crop, the same boxes as two-knot strips': windows(crop("mr_strip_crop", d_s2, b)),
           'mr_strip_crop, 256 arches of 12 knots': windows(crop("mr_strip_crop", d_s12, b))}
    crop("mr_strip_crop", d_s2, b)()
    torch.cuda.synchronize()
    out['largest difference between the box crops'] = float((a - b).abs().max())
    out['bytes written'] = int(a.numel() * 4)
    return out


def bench_reader(masks):
    charset = EnglishCharset()
    photos = [np.repeat((m.astype(np.uint8) * 255)[:, :, None], 3, axis=2) for m in masks]

    def detector(x):
        return {'binary': (x[:, :1] > 0).float()}

    class Stub(torch.nn.Module):
        def forward(self, crops):
            out = torch.zeros((crops.shape[0], len(charset), 1, 16), dtype=torch.float32, device=crops.device)
            out[:, 0] = 1.0
            return out

    out = {}
    for curved in (False, True):
        reader = TextReader(detector, Stub(), charset, det_size=(H, W), rec_size=(32, 128), curved=curved,
                            representer=SegDetectorRepresenter(resize=True, box_thresh=0.2, device_geometry=True))
        found = reader.read(photos)
        out['curved=%s' % curved] = dict(single_calls(lambda: reader.read(photos)), crops=sum(len(f) for f in found))
        if curved:
            out['curved=True']['ribbons'] = sum(len(item['polygon']) > 4 for f in found for item in f)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    masks = [scene(seed) for seed in range(N)]
    photos = [torch.from_numpy(np.repeat((m.astype(np.uint8) * 255)[:, :, None], 3, axis=2).copy()).cuda() for m in masks]
    result = {'device': torch.cuda.get_device_name(0), 'ribbons': bench_ribbons(masks), 'crops': bench_crops(photos),
              'reader': bench_reader(masks)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
