#!/usr/bin/env python
"""Time the GPU JPEG decoder (mr_jpeg_decode, `EncodedDevicePipeline`) beside the host decoder it replaces.

    python tools/bench_jpeg_decode.py             # one line per measurement and one JSON line at the end

Workload (seeded, generated with PIL: nothing is downloaded):
  crops   256 recognition crops of 100x32, quality 75, 4:2:0
            - mr_jpeg_decode alone: device events around the call on a staged batch, median of --repeats after warm-up
            - EncodedDevicePipeline.process end to end (host plan + staging + one copy + decode + resize + labels), host clock
              around calls that end in a synchronise
            - the same for DevicePipeline.process fed with the pixels already decoded (what the host path does AFTER PIL)
            - PIL decode of the same blobs on one core (the host path's decode), host clock
  photo   one 1280x720 quality-90 4:2:0 photo with restart_marker_rows=1 (45 work items) and without restart markers (one
          work item: ONE wavefront decodes the whole image), mr_jpeg_decode alone, beside PIL on one core
Every GPU result is checked against PIL's pixels before it is timed."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_jpeg_fixtures import content, encode  # noqa: E402
from megreader_amd._lib import call  # noqa: E402
from megreader_amd.data import DevicePipeline, EncodedDevicePipeline  # noqa: E402
from megreader_amd.data import jpeg_decode as jd  # noqa: E402


def median(xs):
    return float(np.median(np.asarray(xs)))


def pil_bgr(blob):
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(io.BytesIO(blob)).convert('RGB'))[:, :, ::-1])


def host_clock(fn, repeats, warmup):
    """Median and spread (min, max) in ms of fn(), which must end synchronised."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return median(times), min(times), max(times)


def staged_decode(blobs):
    """The batch staged on the device once: (plan, launch() -> status tensor, output bytes on the device)."""
    plan = jd.make_plan(blobs)
    dev = torch.device("cuda")
    blob_buf = np.zeros(plan.blob_bytes, dtype=np.uint8)
    plan.fill_blobs(blob_buf)
    table = np.concatenate([np.frombuffer(s, dtype=np.uint8) for s in plan.sections()[1:] if not isinstance(s, int)])
    d_blobs, d_plan = torch.from_numpy(blob_buf).to(dev), torch.from_numpy(table.copy()).to(dev)
    d_ws = torch.empty((plan.workspace_bytes,), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((plan.out_bytes,), dtype=torch.uint8, device=dev)
    d_status = torch.empty((plan.n,), dtype=torch.int32, device=dev)

    def launch():
        call("mr_jpeg_decode", d_blobs.data_ptr(), d_plan.data_ptr(), plan.n, plan.n_items, d_ws.data_ptr(), d_out.data_ptr(),
             d_status.data_ptr(), 0)
        return d_status
    return plan, launch, d_out


def device_events(launch, repeats, warmup):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return median(times), min(times), max(times)


def check(plan, d_out, status, pixels):
    assert status.tolist() == [jd.OK] * plan.n, status.tolist()
    out = d_out.cpu().numpy()
    for im, px in zip(plan.images, pixels):
        assert np.array_equal(out[im.out_off:im.out_off + px.size].reshape(px.shape), px), "GPU decode differs from PIL"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--crops", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode.py needs the GPU: a CPU run says nothing about it")
    result = {}

    def report(key, ms, lo, hi, per=None, unit="images"):
        result[key] = {"ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
        rate = ""
        if per:
            result[key]["per_s"] = round(per / ms * 1e3, 1)
            rate = "  %10.0f %s/s" % (per / ms * 1e3, unit)
        print("%-44s %9.3f ms  [%.3f, %.3f]%s" % (key, ms, lo, hi, rate), flush=True)

    # ---- recognition crops
    n = args.crops
    blobs = [encode(content(100, 32, 5000 + i), quality=75, subsampling=2) for i in range(n)]
    texts = ["word%d" % (i % 97) for i in range(n)]
    pixels = [pil_bgr(b) for b in blobs]
    result["crops"] = {"n": n, "encoded_bytes": sum(len(b) for b in blobs), "decoded_bytes": sum(p.size for p in pixels)}
    print("crops: %d x 100x32 q75 4:2:0, %d encoded bytes, %d decoded bytes" % (n, result["crops"]["encoded_bytes"],
                                                                              result["crops"]["decoded_bytes"]), flush=True)
    plan, launch, d_out = staged_decode(blobs)
    status = launch()
    torch.cuda.synchronize()
    check(plan, d_out, status, pixels)
    report("crops: mr_jpeg_decode (device events)", *device_events(launch, args.repeats, args.warmup), per=n)
    report("crops: PIL decode, one core", *host_clock(lambda: [pil_bgr(b) for b in blobs], max(3, args.repeats // 6), 1), per=n)
    report("crops: mr_jpeg_plan (host)", *host_clock(lambda: jd.make_plan(blobs), args.repeats, args.warmup), per=n)
    encoded = EncodedDevicePipeline(image_size=(32, 100))
    plain = DevicePipeline(image_size=(32, 100))
    a, b = encoded.process(blobs, texts), plain.process(pixels, texts)
    torch.cuda.synchronize()
    assert torch.equal(a['image'], b['image']) and torch.equal(a['label'], b['label'])

    def run_encoded():
        encoded.process(blobs, texts)
        torch.cuda.synchronize()

    def run_plain():
        plain.process(pixels, texts)
        torch.cuda.synchronize()
    # alternately, so that both see the same machine
    enc, pla = [], []
    for _ in range(3):
        enc.append(host_clock(run_encoded, args.repeats, args.warmup))
        pla.append(host_clock(run_plain, args.repeats, args.warmup))
    report("crops: EncodedDevicePipeline.process", median([e[0] for e in enc]), min(e[1] for e in enc), max(e[2] for e in enc), per=n)
    report("crops: DevicePipeline.process (decoded)", median([p[0] for p in pla]), min(p[1] for p in pla), max(p[2] for p in pla), per=n)

    # ---- one photo, with and without restart markers
    photo = content(1280, 720, 77)
    for key, options in (("photo rst rows", dict(restart_marker_rows=1)), ("photo no rst", {})):
        blob = encode(photo, quality=90, subsampling=2, **options)
        px = pil_bgr(blob)
        plan, launch, d_out = staged_decode([blob])
        status = launch()
        torch.cuda.synchronize()
        check(plan, d_out, status, [px])
        result[key] = {"encoded_bytes": len(blob), "work_items": plan.n_items}
        print("%s: 1280x720 q90 4:2:0, %d bytes, %d work items" % (key, len(blob), plan.n_items), flush=True)
        reps = args.repeats if plan.n_items > 1 else max(3, args.repeats // 6)
        report(key + ": mr_jpeg_decode (device events)", *device_events(launch, reps, 2))
        report(key + ": PIL decode, one core", *host_clock(lambda: pil_bgr(blob), args.repeats, 2))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
