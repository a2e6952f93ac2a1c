#!/usr/bin/env python
"""Time the split JPEG decoder (mr_jpeg_decode_split, csrc/jpeg_split.hip) on whole photos, beside the single-wave decoder and
the host decoder it stands in for.

    python tools/bench_jpeg_split.py              # one line per measurement and one JSON line at the end

Inputs (seeded, generated with PIL: nothing is downloaded), all quality 90, 4:2:0:
  photo        1280x720 without restart markers: ONE work item
  photo rst    the same pixels with restart_marker_rows=1: 45 items
  photo 640    640x360 without restart markers
  batch        8 different 1280x720 photos without restart markers
For each, with subseq_bytes in {64, 128, 256, 512} and split_above=0: the decode alone (device events round the call on a staged
batch, median [min, max] after a warm-up), the kernels of one call by name (torch.profiler, where it works), the host plan
(mr_jpeg_plan + mr_jpeg_plan_split).  Yardsticks measured in the same run: mr_jpeg_decode without splitting (one wavefront per
item) and PIL on one core.  Then `EncodedDetectionPipeline.process` against PIL + `DetectionPipeline.process` on the batch with
fixed augmentation plans, and the crossover: single-item files of growing size through both paths.
Every GPU result is checked against PIL's pixels before it is timed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_jpeg_decode import check, device_events, host_clock, median, pil_bgr  # noqa: E402
from make_jpeg_fixtures import content, encode  # noqa: E402
from megreader_amd._lib import call  # noqa: E402
from megreader_amd.data import DetectionAugmenter, DetectionPipeline, EncodedDetectionPipeline  # noqa: E402
from megreader_amd.data import jpeg_decode as jd  # noqa: E402

SIZES = (64, 128, 256, 512)


def staged(blobs, split_above=None, S=128):
    """The batch staged on the device once: (plan, launch() -> status tensor, output bytes on the device)."""
    plan = jd.make_plan(blobs)
    if split_above is not None:
        plan.split(split_above, S)
    dev = torch.device("cuda")
    blob_buf = np.zeros(plan.blob_bytes, dtype=np.uint8)
    plan.fill_blobs(blob_buf)
    parts = [np.frombuffer(s, dtype=np.uint8) for s in plan.sections()[1:3] if not isinstance(s, int)]
    d_blobs, d_plan = torch.from_numpy(blob_buf).to(dev), torch.from_numpy(np.concatenate(parts)).to(dev)
    d_split = torch.from_numpy(np.frombuffer(plan.split_table(), dtype=np.uint8).copy()).to(dev) if plan.n_splits else None
    d_ws = torch.empty((plan.workspace_bytes,), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((plan.out_bytes,), dtype=torch.uint8, device=dev)
    d_status = torch.empty((plan.n,), dtype=torch.int32, device=dev)

    def launch():
        call("mr_jpeg_decode_split", d_blobs.data_ptr(), d_plan.data_ptr(), plan.n, plan.n_items,
             plan.split_table() if plan.n_splits else None, d_split.data_ptr() if plan.n_splits else None, plan.n_splits,
             d_ws.data_ptr(), d_out.data_ptr(), d_status.data_ptr(), 0)
        return d_status
    return plan, launch, d_out


def kernels_by_name(launch, repeats):
    """{short kernel name: mean ms per call} of the kernels `launch` enqueues, or None where the profiler gives nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(repeats):
                launch()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            name = ev.key
            if "jpeg_" not in name:
                continue
            short = name[name.index("jpeg_"):].split("E")[0] if "_kernel" in name else name
            short = short[:short.index("_kernel")] if "_kernel" in short else short
            total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            out[short] = round(out.get(short, 0.0) + total / 1e3 / repeats, 4)
        return out or None
    except Exception as e:  # measurement aid only: the decode times above do not depend on it
        print("(no per-kernel times: %s)" % e, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-single-wave", action="store_true", help="do not time the 100 ms-class single-wave decodes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_split.py needs the GPU: a CPU run says nothing about it")
    result = {}

    def report(key, ms, lo, hi):
        result[key] = {"ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
        print("%-58s %9.3f ms  [%.3f, %.3f]" % (key, ms, lo, hi), flush=True)

    big = [content(1280, 720, 77 + i) for i in range(8)]
    inputs = [("photo", [encode(big[0], quality=90, subsampling=2)]),
              ("photo rst", [encode(big[0], quality=90, subsampling=2, restart_marker_rows=1)]),
              ("photo 640", [encode(content(640, 360, 78), quality=90, subsampling=2)]),
              ("batch", [encode(p, quality=90, subsampling=2) for p in big])]
    for key, blobs in inputs:
        pixels = [pil_bgr(b) for b in blobs]
        plan = jd.make_plan(blobs)
        result[key] = {"images": len(blobs), "encoded_bytes": sum(len(b) for b in blobs), "work_items": plan.n_items}
        print("%s: %d image(s), %d encoded bytes, %d work item(s)" % (key, len(blobs), result[key]["encoded_bytes"], plan.n_items),
              flush=True)
        report(key + ": PIL decode, one core", *host_clock(lambda: [pil_bgr(b) for b in blobs], max(5, args.repeats // 3), 2))
        if not args.skip_single_wave:
            plan, launch, d_out = staged(blobs)
            status = launch()
            torch.cuda.synchronize()
            check(plan, d_out, status, pixels)
            reps = args.repeats if key == "photo rst" else 5
            report(key + ": single wave per item (device events)", *device_events(launch, reps, 2))
        report(key + ": mr_jpeg_plan (host)", *host_clock(lambda: jd.make_plan(blobs), args.repeats, args.warmup))
        for S in SIZES:
            plan, launch, d_out = staged(blobs, 0, S)
            status = launch()
            torch.cuda.synchronize()
            check(plan, d_out, status, pixels)
            tag = "%s: split S=%d" % (key, S)
            report(tag + " (device events)", *device_events(launch, args.repeats, args.warmup))
            report(tag + " mr_jpeg_plan + mr_jpeg_plan_split (host)",
                   *host_clock(lambda: jd.make_plan(blobs).split(0, S), args.repeats, args.warmup))
            stages = kernels_by_name(launch, 10)
            if stages:
                result[tag + " kernels"] = stages
                print("%-58s %s" % (tag + " kernels (ms per call)", "  ".join("%s %.3f" % kv for kv in sorted(stages.items()))),
                      flush=True)

    # ---- the crossover: one item of growing length through both paths
    print("crossover: single-item files, single wave against split S=128 (decode alone, device events)", flush=True)
    cross = []
    for side in (24, 40, 64, 96, 128, 192, 256, 384):
        blob = encode(content(side, side, 900 + side), quality=90, subsampling=2)
        px = [pil_bgr(blob)]
        times = []
        for above in (None, 0):
            plan, launch, d_out = staged([blob], above, 128)
            status = launch()
            torch.cuda.synchronize()
            check(plan, d_out, status, px)
            times.append(device_events(launch, args.repeats, args.warmup)[0])
        item = int(plan.items[0].len)
        cross.append({"side": side, "item_bytes": item, "single_ms": round(times[0], 4), "split_ms": round(times[1], 4)})
        print("  %4dx%-4d item %7d bytes   single %8.3f ms   split %8.3f ms" % (side, side, item, times[0], times[1]), flush=True)
    result["crossover"] = cross

    # ---- EncodedDetectionPipeline.process against PIL + DetectionPipeline.process, the batch of 8, fixed plans
    blobs = inputs[3][1]
    pixels = [pil_bgr(b) for b in blobs]
    rng = np.random.RandomState(3)
    polys, tags = [], []
    for _ in blobs:
        x0, y0 = rng.uniform(0, 900, 6), rng.uniform(0, 500, 6)
        w, h = rng.uniform(60, 300, 6), rng.uniform(20, 120, 6)
        polys.append(np.stack([np.stack([x0, y0], 1), np.stack([x0 + w, y0], 1), np.stack([x0 + w, y0 + h], 1),
                               np.stack([x0, y0 + h], 1)], 1))
        tags.append([False] * 6)
    aug = DetectionAugmenter(size=(640, 640), seed=11)
    plans = [aug.sample(px.shape, q, t) for px, q, t in zip(pixels, polys, tags)]
    plain = DetectionPipeline()
    for S in SIZES:
        encoded = EncodedDetectionPipeline(split_above=0, subseq_bytes=S)
        a, b = encoded.process(blobs, polys, tags, plans=plans), plain.process(pixels, polys, tags, plans=plans)
        torch.cuda.synchronize()
        assert all(torch.equal(a[k], b[k]) for k in ("image", "gt", "mask", "thresh_map", "thresh_mask"))

        def run_encoded():
            encoded.process(blobs, polys, tags, plans=plans)
            torch.cuda.synchronize()

        def run_host():
            plain.process([pil_bgr(blob) for blob in blobs], polys, tags, plans=plans)
            torch.cuda.synchronize()
        enc, hst = [], []
        for _ in range(2):      # alternately, so that both see the same machine
            enc.append(host_clock(run_encoded, max(5, args.repeats // 2), 2))
            if S == SIZES[0]:
                hst.append(host_clock(run_host, max(5, args.repeats // 3), 1))
        report("batch: EncodedDetectionPipeline.process S=%d" % S, median([e[0] for e in enc]), min(e[1] for e in enc),
               max(e[2] for e in enc))
        if hst:
            report("batch: PIL + DetectionPipeline.process", median([e[0] for e in hst]), min(e[1] for e in hst),
                   max(e[2] for e in hst))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
