"""Time of the recognition augmentation (data/recognition_augment.py over csrc/rec_augment.hip) on the GPU, beside the plain
resize it replaces, beside a PIL / numpy chain on one core and beside the CRNN training step it feeds.
  python tools/bench_rec_augment.py [--out FILE]
The workload: 256 stored crops of about 40 x 150 (heights 32..48, widths 120..180) onto 32 x 128, every effect on at p = 1.
  launch    `mr_rec_augment` alone, and `mr_resize_normalize` alone on the same batch (the floor of a byte gather of this form),
            tables already on the device: 5 warm-up launches, then 7 windows of 50 back-to-back launches between two device
            events; the figure is the median window / 50 with the lowest and highest window beside it.  It is launch-to-launch
            time: where the host cannot enqueue faster than the device runs, it is the enqueue that is timed, and the kernel
            takes at most this.  Bytes moved: the source pixels once and the f32 planes once;
  whole     `DevicePipeline.process` with the augmenter and without it, ended by a device synchronisation, host clock: 3 warm-up
            calls, then the median of 15 single calls;
  plan      `RecognitionAugmenter.sample` alone for the 256 shapes, host clock, median of 15;
  PIL       per crop `Image.transform(PERSPECTIVE, BILINEAR)` onto 128 x 32, `ImageFilter.GaussianBlur`, uniform numpy noise, the
            mean and the scale, on one core, wall clock of one pass.  It leaves out the knots, the colour map, motion blur,
            pixelation and the rectangles, and resamples an already resampled image for the blur: a floor of a host chain, not
            an equal."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data import DevicePipeline, RecognitionAugmenter  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402

STEP_MS = 2.37          # README.md: the CRNN training step at 256 crops of 32 x 128, bf16
SYNTH_US = 54.0         # README.md: mr_synth_render, 256 crops of 32 x 128 (the same tile / blur / noise structure)
HBM_GBS = 8000.0        # MI355X: 8 TB/s peak
SIZE = (32, 128)


def all_on(p=1.0):
    return RecognitionAugmenter(seed=0, p=p, gray_prob=0.5, invert_prob=0.5, gaussian_sigma=(0.5, 1.2), motion_prob=0.5,
                                pixelate_prob=0.5, erase_prob=1.0, erase_count=(1, 4))


def median_ms(fn, n=15, warm=3):
    ts = []
    for k in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def host_ms(fn, n=15, warm=3):
    ts = []
    for k in range(warm + n):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def windows_us(launch):
    for _ in range(5):
        launch()
    windows = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            launch()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e3 / 50)
    return statistics.median(windows), min(windows), max(windows)


def pil_pass(images, table):
    """One core: perspective warp, Gaussian blur, noise, normalisation.  Wall clock of one pass, milliseconds."""
    from PIL import Image, ImageFilter
    H, W = SIZE
    rng = np.random.default_rng(0)
    mean = np.array(RGB_MEAN, dtype=np.float32)
    t0 = time.perf_counter()
    out = np.empty((len(images), 3, H, W), dtype=np.float32)
    for k, (im, d) in enumerate(zip(images, table)):
        g = d["g"].reshape(3, 3)
        # PIL's PERSPECTIVE takes the map output pixel -> input pixel: the resize's sampling rule, then g
        s = np.array([[d["sx"], 0.0, 0.5 * d["sx"] - 0.5], [0.0, d["sy"], 0.5 * d["sy"] - 0.5], [0.0, 0.0, 1.0]])
        m = g @ s
        m = m / m[2, 2]
        warped = Image.fromarray(im).transform((W, H), Image.PERSPECTIVE, tuple(m.reshape(9)[:8]), Image.BILINEAR)
        warped = warped.filter(ImageFilter.GaussianBlur(0.9))
        a = np.asarray(warped, dtype=np.float32) + float(d["noise_amp"]) * (rng.random((H, W, 3), dtype=np.float32) - 0.5)
        out[k] = ((np.clip(a, 0.0, 255.0) - mean) / 255.0).transpose(2, 0, 1)
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rec_augment.py measures on the GPU; there is none")
    H, W = SIZE
    n = 256
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (int(rng.randint(32, 49)), int(rng.randint(120, 181)), 3)).astype(np.uint8) for _ in range(n)]
    texts = ["word%d" % k for k in range(n)]
    src_bytes = sum(im.nbytes for im in images)
    aug = all_on()
    plain = DevicePipeline(SIZE, 'resize', EnglishCharset())
    pipe = DevicePipeline(SIZE, 'resize', EnglishCharset(), augmenter=aug)
    lines = ["%s; %d stored crops (%d source bytes) onto %d x %d, every effect on, p = 1" % (torch.cuda.get_device_name(0), n,
                                                                                            src_bytes, H, W)]
    # the kernels alone, on the buffer one upload left on the device
    staged, layout = pipe.pack(images, texts, index=0)
    dbuf = pipe.upload(staged, layout)['_keepalive']
    torch.cuda.synchronize()
    desc_off = layout[1]
    _, M, table_off, aug_off, rows = layout[-1]
    image = torch.empty((n, 3, H, W), dtype=torch.float32, device=pipe.device)
    resize = windows_us(lambda: call("mr_resize_normalize", ptr(dbuf), dbuf.data_ptr() + desc_off, n, H, W, RGB_MEAN[0],
                                     RGB_MEAN[1], RGB_MEAN[2], ptr(image)))
    augment = windows_us(lambda: call("mr_rec_augment", ptr(dbuf), dbuf.data_ptr() + table_off, n, dbuf.data_ptr() + aug_off, M,
                                      n, H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(image)))
    moved = src_bytes + n * 3 * H * W * 4 + M * 560
    lines += ["launch to launch, at most the kernel, median (min, max) of 7 windows of 50:",
              "  mr_resize_normalize  %.1f us (%.1f, %.1f)" % resize,
              "  mr_rec_augment       %.1f us (%.1f, %.1f), %d descriptors = %.2f x the resize, %.2f x mr_synth_render's %.0f us"
              % (augment + (M, augment[0] / resize[0], augment[0] / SYNTH_US, SYNTH_US)),
              "  bytes moved %d (source once, f32 planes once, descriptors) = %.1f GB/s = %.2f %% of %.0f GB/s HBM"
              % (moved, moved / augment[0] / 1e3, 100.0 * moved / augment[0] / 1e3 / HBM_GBS, HBM_GBS)]
    # the whole call
    whole_plain = median_ms(lambda: plain.process(images, texts))
    whole_aug = median_ms(lambda: pipe.process(images, texts))
    shapes = [im.shape for im in images]
    planning = host_ms(lambda: aug.sample(shapes, SIZE, 'resize', 0))
    lines += ["DevicePipeline.process, median (min, max) of 15 single calls, host clock with a synchronisation:",
              "  without the augmenter %.3f ms (%.3f, %.3f)" % whole_plain,
              "  with the augmenter    %.3f ms (%.3f, %.3f) = %.2f x" % (whole_aug + (whole_aug[0] / whole_plain[0],)),
              "  planning alone (RecognitionAugmenter.sample, host) %.3f ms (%.3f, %.3f)" % planning,
              "  beside the CRNN step of %.2f ms (README) that Prefetcher overlaps it with: whole call %.0f %%, planning %.0f %%%s"
              % (STEP_MS, 100 * whole_aug[0] / STEP_MS, 100 * planning[0] / STEP_MS,
                 "" if whole_aug[0] < STEP_MS else "  -- the call EXCEEDS the step: the input side would bound the training")]
    table, _ = aug.sample(shapes, SIZE, 'resize', 0)
    pil_ms, _ = pil_pass(images, table)
    lines.append("PIL + numpy on one core, warp + Gaussian blur + noise + normalisation of the same crops: %.1f ms = %.0f crops/s"
                 " = %.0f x the whole call" % (pil_ms, n / pil_ms * 1e3, pil_ms / whole_aug[0]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
