"""Time of the synthetic-text generator (data/synth_text.py over csrc/synth_text.hip) on the GPU, beside PIL drawing and warping
the same words on one core and beside the CRNN training step it feeds (README: 2.37 ms at 256 crops).
  python tools/bench_synth_text.py [--out FILE]
Three workloads: `SynthText.batch(256)` at 32 x 128 and at 32 x 100, and `SynthScenes.batch(8)` at 640 x 640 with 12 words.
For each:
  whole     the call -- planning on the host, one pinned staging copy of the tables, the launch -- ended by a device
            synchronisation, host clock: 3 warm-up calls, then the median of 15 single calls;
  plan      the host planning alone (`plan()`), host clock, median of 15;
  copy      the staging copy alone: the tables (for the crops with the labels and lengths, as `batch` stages them) into the pinned
            buffer and the async H2D copy, between two device events with a synchronisation in front, median of 15;
  launch    `mr_synth_render` alone, tables already on the device: 5 warm-up launches, then 7 windows of 50 back-to-back launches
            between two device events; the figure is the median window / 50, with the lowest and highest window beside it.  It
            is launch-to-launch time: every launch goes through ctypes and the entry point's checks, so where the host cannot
            enqueue faster than the device runs it is the enqueue that is timed.  The kernel takes at most this; its own time
            needs a kernel trace in a run of its own, which this tool does not make;
  PIL       the same words of the same plan drawn with `ImageDraw.text` on a line image and warped onto the canvas with
            `Image.transform(PERSPECTIVE, BILINEAR)`, alpha-composited over a flat ground, on one core, wall clock of one pass.  It
            leaves out shadow, gradient, blur and noise: it is the floor of a host renderer, not an equal.
Needs PIL with FreeType for the atlas of Pillow's built-in font (the words are legible; the kernel does not care)."""
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
from megreader_amd.data import GlyphAtlas, SynthScenes, SynthText  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.data.staging import Sections, upload  # noqa: E402

STEP_MS = 2.37          # README.md: the CRNN training step at 256 crops of 32 x 128, bf16
WORDS = ["the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "MI355X", "gfx950", "reader", "2024", "synthetic",
         "text", "wavefront", "kernel", "a", "of", "recognition", "detector"]


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


def event_ms(fn, n=15, warm=3):
    ts = []
    for k in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def launch_us(renderer, items, canvases, H, W, u8, f32):
    """Launch to launch: median, lowest and highest of 7 windows of 50 launches, microseconds per launch."""
    lay = Sections([items, canvases], pad_end=True)
    staged, _ = renderer._staging.stage(0, lay)
    dbuf = upload(staged, renderer.device)
    n = len(canvases)
    out_u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=renderer.device) if u8 else None
    out_f32 = torch.empty((n, 3, H, W), dtype=torch.float32, device=renderer.device) if f32 else None
    base = renderer.resident.data_ptr()

    def launch():
        call("mr_synth_render", base, base + renderer.fonts_off, len(renderer.atlases), base + renderer.pairs_off,
             renderer.n_pairs, dbuf.data_ptr() + lay.offsets[0], len(items), dbuf.data_ptr() + lay.offsets[1], n, H, W,
             RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(out_u8), ptr(out_f32))
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


def pil_pass(texts, quads, canvases_of, H, W, n_canvases, size):
    """One core: draw every word on a line image, warp it onto its canvas, composite.  Wall clock of one pass, milliseconds."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default(size=size)
    t0 = time.perf_counter()
    grounds = [Image.new("RGB", (W, H), (90, 60, 30)) for _ in range(n_canvases)]
    for text, quad, c in zip(texts, quads, canvases_of):
        left, top, right, bottom = font.getbbox(text.upper())
        lw, lh = max(right, 1), max(bottom, 1)
        line = Image.new("L", (lw, lh), 0)
        ImageDraw.Draw(line).text((0, 0), text.upper(), fill=255, font=font)
        # PIL's PERSPECTIVE takes the map output -> input: the canvas -> line homography through the four corners
        A, b = [], []
        for (x, y), (u, v) in zip(quad, [(0, 0), (lw, 0), (lw, lh), (0, lh)]):
            A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
            b += [u, v]
        coef = np.linalg.solve(np.array(A, dtype=np.float64), np.array(b, dtype=np.float64))
        mask = line.transform((W, H), Image.PERSPECTIVE, tuple(coef), Image.BILINEAR)
        grounds[c].paste((250, 240, 230), (0, 0), mask)
    out = np.stack([np.asarray(g) for g in grounds])
    return (time.perf_counter() - t0) * 1e3, out


def bench(name, gen, n, H, W, u8, f32, scene):
    gen.batch(n)                                            # builds the renderer
    plan = gen.plan(n, 0)
    items, canvases, quads = plan[0], plan[1], plan[2]
    texts = [t for ts in plan[3] for t in ts] if scene else plan[3]
    whole = median_ms(lambda: gen.batch(n, index=0))
    planning = median_ms(lambda: gen.plan(n, 0))
    extra = [] if scene else [np.zeros((n, gen.max_size), dtype=np.int32), np.zeros(n, dtype=np.int32)]   # label, length
    lay = Sections([items, canvases] + extra, pad_end=True)
    copy = event_ms(lambda: upload(gen._renderer._staging.stage(0, lay)[0], gen._renderer.device))
    kern = launch_us(gen._renderer, items, canvases, H, W, u8, f32)
    pil_ms, _ = pil_pass(texts, quads, items["canvas"].tolist(), H, W, n, 48)
    pixels = n * H * W
    lines = ["%s: %d canvases of %d x %d, %d words" % (name, n, H, W, len(items)),
             "  whole call   median %.3f ms (min %.3f, max %.3f) of 15" % whole,
             "  planning     median %.3f ms (min %.3f, max %.3f) of 15, host" % planning,
             "  staging copy median %.3f ms (min %.3f, max %.3f) of 15, device events, %d bytes" % (copy + (lay.total,)),
             "  launch to launch, at most the kernel: median %.1f us (min %.1f, max %.1f) of 7 windows of 50 = %.2f ns per pixel"
             % (kern + (kern[0] * 1e3 / pixels,)),
             "  PIL, one core, draw + perspective warp + composite of the same words: %.1f ms = %.0f x the whole call"
             % (pil_ms, pil_ms / whole[0])]
    if not scene:
        lines.append("  beside the CRNN step of %.2f ms (README): whole call %.1f %%, launch to launch %.1f %%"
                     % (STEP_MS, 100 * whole[0] / STEP_MS, 100 * kern[0] / 1e3 / STEP_MS))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_synth_text.py measures on the GPU; there is none")
    charset = EnglishCharset()
    atlas = GlyphAtlas.from_font(charset, size=48)
    lines = ["%s; atlas of Pillow's built-in font, %d x %d" % (torch.cuda.get_device_name(0), atlas.gh, atlas.coverage.shape[1])]
    lines += bench("SynthText 32 x 128", SynthText(charset, [atlas], WORDS, image_size=(32, 128)), 256, 32, 128, False, True, False)
    lines += bench("SynthText 32 x 100", SynthText(charset, [atlas], WORDS, image_size=(32, 100)), 256, 32, 100, False, True, False)
    lines += bench("SynthScenes 640 x 640", SynthScenes(charset, [atlas], WORDS, canvas=(640, 640), words_per_scene=(12, 12)),
                   8, 640, 640, True, False, True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
