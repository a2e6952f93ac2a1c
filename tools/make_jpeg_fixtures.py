"""Writes the JPEG fixtures of tests/golden/jpeg/ and the two host-fallback files of tests/golden/jpeg_host/ with PIL (run once,
on a machine that has it; the files are committed so that the GPU tests need no PIL):  python tools/make_jpeg_fixtures.py

Content: a smooth gradient plus noise plus saturated patches, so that coefficients of every size and the range limit occur.
The same generator (`content`, `encode`) feeds the random matrix of tests/test_jpeg_decode_cpu.py and tools/bench_jpeg_decode.py."""
import io
import os

import numpy as np

# name: (width, height, PIL mode, save options)
FIXTURES = {
    "c444_1x1_q75": (1, 1, "RGB", dict(quality=75, subsampling=0)),
    "c420_2x2_q75": (2, 2, "RGB", dict(quality=75, subsampling=2)),
    "c420_3x3_q30": (3, 3, "RGB", dict(quality=30, subsampling=2)),
    "c422_7x5_q95": (7, 5, "RGB", dict(quality=95, subsampling=1)),
    "gray_8x8_q100": (8, 8, "L", dict(quality=100)),
    "c420_9x17_q75_opt": (9, 17, "RGB", dict(quality=75, subsampling=2, optimize=True)),
    "c444_16x16_q100": (16, 16, "RGB", dict(quality=100, subsampling=0)),
    "c422_17x33_q75_rst1": (17, 33, "RGB", dict(quality=75, subsampling=1, restart_marker_blocks=1)),
    "c420_100x32_q75": (100, 32, "RGB", dict(quality=75, subsampling=2)),
    "c420_101x33_q75_rst3": (101, 33, "RGB", dict(quality=75, subsampling=2, restart_marker_blocks=3)),
    "c444_101x33_q95_opt": (101, 33, "RGB", dict(quality=95, subsampling=0, optimize=True)),
    "gray_256x64_q30_rstrow": (256, 64, "L", dict(quality=30, restart_marker_rows=1, optimize=True)),
    "c420_300x200_q75_rstrow": (300, 200, "RGB", dict(quality=75, subsampling=2, restart_marker_rows=1)),
}


def content(width, height, seed, channels=3):
    """uint8 [height, width, channels]: gradient + noise + saturated patches."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    img = np.empty((height, width, channels))
    for c in range(channels):
        fx, fy, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 6.28)
        img[:, :, c] = 128 + 100 * np.sin(fx * xx / max(width, 8) * 6.28 + fy * yy / max(height, 8) * 6.28 + ph)
    img += rng.normal(0, 12, img.shape)
    for _ in range(3):
        y0, x0 = rng.randint(0, height), rng.randint(0, width)
        y1, x1 = y0 + rng.randint(1, max(2, height // 3 + 1)), x0 + rng.randint(1, max(2, width // 3 + 1))
        img[y0:y1, x0:x1] = rng.choice([0.0, 255.0], size=channels)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(pixels, mode="RGB", **options):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels if mode == "RGB" else pixels[:, :, 0], mode).save(buf, "JPEG", **options)
    return buf.getvalue()


def main():
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg")
    os.makedirs(out, exist_ok=True)
    for seed, (name, (w, h, mode, options)) in enumerate(sorted(FIXTURES.items())):
        blob = encode(content(w, h, 100 + seed, 3 if mode == "RGB" else 1), mode, **options)
        with open(os.path.join(out, name + ".jpg"), "wb") as f:
            f.write(blob)
        print("%-28s %6d bytes" % (name, len(blob)))
    # what the device does not decode: the host-fallback cases of tests/test_jpeg_decode_gpu.py (tests/golden/jpeg_host/)
    from PIL import Image
    host = os.path.join(os.path.dirname(out), "jpeg_host")
    os.makedirs(host, exist_ok=True)
    Image.fromarray(content(90, 30, 300)).save(os.path.join(host, "progressive_90x30.jpg"), "JPEG", quality=80, progressive=True)
    Image.fromarray(content(64, 24, 301)).save(os.path.join(host, "rgb_64x24.png"), "PNG")


if __name__ == "__main__":
    main()
