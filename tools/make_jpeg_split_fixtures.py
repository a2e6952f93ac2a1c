"""Writes the fixtures of tests/golden/jpeg_split/ with PIL (run once, on a machine that has it; the files are committed):
    python tools/make_jpeg_split_fixtures.py

The smallest files on which the split JPEG decoder (csrc/jpeg_split.hip) can go wrong: all without restart markers unless named
so, so that each is ONE long work item.  tests/test_jpeg_split_cpu.py asserts what they are chosen for (more than two workgroups
of 16-byte sub-sequences, a wrong workgroup-boundary guess, a synchronisation distance above 3, a sub-sequence that never
synchronises), so that a regenerated file cannot quietly stop testing it.  `padded` makes the 640x640 inputs of the
EncodedDetectionPipeline test from fixture content."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_jpeg_fixtures import content, encode  # noqa: E402

# in seed order (500, 501, ...): name, (width, height, PIL mode, save options)
FIXTURES = [
    ("c420_300x200_q75", (300, 200, "RGB", dict(quality=75, subsampling=2))),
    ("c444_101x33_q95", (101, 33, "RGB", dict(quality=95, subsampling=0))),
    ("c422_120x48_q50_opt", (120, 48, "RGB", dict(quality=50, subsampling=1, optimize=True))),
    ("gray_256x64_q30_opt", (256, 64, "L", dict(quality=30, optimize=True))),
    ("c420_300x200_q75_rst5rows", (300, 200, "RGB", dict(quality=75, subsampling=2, restart_marker_rows=5))),
    ("c444_1x1", (1, 1, "RGB", dict(quality=75, subsampling=0))),
]


def padded(pixels, height=640, width=640, fill=128, **options):
    """The RGB pixels in the top left corner of a height x width image of `fill`, encoded without restart markers."""
    big = np.full((height, width, 3), fill, dtype=np.uint8)
    big[:pixels.shape[0], :pixels.shape[1]] = pixels
    return encode(big, "RGB", **(options or dict(quality=75, subsampling=2)))


def main():
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_split")
    os.makedirs(out, exist_ok=True)
    for seed, (name, (w, h, mode, options)) in enumerate(FIXTURES):
        blob = encode(content(w, h, 500 + seed, 3 if mode == "RGB" else 1), mode, **options)
        with open(os.path.join(out, name + ".jpg"), "wb") as f:
            f.write(blob)
        print("%-28s %6d bytes" % (name, len(blob)))
    # the detector-sized inputs of the EncodedDetectionPipeline test: fixture content padded to 640 x 640, one item each
    for seed, (name, options) in enumerate([("pad640_c420_q75", dict(quality=75, subsampling=2)),
                                            ("pad640_c444_q50", dict(quality=50, subsampling=0))]):
        blob = padded(content(300 - 67 * seed, 200 + 31 * seed, 520 + seed), **options)
        with open(os.path.join(out, name + ".jpg"), "wb") as f:
            f.write(blob)
        print("%-28s %6d bytes" % (name, len(blob)))
    # the photos of tests/test_text_reader_gpu.py as files, for tests/test_text_reader_encoded_gpu.py
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(out))), os.path.dirname(os.path.dirname(out))]
    from test_text_reader_gpu import photos
    for i, photo in enumerate(photos()):
        blob = encode(np.ascontiguousarray(photo[:, :, ::-1]), "RGB", quality=100, subsampling=0)
        with open(os.path.join(out, "reader_scene%d.jpg" % i), "wb") as f:
            f.write(blob)
        print("%-28s %6d bytes" % ("reader_scene%d" % i, len(blob)))


if __name__ == "__main__":
    main()
