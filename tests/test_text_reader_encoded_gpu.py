"""`TextReader(encoded=True)`: the photos as encoded files, decoded on the device (data/jpeg_decode.py, csrc/jpeg_split.hip), read
exactly like the same photos decoded beforehand.  The files are the scenes of tests/test_text_reader_gpu.py, written by
tools/make_jpeg_split_fixtures.py; the decoded arrays are the restatement's (tests/_jpeg_ref.py), so no PIL is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _jpeg_ref as ref  # noqa: E402
from test_text_reader_gpu import DET_SIZE, SCENES, SoftSpell, SpellByBrightness, check, detector  # noqa: E402
from megreader_amd import TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_split")


@pytest.fixture(scope="module")
def scenes():
    """(blobs, the restatement's BGR pixels)."""
    blobs = []
    for i in range(len(SCENES)):
        with open(os.path.join(GOLDEN, "reader_scene%d.jpg" % i), "rb") as f:
            blobs.append(f.read())
    return blobs, [np.ascontiguousarray(ref.decode(b)) for b in blobs]


@pytest.mark.parametrize("split_above", [None, 0])
def test_greedy_reading_from_bytes_equals_reading_from_pixels(scenes, split_above):
    blobs, pixels = scenes
    charset = EnglishCharset()
    want = TextReader(detector, SpellByBrightness(charset), charset, det_size=DET_SIZE).read(pixels)
    check(want)                                                         # the lossy files still read as the painted scenes
    reader = TextReader(detector, SpellByBrightness(charset), charset, det_size=DET_SIZE, encoded=True)
    if split_above is not None:                                         # every photo through the split path, however small
        reader.det_pipeline.decoder.split_above = split_above
        assert reader.det_pipeline.decoder.plan(blobs).n_splits == len(blobs)
    assert reader.read(blobs) == want
    assert reader.read([]) == []


def test_character_boxes_from_bytes_equal_those_from_pixels(scenes):
    blobs, pixels = scenes
    charset = EnglishCharset()
    kwargs = dict(det_size=DET_SIZE, decode='beam', beam_width=4, chars=True, scores=True)
    want = TextReader(detector, SoftSpell(charset), charset, **kwargs).read(pixels)
    reader = TextReader(detector, SoftSpell(charset), charset, encoded=True, **kwargs)
    reader.det_pipeline.decoder.split_above = 0
    got = reader.read(blobs)
    assert got == want
    assert any(item['chars'] for found in got for item in found)
