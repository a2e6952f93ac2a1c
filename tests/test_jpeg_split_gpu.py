"""The split JPEG decoder on the GPU (csrc/jpeg_split.hip) against its restatement (tests/_jpeg_split_ref.py, which
tests/test_jpeg_split_cpu.py holds against the serial restatement and, through it, PIL): bit for bit, no tolerance.  All inputs
are committed files (tests/golden/jpeg_split/, tools/make_jpeg_split_fixtures.py); the host-fallback cases run where PIL imports."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _jpeg_ref as ref  # noqa: E402
import _jpeg_split_ref as sref  # noqa: E402
from test_jpeg_split_cpu import NAMES, blob_of, damaged  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd.data import (DetectionAugmenter, DetectionPipeline, EncodedDetectionPipeline, JpegDecoder,  # noqa: E402
                                Prefetcher)
from megreader_amd.data import jpeg_decode as jd  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL, WS_FILL = 0xA5, 0x5A
GUARD = 256                     # guard bytes in front of and behind the workspace, and behind the output


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def fixtures():
    """{name: (blob, the serial restatement's BGR pixels)}: computed once, never modified.  (The CPU tests show that the split
    restatement gives exactly these pixels at every sub-sequence size.)"""
    out = {}
    for name in NAMES:
        pixels = ref.decode(blob_of(name))
        pixels.setflags(write=False)
        out[name] = (blob_of(name), pixels)
    return out


def decode_raw(blobs, split_above, S, rgb=False):
    """mr_jpeg_decode_split at the C ABI with guard bytes round the workspace and behind the output: (plan, workspace, output
    incl. its guard, status) on the host; asserts that the workspace guards are intact."""
    plan = jd.make_plan(blobs).split(split_above, S)
    dev = torch.device("cuda")
    blob_buf = np.zeros(max(plan.blob_bytes, 16), dtype=np.uint8)
    plan.fill_blobs(blob_buf)
    sections = plan.sections()
    table = np.concatenate([np.frombuffer(s, dtype=np.uint8) for s in sections[1:3] if not isinstance(s, int)])
    d_blobs, d_plan = torch.from_numpy(blob_buf).to(dev), torch.from_numpy(table.copy()).to(dev)
    d_split = torch.from_numpy(np.frombuffer(plan.split_table(), dtype=np.uint8).copy() if plan.n_splits
                               else np.zeros(16, dtype=np.uint8)).to(dev)
    d_ws = torch.full((GUARD + max(plan.workspace_bytes, 16) + GUARD,), WS_FILL, dtype=torch.uint8, device=dev)
    d_out = torch.full((plan.out_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    d_status = torch.full((plan.n,), -7, dtype=torch.int32, device=dev)
    _lib.call("mr_jpeg_decode_split", d_blobs.data_ptr(), d_plan.data_ptr(), plan.n, plan.n_items,
              plan.split_table() if plan.n_splits else None, d_split.data_ptr() if plan.n_splits else None, plan.n_splits,
              d_ws.data_ptr() + GUARD, d_out.data_ptr(), d_status.data_ptr(), 1 if rgb else 0)
    torch.cuda.synchronize()
    ws = d_ws.cpu().numpy()
    assert (ws[:GUARD] == WS_FILL).all() and (ws[GUARD + plan.workspace_bytes:] == WS_FILL).all()
    return plan, ws[GUARD:GUARD + plan.workspace_bytes], d_out.cpu().numpy(), d_status.cpu().numpy()


def check_regions(plan, out, want, skip=()):
    """Every image region equals `want[i]` bit for bit (except `skip`), and every byte outside the regions of OK images is still
    the sentinel."""
    covered = np.zeros(out.shape, dtype=bool)
    for i, im in enumerate(plan.images):
        if im.status != jd.OK:
            continue
        n = im.h * im.w * 3
        covered[im.out_off:im.out_off + n] = True
        if i in skip:
            continue
        got = out[im.out_off:im.out_off + n].reshape(im.h, im.w, 3)
        assert got.shape == want[i].shape, i
        assert np.array_equal(got, want[i]), (i, int((got != want[i]).sum()))
    assert (~covered).sum() >= GUARD
    assert (out[~covered] == SENTINEL).all()


@pytest.mark.parametrize("S", [16, 32, 128])
@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_split_from_the_first_byte(fixtures, name, S):
    blob, pixels = fixtures[name]
    plan, _, out, status = decode_raw([blob], 0, S)
    assert plan.n_splits == plan.n_items >= 1 and status.tolist() == [jd.OK]
    check_regions(plan, out, [pixels])
    plan, _, out, status = decode_raw([blob], 0, S, rgb=True)
    assert status.tolist() == [jd.OK]
    check_regions(plan, out, [pixels[:, :, ::-1]])


@pytest.mark.parametrize("name", NAMES)
def test_entry_states_and_block_offsets_in_the_workspace(fixtures, name):
    blob = fixtures[name][0]
    plan, ws, _, _ = decode_raw([blob], 0, 16)
    p = ref.parse(blob)
    for e, (mcu0, nmcu, off, length) in zip(plan.split_table(), p.items):
        st = sref.Stream(p, blob[off:off + length], nmcu, 16)
        states, counts = st.serial_states()
        assert e.n_sub == st.n_sub
        meta = ws[e.meta_off:e.meta_off + 16].view(np.int32)
        assert meta[0] == len(st.raw) and meta[1] == sum(counts)
        assert bytes(ws[e.raw_off:e.raw_off + len(st.raw)]) == st.raw
        assert not ws[e.raw_off + len(st.raw):e.raw_off + e.raw_bytes].any()
        got = ws[e.in_off:e.in_off + 8 * e.n_sub].view(np.uint32).reshape(-1, 2)
        assert [(int(a), int(b >> 8 & 255), int(b & 255)) for a, b in got] == states
        exits = ws[e.exit_off:e.exit_off + 8 * e.n_sub].view(np.uint32).reshape(-1, 2)
        assert [int(b >> 16) for _, b in exits] == counts
        block_off = ws[e.block_off:e.block_off + 4 * e.n_sub].view(np.int32)
        assert block_off.tolist() == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()


def host_fallback_blobs():
    try:
        import PIL  # noqa: F401
    except ImportError:
        return []
    return [(read(p), jd.host_decode(read(p))) for p in sorted(glob.glob(os.path.join(GOLDEN, "jpeg_host", "*")))]


def test_a_batch_that_mixes_everything(fixtures):
    """Split images, unsplit ones (the fixtures of tests/golden/jpeg/), the truncated file, and -- through JpegDecoder, where PIL
    imports -- a progressive JPEG and a PNG on the host path: every image is exact whatever surrounds it."""
    old = [(read(p), ref.decode(read(p))) for p in sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg")))]
    assert len(old) >= 12
    blob, _ = fixtures["c420_300x200_q75"]
    p = ref.parse(blob)
    cut = blob[:p.scan_off + p.scan_len // 2]
    pairs = [fixtures[NAMES[0]], old[0], fixtures[NAMES[1]], old[5], (cut, None), fixtures[NAMES[4]], old[11], fixtures[NAMES[2]],
             old[12], fixtures[NAMES[3]], fixtures[NAMES[5]]] + old[1:5]
    victim = 4
    blobs, want = [b for b, _ in pairs], [px for _, px in pairs]
    for S in (16, 128):
        plan, _, out, status = decode_raw(blobs, 1024, S)
        assert 0 < plan.n_splits < plan.n_items                         # both paths in one launch sequence
        assert status[victim] == jd.CORRUPT and (np.delete(status, victim) == jd.OK).all()
        check_regions(plan, out, want, skip=(victim,))
    host = host_fallback_blobs()
    dec = JpegDecoder(split_above=1024, subseq_bytes=32, host_above=None)
    tensors, status = dec.decode(blobs + [b for b, _ in host], check=False)
    assert status.tolist() == [jd.CORRUPT if i == victim else jd.OK for i in range(len(blobs))] + [jd.UNSUPPORTED] * len(host)
    for i, (t, px) in enumerate(zip(tensors, want + [px for _, px in host])):
        if i != victim:
            assert np.array_equal(t.cpu().numpy(), px), i


def test_several_split_items_in_one_image(fixtures):
    blob, pixels = fixtures["c420_300x200_q75_rst5rows"]
    for S in (16, 128):
        plan, _, out, status = decode_raw([blob], 1024, S)
        assert plan.n_splits == plan.n_items > 1                         # every restart interval is a split item of its own
        assert status.tolist() == [jd.OK]
        check_regions(plan, out, [pixels])


def test_one_sub_sequence(fixtures):
    blob, pixels = fixtures["c444_1x1"]
    plan, _, out, status = decode_raw([blob], 0, 1024)
    assert plan.n_splits == 1 and plan.split_table()[0].n_sub == 1 and status.tolist() == [jd.OK]
    check_regions(plan, out, [pixels])


def test_damaged_streams_keep_the_serial_status_and_stay_contained(fixtures):
    blob, _ = fixtures["c420_300x200_q75"]
    cases = damaged(blob, ref.parse(blob))
    names = sorted(cases)
    want = [ref.decode_status(cases[n]) for n in names]
    for S in (16, 128):
        plan, _, out, status = decode_raw([cases[n] for n in names], 0, S)      # (the guards are checked inside)
        assert plan.n_splits == len(names)
        assert status.tolist() == [s for _, s in want]
        ok = [i for i, (_, s) in enumerate(want) if s == ref.OK]
        assert ok and len(ok) < len(names)
        check_regions(plan, out, [px for px, _ in want], skip=[i for i in range(len(names)) if i not in ok])


def test_without_a_threshold_nothing_is_split(fixtures):
    blob, pixels = fixtures["c420_300x200_q75"]
    dec = JpegDecoder(host_above=None)
    assert dec.plan([blob]).n_splits == 0
    assert np.array_equal(dec.decode([blob])[0].cpu().numpy(), pixels)
    split = JpegDecoder(host_above=4096, split_above=4096)               # host_above is for what is still one wavefront's
    plan = split.plan([blob, fixtures["c444_1x1"][0]])
    assert plan.n_splits == 1 and plan.status == [jd.OK, jd.OK] and not plan.host
    assert np.array_equal(split.decode([blob])[0].cpu().numpy(), pixels)


# ---- EncodedDetectionPipeline

KEYS = ("image", "gt", "mask", "thresh_map", "thresh_mask", "ignore_tags")


def quads_for(shape, seed):
    rng = np.random.RandomState(seed)
    h, w = shape[:2]
    out = []
    for _ in range(3):
        x0, y0 = rng.uniform(0, w * 0.6), rng.uniform(0, h * 0.6)
        bw, bh = rng.uniform(20, w * 0.35), rng.uniform(12, h * 0.35)
        out.append([[x0, y0], [x0 + bw, y0 + 2], [x0 + bw, y0 + bh], [x0, y0 + bh - 2]])
    return np.array(out), [False, seed % 2 == 1, False]


@pytest.fixture(scope="module")
def detector_inputs():
    """[(blob, the restatement's BGR pixels)] of the two 640 x 640 files."""
    out = []
    for name in ("pad640_c420_q75", "pad640_c444_q50"):
        blob = blob_of(name)
        out.append((blob, np.ascontiguousarray(ref.decode(blob))))
    return out


def assert_same(got, want):
    for key in KEYS:
        assert torch.equal(got[key], want[key]), key


def test_encoded_detection_pipeline_without_an_augmenter(detector_inputs):
    blobs = [b for b, _ in detector_inputs]
    pixels = [px for _, px in detector_inputs]
    polys, tags = zip(*[quads_for((640, 640), s) for s in range(len(blobs))])
    want = DetectionPipeline().process(pixels, polys, tags)
    pipe = EncodedDetectionPipeline(split_above=2048, subseq_bytes=64)
    assert pipe.decoder.plan(blobs).n_splits == len(blobs)
    got = pipe.process(blobs, polys, tags)
    assert_same(got, want)
    assert got['jpeg_status'].tolist() == [jd.OK] * len(blobs)
    batches = list(Prefetcher([(blobs, polys, tags), (blobs[::-1], polys[::-1], tags[::-1])], pipe))
    assert_same(batches[0], want)
    assert_same(batches[1], DetectionPipeline().process(pixels[::-1], polys[::-1], tags[::-1]))
    with pytest.raises(ValueError, match=r"\[1\]"):
        pipe.pack([blobs[0], blobs[0][:40]], polys, tags)


def test_encoded_detection_pipeline_with_fixed_plans(fixtures, detector_inputs):
    pairs = [fixtures["c420_300x200_q75"], detector_inputs[1], fixtures["c422_120x48_q50_opt"]] + host_fallback_blobs()[:1]
    blobs, pixels = [b for b, _ in pairs], [np.ascontiguousarray(px) for _, px in pairs]
    polys, tags = zip(*[quads_for(px.shape, 10 + i) for i, px in enumerate(pixels)])
    aug = DetectionAugmenter(size=(640, 640), seed=5)
    plans = [aug.sample(px.shape, q, t) for px, q, t in zip(pixels, polys, tags)]
    want = DetectionPipeline().process(pixels, polys, tags, plans=plans)
    pipe = EncodedDetectionPipeline(split_above=1024, subseq_bytes=128)
    got = pipe.process(blobs, polys, tags, plans=plans)
    assert_same(got, want)
    assert got['jpeg_status'].tolist()[:3] == [jd.OK] * 3
