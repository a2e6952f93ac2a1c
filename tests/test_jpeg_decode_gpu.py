"""The GPU JPEG decoder (csrc/jpeg.hip) against the numpy restatement (tests/_jpeg_ref.py, which the CPU tests hold against PIL):
bit for bit, no tolerance.  The fixtures are committed files, so nothing here needs PIL; the host-fallback cases run where it
imports."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _jpeg_ref as ref  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data import DevicePipeline, EncodedDevicePipeline, JpegDecoder, Prefetcher  # noqa: E402
from megreader_amd.data import jpeg_decode as jd  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0xA5
TAIL = 256                      # guard bytes behind the last image region


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def fixtures():
    """{name: (blob, the restatement's BGR pixels)}: computed once, never modified."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg"))):
        blob = read(path)
        pixels = ref.decode(blob)
        pixels.setflags(write=False)
        out[os.path.splitext(os.path.basename(path))[0]] = (blob, pixels)
    assert len(out) >= 12
    return out


def decode_raw(blobs, rgb=False):
    """mr_jpeg_decode at the C ABI into an output buffer pre-filled with a sentinel: (plan, uint8 output incl. TAIL guard bytes,
    int32 status), all on the host."""
    plan = jd.make_plan(blobs)
    dev = torch.device("cuda")
    blob_buf = np.zeros(max(plan.blob_bytes, 16), dtype=np.uint8)
    plan.fill_blobs(blob_buf)
    table = np.concatenate([np.frombuffer(s, dtype=np.uint8) for s in plan.sections()[1:] if not isinstance(s, int)])
    d_blobs, d_plan = torch.from_numpy(blob_buf).to(dev), torch.from_numpy(table.copy()).to(dev)
    d_ws = torch.full((max(plan.workspace_bytes, 16),), 0x5A, dtype=torch.uint8, device=dev)
    d_out = torch.full((plan.out_bytes + TAIL,), SENTINEL, dtype=torch.uint8, device=dev)
    d_status = torch.full((plan.n,), -7, dtype=torch.int32, device=dev)
    _lib.call("mr_jpeg_decode", d_blobs.data_ptr(), d_plan.data_ptr(), plan.n, plan.n_items, d_ws.data_ptr(), d_out.data_ptr(),
              d_status.data_ptr(), 1 if rgb else 0)
    torch.cuda.synchronize()
    return plan, d_out.cpu().numpy(), d_status.cpu().numpy()


def check_regions(plan, out, want, skip=()):
    """Every image region equals `want[i]` bit for bit (except `skip`), and every byte outside the regions of OK images is still
    the sentinel: between two regions (odd widths leave gaps up to 15 bytes) and behind the last one."""
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
    assert (~covered).sum() >= TAIL
    assert (out[~covered] == SENTINEL).all()


def test_all_fixtures_in_one_batch(fixtures):
    blobs = [b for b, _ in fixtures.values()]
    want = [p for _, p in fixtures.values()]
    plan, out, status = decode_raw(blobs)
    assert plan.n_items > plan.n                                        # the restart fixtures are several work items each
    assert len({(im.hs, im.vs, im.ncomp) for im in plan.images}) == 4   # mixed samplings and sizes in one plan
    assert (status == jd.OK).all()
    check_regions(plan, out, want)
    plan, out, status = decode_raw(blobs, rgb=True)
    assert (status == jd.OK).all()
    check_regions(plan, out, [p[:, :, ::-1] for p in want])


@pytest.mark.parametrize("name", ["c420_101x33_q75_rst3", "c444_1x1_q75"])
def test_batch_of_one(fixtures, name):
    blob, pixels = fixtures[name]
    plan, out, status = decode_raw([blob])
    assert status.tolist() == [jd.OK]
    check_regions(plan, out, [pixels])


def test_more_images_than_lanes(fixtures):
    names = ["c420_3x3_q30", "c422_7x5_q95"] * 70
    plan, out, status = decode_raw([fixtures[n][0] for n in names])
    assert plan.n == plan.n_items == 140 and (status == jd.OK).all()
    check_regions(plan, out, [fixtures[n][1] for n in names])


def test_truncated_stream_is_reported_and_contained(fixtures):
    """One image's entropy-coded segment cut in half (the file ends there) inside an otherwise well-formed batch: the plan
    cannot know, the kernel runs out of bytes, reads zeros, and reports it; nothing else changes."""
    names = list(fixtures)
    victim = names.index("c444_101x33_q95_opt")
    blobs = [b for b, _ in fixtures.values()]
    p = ref.parse(blobs[victim])
    blobs[victim] = blobs[victim][:p.scan_off + p.scan_len // 2]
    assert ref.decode_status(blobs[victim])[1] == ref.CORRUPT
    plan, out, status = decode_raw(blobs)
    assert plan.status == [jd.OK] * len(blobs)
    assert status[victim] == jd.CORRUPT
    assert (np.delete(status, victim) == jd.OK).all()
    check_regions(plan, out, [px for _, px in fixtures.values()], skip=(victim,))


def test_decoder_returns_views_and_names_corrupt_images(fixtures):
    names = ["c420_100x32_q75", "gray_256x64_q30_rstrow", "c422_7x5_q95"]
    blobs = [fixtures[n][0] for n in names]
    images = JpegDecoder(host_above=None).decode(blobs)
    for n, t in zip(names, images):
        assert t.dtype == torch.uint8 and t.is_cuda and np.array_equal(t.cpu().numpy(), fixtures[n][1])
    assert len({t.untyped_storage().data_ptr() for t in images}) == 1   # views of one buffer
    rgb = JpegDecoder(mode='RGB', host_above=None).decode(blobs[:1])[0]
    assert np.array_equal(rgb.cpu().numpy(), fixtures[names[0]][1][:, :, ::-1])
    p = ref.parse(blobs[0])
    cut = blobs[0][:p.scan_off + p.scan_len // 2]                       # ends inside its entropy-coded segment: the kernel finds out
    with pytest.raises(ValueError, match=r"\[1\]"):
        JpegDecoder(host_above=None).decode([blobs[0], cut, blobs[2]])
    tensors, status = JpegDecoder(host_above=None).decode([blobs[0], cut, blobs[0][:30]], check=False)
    assert status.tolist() == [jd.OK, jd.CORRUPT, jd.CORRUPT] and tensors[2] is None
    assert np.array_equal(tensors[0].cpu().numpy(), fixtures[names[0]][1])


def host_fallback_blobs():
    """[(blob, BGR pixels)] of files the device does not decode, where PIL is there to decode them on the host."""
    try:
        import PIL  # noqa: F401
    except ImportError:
        return []
    return [(read(p), jd.host_decode(read(p))) for p in sorted(glob.glob(os.path.join(GOLDEN, "jpeg_host", "*")))]


@pytest.fixture(scope="module")
def mixed_batch(fixtures):
    """(blobs, pixels, texts): recognition-sized fixtures, and the host-fallback files where PIL imports."""
    names = ["c420_100x32_q75", "c420_101x33_q75_rst3", "c444_101x33_q95_opt", "gray_256x64_q30_rstrow", "c420_9x17_q75_opt",
             "c422_17x33_q75_rst1"]
    pairs = [fixtures[n] for n in names] + host_fallback_blobs()
    texts = ["word%d" % i for i in range(len(pairs))]
    return [b for b, _ in pairs], [np.ascontiguousarray(p) for _, p in pairs], texts


def assert_batches_equal(got, want):
    for key in ("image", "label", "length"):
        assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("mode", ["resize", "pad"])
def test_encoded_pipeline_equals_device_pipeline(mixed_batch, mode):
    blobs, pixels, texts = mixed_batch
    charset = EnglishCharset()
    plain = DevicePipeline(image_size=(32, 128), mode=mode, charset=charset)
    encoded = EncodedDevicePipeline(image_size=(32, 128), mode=mode, charset=charset)
    want = plain.process(pixels, texts)
    got = encoded.process(blobs, texts)
    assert_batches_equal(got, want)
    assert got['jpeg_status'].dtype == torch.int32
    expect = [jd.OK] * 6 + [jd.UNSUPPORTED] * (len(blobs) - 6)
    assert got['jpeg_status'].tolist() == expect
    staged, layout = encoded.pack(blobs, texts)
    for photo, px in zip(encoded.photos(encoded.upload(staged, layout), layout), pixels):
        assert np.array_equal(photo.cpu().numpy(), px)
    # the same batches through the prefetcher, both slots in use
    batches = list(Prefetcher([(blobs, texts), (blobs[::-1], texts[::-1]), (blobs[:3], texts[:3])], encoded))
    assert len(batches) == 3
    assert_batches_equal(batches[0], want)
    assert_batches_equal(batches[1], plain.process(pixels[::-1], texts[::-1]))
    assert_batches_equal(batches[2], plain.process(pixels[:3], texts[:3]))


def test_encoded_pipeline_refuses_corrupt_headers(fixtures):
    blob = fixtures["c420_100x32_q75"][0]
    with pytest.raises(ValueError, match=r"\[1\]"):
        EncodedDevicePipeline().pack([blob, blob[:50]], ["a", "b"])


def test_records_to_batch_on_the_device_equals_the_host_path(fixtures):
    msgpack = pytest.importorskip("msgpack")
    pytest.importorskip("PIL")
    from megreader_amd.data import records_to_batch
    names = ["c420_100x32_q75", "c422_17x33_q75_rst1", "gray_256x64_q30_rstrow"]
    records = [msgpack.dumps({b'img': fixtures[n][0], b'gt': n[:6].encode()}) for n in names]
    host = records_to_batch(records, DevicePipeline(image_size=(32, 100)))
    device = records_to_batch(records, EncodedDevicePipeline(image_size=(32, 100)), decode='device')
    assert_batches_equal(device, host)
    with pytest.raises(TypeError):
        records_to_batch(records, DevicePipeline(image_size=(32, 100)), decode='device')


def test_large_items_go_to_the_host(fixtures):
    pytest.importorskip("PIL")
    names = ["c444_101x33_q95_opt", "c420_100x32_q75"]
    blobs = [fixtures[n][0] for n in names]
    dec = JpegDecoder(host_above=4096)                                   # the 5 KB single-item file exceeds it
    plan = dec.plan(blobs)
    assert plan.status == [jd.UNSUPPORTED, jd.OK] and list(plan.host) == [0]
    for n, t in zip(names, dec.decode(blobs)):
        assert np.array_equal(t.cpu().numpy(), fixtures[n][1])
