"""On-device input pipeline (csrc/image_sample.hip and csrc/pipeline.hip, megreader_amd.data.DevicePipeline) against oracle/pipeline.py: resize
(up / down / identity, both modes) + normalise + CHW bit-exact with the numpy restatement of cv2's float32 path, label
encoding identical to charsets.string_to_label, and the prefetcher delivering batches in order.  Second half: degenerate and
large source shapes, the copy branch, the padding columns, hand-built descriptors (pitch, offsets) through the C ABI; label
encoding with charsets that fold case or hold 5 360 classes, at other max_size, and of every codepoint once."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data import DevicePipeline, Prefetcher  # noqa: E402
from oracle.pipeline import process_sample  # noqa: E402


def _samples(seed, n):
    rng = np.random.RandomState(seed)
    shapes = [(32, 128), (31, 100), (48, 200), (20, 37), (64, 256), (17, 300), (33, 33), (100, 40)]
    images = [rng.randint(0, 256, size=shapes[i % len(shapes)] + (3,)).astype(np.uint8) for i in range(n)]
    alphabet = "ABCxyz019 -_Zq"
    texts = ["".join(alphabet[j] for j in rng.randint(0, len(alphabet), size=rng.randint(1, 40))) for _ in range(n)]
    return images, texts


@pytest.mark.parametrize("mode", ["resize", "pad"])
@pytest.mark.parametrize("size", [(32, 128), (64, 256)])
def test_pipeline_matches_oracle(mode, size):
    cs = EnglishCharset()
    pipe = DevicePipeline(image_size=size, mode=mode, charset=cs)
    images, texts = _samples(1, 19)
    batch = pipe.process(images, texts)
    torch.cuda.synchronize()
    assert batch['image'].shape == (19, 3) + size and batch['image'].dtype == torch.float32
    worst = 0.0
    for i, (im, tx) in enumerate(zip(images, texts)):
        chw, lab, ln = process_sample(im, tx, size, mode, cs.index)
        got = batch['image'][i].cpu().numpy()
        worst = max(worst, float(np.abs(got - chw).max()))
        assert np.array_equal(got, chw), (i, im.shape, float(np.abs(got - chw).max()))
        assert np.array_equal(batch['label'][i].cpu().numpy(), lab), (i, tx)
        assert int(batch['length'][i]) == int(ln)


def test_prefetcher_order_and_overlap():
    cs = EnglishCharset()
    pipe = DevicePipeline(image_size=(32, 128), mode='resize', charset=cs)
    batches = [_samples(10 + k, 8) for k in range(5)]
    got = []
    for b in Prefetcher(batches, pipe):
        got.append((b['image'].clone(), b['label'].clone(), b['length'].clone()))
    torch.cuda.synchronize()
    assert len(got) == 5
    for (images, texts), (img, lab, ln) in zip(batches, got):
        for i, (im, tx) in enumerate(zip(images, texts)):
            chw, l_, n_ = process_sample(im, tx, (32, 128), 'resize', cs.index)
            assert np.array_equal(img[i].cpu().numpy(), chw)
            assert np.array_equal(lab[i].cpu().numpy(), l_) and int(ln[i]) == int(n_)


# --------------------------------------------------------------------------------- resize / normalise at the edges
import ctypes  # noqa: E402

from megreader_amd import _lib  # noqa: E402
from megreader_amd.charsets import Charset, EnglishPrintableCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN, ImgDesc, charset_table, target_width  # noqa: E402

EDGE_SHAPES = [(1, 1), (1, 50), (50, 1), (2, 2), (32, 77), (100, 5), (3, 400), (255, 1000)]


def _zero_pixel():
    """the normalised value of a zero pixel, per channel: (f32)(0.0 - mean) / 255.f"""
    return (np.zeros(3, np.float64) - np.array(RGB_MEAN)).astype(np.float32) / np.float32(255.)


@pytest.mark.parametrize("mode", ["resize", "pad"])
@pytest.mark.parametrize("size", [(32, 128), (48, 160)])
def test_pipeline_edge_shapes_match_oracle(mode, size):
    """one-pixel, one-row, one-column, tiny, tall, very wide and large sources; the canvas size itself (cv2.resize returns a
    copy) and the canvas height at other widths (only the horizontal pass interpolates)"""
    cs = EnglishCharset()
    H, W = size
    shapes = EDGE_SHAPES + [(H, W), (H, W - 1), (H, 40), (H, 3 * W), (H, 32), (H - 1, W), (H + 1, W)]
    rng = np.random.RandomState(H)
    images = [rng.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in shapes]
    texts = ["A%d" % i for i in range(len(images))]
    batch = DevicePipeline(image_size=size, mode=mode, charset=cs).process(images, texts)
    torch.cuda.synchronize()
    got_all = batch['image'].cpu().numpy()
    zero = _zero_pixel()
    copies = 0
    for i, (im, tx) in enumerate(zip(images, texts)):
        chw, lab, ln = process_sample(im, tx, size, mode, cs.index)
        got = got_all[i]
        print("%s %s source %s: max |got - oracle| = %g" % (mode, size, im.shape[:2], float(np.abs(got - chw).max())))
        assert np.array_equal(got, chw), (i, im.shape, float(np.abs(got - chw).max()))
        dst_w = W if mode == 'resize' else target_width('pad', size, im.shape)
        if mode == 'pad':
            assert np.array_equal(got[:, :, dst_w:], np.broadcast_to(zero[:, None, None], (3, H, W - dst_w))), (i, im.shape)
        if im.shape[0] == H and im.shape[1] == dst_w:                # the copy branch: the source pixels, normalised
            copies += 1
            src = ((im.astype(np.float32).astype(np.float64) - np.array(RGB_MEAN)).astype(np.float32) / np.float32(255.))
            assert np.array_equal(got[:, :, :dst_w], src.transpose(2, 0, 1))
        assert np.array_equal(batch['label'][i].cpu().numpy(), lab) and int(batch['length'][i]) == int(ln)
    assert copies >= 1
    if mode == 'pad':
        widths = set(target_width('pad', size, im.shape) for im in images)
        assert 32 in widths and W in widths and len(widths) >= 3       # the floor, the cap and widths between them


def test_resize_normalize_abi_pitch_offsets_and_empty_batch():
    """mr_resize_normalize on a hand-built descriptor array: rows padded to a pitch above 3 * w, images at non-zero 16-byte
    aligned offsets in an order that is not the batch order, every byte that is not a pixel set to 0xA5; and N = 0"""
    assert ctypes.sizeof(ImgDesc) == 40 == _lib.load().mr_sizeof_img_desc()
    # written out by hand, independent of any reading of the header (as tests/test_tuning_cpu.py does for mr_tuning)
    assert [(name, getattr(ImgDesc, name).offset) for name, _ in ImgDesc._fields_] == [
        ("offset", 0), ("h", 8), ("w", 12), ("pitch", 16), ("dst_w", 20), ("scale_x", 24), ("scale_y", 32)]
    assert ImgDesc._fields_ == _lib.STRUCTS["mr_img_desc"]
    H, W = 32, 128
    rng = np.random.RandomState(3)
    #          shape     pitch                 offset   dst_w
    plan = [((20, 37), 37 * 3 + 17, 8224, 128), ((32, 64), 64 * 3 + 64, 16, 64), ((1, 1), 16, 32768, 32),
            ((45, 300), 300 * 3 + 1, 49152, 128), ((32, 128), 128 * 3 + 5, 16384, 128)]
    host = np.full(49152 + 45 * 901 + 64, 0xA5, np.uint8)
    descs = (ImgDesc * len(plan))()
    images = []
    for i, (shape, pitch, offset, dst_w) in enumerate(plan):
        im = rng.randint(0, 256, size=shape + (3,)).astype(np.uint8)
        images.append(im)
        assert offset % 16 == 0 and pitch >= 3 * shape[1]
        end = offset + shape[0] * pitch
        assert end <= host.size and np.all(host[offset:end] == 0xA5)             # the images do not overlap
        rows = host[offset:end].reshape(shape[0], pitch)
        rows[:, :3 * shape[1]] = im.reshape(shape[0], -1)
        descs[i].offset, descs[i].h, descs[i].w, descs[i].pitch, descs[i].dst_w = offset, shape[0], shape[1], pitch, dst_w
        descs[i].scale_x = 1.0 / (float(dst_w) / float(shape[1]))
        descs[i].scale_y = 1.0 / (float(H) / float(shape[0]))
    dbuf = torch.from_numpy(host).to("cuda")
    ddesc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to("cuda")
    out = torch.full((len(plan), 3, H, W), float("nan"), device="cuda")
    _lib.call("mr_resize_normalize", _lib.ptr(dbuf), _lib.ptr(ddesc), len(plan), H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2],
              _lib.ptr(out))
    got = out.cpu().numpy()
    zero = _zero_pixel()
    for i, (im, (shape, pitch, offset, dst_w)) in enumerate(zip(images, plan)):
        if dst_w == W:
            chw = process_sample(im, "", (H, W), 'resize', None)[0]
        else:
            assert dst_w == target_width('pad', (H, W), shape)
            chw = process_sample(im, "", (H, W), 'pad', None)[0]
            assert np.array_equal(got[i][:, :, dst_w:], np.broadcast_to(zero[:, None, None], (3, H, W - dst_w)))
        assert np.array_equal(got[i], chw), (i, shape, float(np.abs(got[i] - chw).max()))
    # N = 0: accepted, nothing is read or written
    _lib.call("mr_resize_normalize", 0, 0, 0, H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], 0)
    batch = DevicePipeline(image_size=(H, W), mode='pad').process([], [])
    assert tuple(batch['image'].shape) == (0, 3, H, W) and tuple(batch['label'].shape) == (0, 32)
    assert tuple(batch['length'].shape) == (0,)
    torch.cuda.synchronize()


def test_pack_bytes_are_the_parents():
    """The staged byte stream of `DevicePipeline.pack` (mode 'pad', three sizes, one empty text) and its layout: LITERALS recorded
    from a build of the commit before `pack` moved onto data/staging.py, not from the code under test.  Packed twice into one
    slot with the buffer set to 0xA5 in between: the bytes between the sections are nobody's (tests/test_staging_cpu.py)."""
    import hashlib
    rng = np.random.RandomState(2)
    images = [rng.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((5, 7), (12, 9), (32, 40))]
    pipe = DevicePipeline(image_size=(32, 128), mode='pad')
    staged, _ = pipe.pack(images, ["Ab", "", "xyz9"])
    staged.fill_(0xA5)
    staged, layout = pipe.pack(images, ["Ab", "", "xyz9"])
    assert staged.is_pinned() and staged.numel() == 4480 and tuple(layout[:4]) == (3, 4288, 4416, 4448)
    assert hashlib.sha256(staged.numpy().tobytes()).hexdigest() == \
        "1951074ccd5555ad3dc0248cca6a398b4fdd5fcd715c6b76caf17a7fbc937a94"
    batch = pipe.upload(staged, layout)                                  # ... and the photos come back as views of the upload
    for im, photo in zip(images, pipe.photos(batch, layout)):
        assert np.array_equal(photo.cpu().numpy(), im)


# ------------------------------------------------------------------------------------------------- label encoding
def _mixed_charset(**kwargs):
    """5 360 classes: ideographs from U+4E00 on, Latin and Greek letters of both cases, the micro sign"""
    cs = Charset([chr(0x4E00 + i) for i in range(5348)] + list("abcXYZΑΒΣµ"), **kwargs)
    assert len(cs) == 5360
    return cs


LABEL_CHARSETS = {
    "printable": lambda: EnglishPrintableCharset(),
    "printable_case_sensitive": lambda: EnglishPrintableCharset(case_sensitive=True),
    "mixed_5360": lambda: _mixed_charset(),
}


@pytest.mark.parametrize("max_size", [5, 70])
@pytest.mark.parametrize("name", sorted(LABEL_CHARSETS))
def test_label_encoding_matches_string_to_label(name, max_size):
    """N = 9 strings (N * max_size = 630 crosses a 256-thread block at max_size 70, 45 stays inside one at 5): empty, one short of
    / exactly / 9 past max_size, astral codepoints, nothing of the charset, the first and last table entry, the codepoints whose
    upper case is not the inverse of a lower case"""
    cs = LABEL_CHARSETS[name]()
    cps, _ = charset_table(cs)
    rng = np.random.RandomState(max_size)
    pool = [chr(c) for c in cps[rng.randint(0, len(cps), size=200)]] + list("aZ9 ~q中文Kk_0é!abcXYZΑΒΣσςµıſ")

    def rand(n):
        return "".join(pool[j] for j in rng.randint(0, len(pool), size=n))
    texts = ["", rand(max_size - 1), rand(max_size), rand(max_size + 9), "A\U0001F600b\U00020000\U0010FFFFz",
             "Ждßあ￿", chr(int(cps[0])) + chr(int(cps[-1])) + chr(int(cps[0]) - 1) + chr(int(cps[-1]) + 1),
             "ıſµIıSſΜµ", rand(3)]
    images = [np.zeros((2, 2, 3), np.uint8)] * len(texts)
    pipe = DevicePipeline(image_size=(32, 32), mode='resize', charset=cs, max_size=max_size)
    batch = pipe.process(images, texts)
    label, length = batch['label'].cpu().numpy(), batch['length'].cpu().numpy()
    assert label.shape == (9, max_size) and label.dtype == np.int32 and length.dtype == np.int32
    for i, tx in enumerate(texts):
        want = cs.string_to_label(tx, max_size)[:max_size]
        assert np.array_equal(label[i], want), (i, tx, label[i].tolist(), want.tolist())
        assert int(length[i]) == min(len(tx), max_size)
    assert (label[5] == cs.unknown)[:min(5, max_size)].all()                  # a string entirely outside the charset
    assert label[6, 0] == cs.index(chr(int(cps[0]))) != cs.unknown and label[6, 1] == cs.index(chr(int(cps[-1]))) != cs.unknown


def _encode(cps_host, per, table, unknown):
    """mr_encode_labels on strings of `per` codepoints each; table = (codepoints, ids) or None for an empty table"""
    n = len(cps_host) // per
    text = torch.from_numpy(np.asarray(cps_host[:n * per], dtype=np.int32)).to("cuda")
    offs = torch.arange(0, (n + 1) * per, per, dtype=torch.int64, device="cuda")
    label = torch.full((n, per), -7, dtype=torch.int32, device="cuda")
    length = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    tab = [None, None] if table is None else [torch.from_numpy(t).to("cuda") for t in table]
    _lib.call("mr_encode_labels", _lib.ptr(text), _lib.ptr(offs), n, per, _lib.ptr(tab[0]), _lib.ptr(tab[1]),
              0 if table is None else tab[0].numel(), int(unknown), _lib.ptr(label), _lib.ptr(length))
    assert length.cpu().tolist() == [per] * n
    return label.cpu().numpy().reshape(-1)


@pytest.mark.parametrize("name", ["printable", "mixed_5360"])
def test_label_encoding_of_every_codepoint(name):
    """every codepoint outside the surrogates once, 32 to a string: the id is charset.index(chr(cp))"""
    cs = LABEL_CHARSETS[name]()
    every = [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF]
    assert len(every) % 32 == 0
    got = _encode(every, 32, charset_table(cs), cs.unknown)
    index = cs.index
    want = np.array([index(chr(cp)) for cp in every], dtype=np.int32)
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, "%d mismatches, e.g. %s" % (
        wrong.size, [(hex(every[k]), int(want[k]), int(got[k])) for k in wrong[:8]])
    assert int((want != cs.unknown).sum()) == len(charset_table(cs)[0])


def test_label_encoding_with_an_empty_table():
    got = _encode(list(range(48, 48 + 96)), 32, None, 1)
    assert got.tolist() == [1] * 96
    got = _encode(list(range(48, 48 + 96)), 32, None, 37)
    assert got.tolist() == [37] * 96
