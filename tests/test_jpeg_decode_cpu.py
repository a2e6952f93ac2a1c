"""Host side of the GPU JPEG decoder, no GPU needed: the numpy restatement (tests/_jpeg_ref.py) against PIL bit for bit, the
host plan `mr_jpeg_plan` (csrc/jpeg_plan.h) against the restatement's parse, its behaviour on damaged input, and the sources
that can hand over bytes instead of pixels."""
import ctypes
import glob
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import _jpeg_ref as ref  # noqa: E402
from megreader_amd.data import jpeg_decode as jd  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
NAMES = sorted(os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(GOLDEN, "*.jpg")))


def blob_of(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def pil_bgr(blob):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(blob)).convert('RGB'))[:, :, ::-1]


def test_fixtures_cover_the_axes():
    assert len(NAMES) >= 12
    parsed = {n: ref.parse(blob_of(n)) for n in NAMES}
    assert all(p.status == ref.OK for p in parsed.values())
    assert {(p.ncomp, p.hs, p.vs) for p in parsed.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {(p.w, p.h) for p in parsed.values()} >= {(1, 1), (2, 2), (3, 3), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33),
                                                      (100, 32), (101, 33), (256, 64), (300, 200)}
    assert sum(len(p.items) > 1 for p in parsed.values()) >= 4           # restart intervals of 1 and 3 MCUs and of MCU rows
    assert {p.restart for p in parsed.values()} >= {0, 1, 3}
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".jpg")) < 16384 for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pil_on_fixture(name):
    pytest.importorskip("PIL")
    blob = blob_of(name)
    out = ref.decode(blob)
    want = pil_bgr(blob)
    assert out.shape == want.shape and out.dtype == np.uint8
    assert np.array_equal(out, want)
    assert np.array_equal(ref.decode(blob, rgb=True), want[:, :, ::-1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_pil_on_a_random_matrix(seed):
    pytest.importorskip("PIL")
    from make_jpeg_fixtures import content, encode
    sizes = ((1, 1), (2, 2), (3, 3), (4, 4), (5, 2), (6, 7), (7, 5), (9, 17), (33, 17), (40, 24))
    for w, h in sizes:
        for sub in (0, 1, 2):
            for quality, options in ((30, {}), (75, dict(optimize=True)), (95, dict(restart_marker_blocks=2)), (100, {})):
                blob = encode(content(w, h, seed * 1000 + 7 * w + h), subsampling=sub, quality=quality, **options)
                assert np.array_equal(ref.decode(blob), pil_bgr(blob)), (w, h, sub, quality, options)
        gray = encode(content(w, h, seed * 1000 + w, 1), "L", quality=75)
        assert np.array_equal(ref.decode(gray), pil_bgr(gray)), (w, h)


def _unpacked(image):
    """The tables of one mr_jpeg_image as the restatement holds them."""
    quant = np.frombuffer(image, dtype=np.uint8, count=256, offset=type(image).quant.offset).reshape(4, 64)
    syms = np.frombuffer(image, dtype=np.uint8, count=1024, offset=type(image).huff_sym.offset).reshape(4, 256)
    maxcode = np.array(image.huff_maxcode).reshape(4, 16)
    valoff = np.array(image.huff_valoff).reshape(4, 16)
    return quant, syms, maxcode, valoff


def test_plan_equals_the_restatements_parse():
    blobs = [blob_of(n) for n in NAMES]
    plan = jd.make_plan(blobs)
    assert plan.status == [jd.OK] * len(blobs)
    assert (jd.OK, jd.UNSUPPORTED, jd.CORRUPT) == (ref.OK, ref.UNSUPPORTED, ref.CORRUPT)
    n_items = 0
    for blob, im in zip(blobs, plan.images):
        p = ref.parse(blob)
        assert (im.h, im.w, im.ncomp, im.hs, im.vs, im.restart) == (p.h, p.w, p.ncomp, p.hs, p.vs, p.restart)
        assert (im.mcu_w, im.mcu_h, im.scan_off, im.scan_len, im.blob_len) == (p.mcu_w, p.mcu_h, p.scan_off, p.scan_len, len(blob))
        assert list(im.comp_tq)[:p.ncomp] == p.comp_tq and list(im.comp_td)[:p.ncomp] == p.comp_td
        assert list(im.comp_ta)[:p.ncomp] == p.comp_ta
        quant, syms, maxcode, valoff = _unpacked(im)
        for t, q in p.quant.items():
            assert np.array_equal(quant[t], q)
        for t, (mc, vo, sy) in p.huff.items():
            assert list(maxcode[t]) == mc[1:] and list(valoff[t]) == vo[1:]
            assert bytes(syms[t][:len(sy)]) == bytes(sy) and not syms[t][len(sy):].any()
        assert im.first_item == n_items and im.n_items == len(p.items)
        items = [plan.items[k] for k in range(im.first_item, im.first_item + im.n_items)]
        assert [(it.mcu0, it.nmcu, it.off, it.len) for it in items] == p.items
        n_items += im.n_items
    assert plan.n_items == n_items > len(blobs)                          # the restart fixtures: more items than images
    for i, im in enumerate(plan.images):
        assert all(plan.items[k].image == i for k in range(im.first_item, im.first_item + im.n_items))


def _check_inside(plan, lens):
    """Every offset and length of an OK image lies inside the blob, the workspace and the output totals."""
    for i, im in enumerate(plan.images):
        assert im.blob_off % 16 == 0 and 0 <= im.blob_off and im.blob_off + lens[i] <= plan.blob_bytes
        if im.status != jd.OK:
            continue
        assert im.h > 0 and im.w > 0 and im.ncomp in (1, 3)
        assert 0 <= im.scan_off and 0 <= im.scan_len and im.scan_off + im.scan_len <= lens[i]
        for c in range(im.ncomp):
            nbytes = im.plane_pitch[c] * im.plane_rows[c]
            assert im.plane_off[c] % 16 == 0 and 0 <= im.plane_off[c] and im.plane_off[c] + nbytes <= plan.workspace_bytes
            assert im.plane_pitch[c] == im.mcu_w * 8 * (im.hs if c == 0 else 1)
            assert im.plane_rows[c] == im.mcu_h * 8 * (im.vs if c == 0 else 1)
            assert 0 <= im.comp_tq[c] <= 3 and 0 <= im.comp_td[c] <= 1 and 0 <= im.comp_ta[c] <= 1
        assert im.plane_pitch[0] >= im.w and im.plane_rows[0] >= im.h
        assert im.out_off % 16 == 0 and 0 <= im.out_off and im.out_off + im.h * im.w * 3 <= plan.out_bytes
        assert 0 <= im.first_item and im.n_items >= 1 and im.first_item + im.n_items <= plan.n_items
        mcu = 0
        for k in range(im.first_item, im.first_item + im.n_items):
            it = plan.items[k]
            assert it.image == i and it.mcu0 == mcu and it.nmcu >= 1
            assert im.scan_off <= it.off and 0 <= it.len and it.off + it.len <= im.scan_off + im.scan_len
            mcu += it.nmcu
        assert mcu == im.mcu_w * im.mcu_h


def test_what_the_device_does_not_decode():
    pytest.importorskip("PIL")
    from PIL import Image
    from make_jpeg_fixtures import content
    pix = content(24, 16, 5)

    def save(image, fmt, **options):
        buf = io.BytesIO()
        image.save(buf, fmt, **options)
        return buf.getvalue()
    progressive = save(Image.fromarray(pix), "JPEG", progressive=True)
    cmyk = save(Image.fromarray(pix).convert("CMYK"), "JPEG")
    png = save(Image.fromarray(pix), "PNG")
    good = blob_of("c420_9x17_q75_opt")
    blobs = [progressive, cmyk, png, b'', b'\xff\xd8', good, good[:40]]
    plan = jd.make_plan(blobs)
    assert plan.status == [jd.UNSUPPORTED, jd.UNSUPPORTED, jd.UNSUPPORTED, jd.UNSUPPORTED, jd.CORRUPT, jd.OK, jd.CORRUPT]
    assert [ref.parse(b).status for b in blobs] == plan.status
    _check_inside(plan, [len(b) for b in blobs])
    assert plan.n_items == 1 and plan.images[5].out_off == 0 and plan.images[5].plane_off[0] == 0   # only OK images get room


@pytest.mark.parametrize("name", ["c420_9x17_q75_opt", "c422_17x33_q75_rst1"])
def test_every_prefix_plans_without_a_crash(name):
    blob = blob_of(name)
    prefixes = [blob[:k] for k in range(len(blob))]
    plan = jd.make_plan(prefixes)                                         # one call, hundreds of broken files
    _check_inside(plan, [len(p) for p in prefixes])
    status = plan.status
    assert status[0] == jd.UNSUPPORTED and status[1] == jd.UNSUPPORTED and status[2] == jd.CORRUPT
    scan_off = ref.parse(blob).scan_off
    assert all(s == jd.CORRUPT for s in status[2:scan_off])               # a header that stops short
    for k in (2, 3, scan_off - 1, scan_off, scan_off + 1, len(blob) - 3, len(blob) - 1):
        assert ref.parse(prefixes[k]).status == status[k], k


@pytest.mark.parametrize("name", NAMES)
def test_every_header_byte_altered(name):
    blob = blob_of(name)
    header = ref.parse(blob).scan_off
    altered = []
    for at in range(header):
        for value in (0x00, 0xFF, blob[at] ^ 0xFF):
            altered.append(blob[:at] + bytes([value]) + blob[at + 1:])
    plan = jd.make_plan(altered)
    _check_inside(plan, [len(b) for b in altered])
    for k in range(0, len(altered), 97):                                  # a sample of them against the restatement's parse
        p = ref.parse(altered[k])
        assert p.status == plan.status[k], k
        if p.status == ref.OK:
            im = plan.images[k]
            assert (im.h, im.w, im.ncomp, im.hs, im.vs, im.restart, im.n_items) == (p.h, p.w, p.ncomp, p.hs, p.vs, p.restart,
                                                                                     len(p.items))


def test_plan_asks_for_a_second_call_when_items_do_not_fit():
    blob = blob_of("c422_17x33_q75_rst1")                                 # 10 restart intervals
    n = 40
    lib = jd.load()
    ptrs = (ctypes.c_char_p * n)(*([blob] * n))
    lens = (ctypes.c_longlong * n)(*([len(blob)] * n))
    images = (jd.JpegImage * n)()
    items = (jd.JpegItem * 16)()
    totals = (ctypes.c_longlong * 4)()
    assert lib.mr_jpeg_plan(n, ptrs, lens, images, items, 15, totals) == 0
    assert totals[0] == 400 and items[15].nmcu == 0 and items[14].nmcu == 1          # counted, not written past the room
    assert jd.make_plan([blob] * n).n_items == 400                                   # (make_plan starts with room for n + 256)


def test_sources_hand_over_bytes_untouched(tmp_path):
    msgpack = pytest.importorskip("msgpack")
    pytest.importorskip("PIL")
    from megreader_amd.data import lmdb_reader
    from megreader_amd.data.msgpack_records import UnpackMsgpackData
    blob = blob_of("c420_100x32_q75")
    record = msgpack.dumps({b'img': blob, b'gt': b'word'})
    kept = UnpackMsgpackData(decode_images=False).convert(record)
    assert kept['img'] == blob and isinstance(kept['img'], bytes) and kept['gt'] == 'word'
    default = UnpackMsgpackData().convert(record)
    assert default['img'].dtype == np.uint8 and np.array_equal(default['img'], pil_bgr(blob))
    assert np.array_equal(UnpackMsgpackData(mode='RGB').convert(record)['img'], pil_bgr(blob)[:, :, ::-1])
    path = str(tmp_path / "db")
    lmdb_reader.write_environment(path, {b'image': {b'id-1': blob}})
    store = lmdb_reader.LMDBImageStore(path)
    try:
        meta = store.default_unpack('id-1', {'db_path': path}, decode=False)
        assert meta['image_bytes'] == blob and 'image' not in meta
        meta = store.default_unpack('id-1', {'db_path': path})
        assert np.array_equal(meta['image'], pil_bgr(blob)) and 'image_bytes' not in meta
    finally:
        store.close()
