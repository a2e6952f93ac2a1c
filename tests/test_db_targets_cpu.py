"""DB training targets, the parts that need no GPU: the numpy restatement (tests/_db_targets_ref.py) against answers
computed by hand, `DetectionPipeline`'s host packing, and the C header's declarations."""
import ctypes

import numpy as np
import pytest

from _db_targets_ref import db_targets_ref

H, W = 48, 64
RECT = [[10, 10], [50, 10], [50, 30], [10, 30]]          # 40 x 20: D = 0.84 * 800 / 120 = 5.6


def run(quads, tags=None, h=H, w=W, **kw):
    polys = np.asarray(quads, dtype=np.float64).reshape(1, -1, 4, 2)
    g = polys.shape[1]
    tags = np.zeros((1, g), dtype=np.int32) if tags is None else np.asarray(tags, dtype=np.int32).reshape(1, g)
    return db_targets_ref(polys, [g], tags, h, w, **kw)


@pytest.fixture(scope="module")
def rect():
    return run([RECT])


def test_rect_distance_and_shrunk_region(rect):
    assert rect['dist'][0, 0] == 0.84 * 800 / 120 == 5.6
    assert rect['ignore_out'][0, 0] == 0
    # shrunk by 5.6 on every side: x in [15.6, 44.4] -> 16..44 (29), y in [15.6, 24.4] -> 16..24 (9)
    expect = np.zeros((H, W), dtype=np.float32)
    expect[16:25, 16:45] = 1
    assert rect['gt'].sum() == 29 * 9 == 261
    np.testing.assert_array_equal(rect['gt'][0, 0], expect)
    assert rect['mask'].min() == 1.0


def test_rect_grown_region_has_round_corners(rect):
    tm = rect['thresh_mask'][0]
    # corner (10, 10): (6, 7) is at sqrt(16 + 9) = 5 <= 5.6, (6, 6) at sqrt(32) = 5.657 > 5.6; same at the other corners
    for cx, cy, sx, sy in ((10, 10, -1, -1), (50, 10, 1, -1), (50, 30, 1, 1), (10, 30, -1, 1)):
        assert tm[cy + 3 * sy, cx + 4 * sx] == 1.0
        assert tm[cy + 4 * sy, cx + 3 * sx] == 1.0
        assert tm[cy + 4 * sy, cx + 4 * sx] == 0.0
    # straight sides reach floor(5.6) = 5 pixels out
    assert tm[5, 30] == 1.0 and tm[4, 30] == 0.0 and tm[35, 30] == 1.0 and tm[36, 30] == 0.0
    assert tm[20, 5] == 1.0 and tm[20, 4] == 0.0 and tm[20, 55] == 1.0 and tm[20, 56] == 0.0
    # rows 10..30 are 51 wide, and 5 more rows on each side narrow with the arc: 2 * sum_k (41 + 2 floor(sqrt(5.6^2 - k^2)))
    rows = 21 * 51 + 2 * sum(41 + 2 * int(np.sqrt(5.6 ** 2 - k * k)) for k in range(1, 6))
    assert tm.sum() == rows


def test_rect_border_map(rect):
    tm = rect['thresh_map'][0]
    f = np.float32
    top = f(1) * f(0.7 - 0.3) + f(0.3)
    for x, y in ((30, 10), (10, 20), (50, 20), (30, 30), (10, 10)):      # edge pixels and a vertex
        assert tm[y, x] == top
        assert abs(float(tm[y, x]) - 0.7) <= 1.2e-7
    # at distance >= D from every edge: inside the shrunk region and outside the band
    assert tm[20, 30] == f(0.3) and tm[4, 30] == f(0.3) and tm[0, 0] == f(0.3) and tm[20, 16] == f(0.3)
    # mid-band, 3 pixels above the top edge and 3 below it: c = 1 - 3 / 5.6
    mid = (f(1) - f(3 / 5.6)) * f(0.7 - 0.3) + f(0.3)
    assert tm[7, 30] == mid and tm[13, 30] == mid
    assert abs(float(mid) - (0.3 + 0.4 * (1 - 3 / 5.6))) < 1e-7
    assert tm.min() == f(0.3) and tm.max() == top


def test_orientation_does_not_matter():
    quad = [[12.3, 9.1], [48.7, 13.4], [46.2, 33.9], [9.8, 29.5]]
    a, b = run([quad]), run([[quad[0], quad[3], quad[2], quad[1]]])
    assert a['ignore_out'][0, 0] == 0 and a['dist'][0, 0] == b['dist'][0, 0] > 0
    for k in ('gt', 'mask', 'thresh_map', 'thresh_mask'):
        np.testing.assert_array_equal(a[k], b[k])
    assert a['gt'].sum() > 0


def test_small_side_only_zeroes_the_mask():
    r = run([[[10.5, 10.5], [40.5, 10.5], [40.5, 17.5], [10.5, 17.5]]])          # 30 x 7: below min_text_size = 8
    assert r['ignore_out'][0, 0] == 1 and r['dist'][0, 0] == 0.0
    assert r['gt'].sum() == 0 and r['thresh_mask'].sum() == 0 and (r['thresh_map'] == np.float32(0.3)).all()
    expect = np.ones((H, W), dtype=np.float32)
    expect[10:18, 10:41] = 0                                                      # the truncated points (10, 10)..(40, 17), filled
    np.testing.assert_array_equal(r['mask'][0], expect)


def test_pretagged_polygon_is_ignored():
    r = run([RECT], tags=[1])
    assert r['ignore_out'][0, 0] == 1 and r['gt'].sum() == 0
    assert r["mask"][0, 10:31, 10:51].sum() == 0 and r["mask"].sum() == H * W - 21 * 41


def test_overhanging_quad_is_clipped_first():
    over = [[40, -10], [90, -10], [90, 20], [40, 20]]
    clipped = [[40, 0], [W - 1, 0], [W - 1, 20], [40, 20]]
    a, b = run([over]), run([clipped])
    assert a['dist'][0, 0] == b['dist'][0, 0] == 0.84 * (23 * 20) / (2 * 23 + 2 * 20)
    for k in ('gt', 'mask', 'thresh_map', 'thresh_mask'):
        np.testing.assert_array_equal(a[k], b[k])
    assert a['gt'].sum() > 0


def test_empty_image():
    r = db_targets_ref(np.zeros((1, 0, 4, 2)), [0], np.zeros((1, 0), np.int32), 5, 7)
    assert r['gt'].sum() == 0 and r['mask'].min() == 1 and r['thresh_mask'].sum() == 0
    assert (r['thresh_map'] == np.float32(0.3)).all()


# ---- DetectionPipeline: host packing ------------------------------------------------------------------------------------

def _pipe(**kw):
    from megreader_amd.data import DetectionPipeline
    return DetectionPipeline(image_size=(6, 10), **kw)


def _images(n):
    rng = np.random.RandomState(0)
    return [rng.randint(0, 256, (6, 10, 3)).astype(np.uint8) for _ in range(n)]


def _views(buf, layout):
    n, G, desc_off, poly_off, count_off, tag_off = layout
    host = buf.numpy()
    return (host[poly_off:poly_off + n * G * 64].view(np.float64).reshape(n, G, 4, 2),
            host[count_off:count_off + n * 4].view(np.int32), host[tag_off:tag_off + n * G * 4].view(np.int32).reshape(n, G))


def test_pack_layout_counts_and_tags():
    from megreader_amd.data.device_pipeline import ImgDesc
    images = _images(3)
    q = np.arange(16, dtype=np.float64).reshape(2, 4, 2)
    buf, layout = _pipe().pack(images, [q, np.zeros((0, 4, 2)), q[:1] + 0.5], [[False, True], [], [True]])
    n, G, desc_off, poly_off, count_off, tag_off = layout
    assert (n, G) == (3, 2) and buf.dtype.is_floating_point is False and buf.numel() >= tag_off + 3 * 2 * 4
    assert poly_off % 16 == 0 and count_off % 16 == 0 and tag_off % 16 == 0
    polys, count, tags = _views(buf, layout)
    np.testing.assert_array_equal(count, [2, 0, 1])
    np.testing.assert_array_equal(tags, [[0, 1], [0, 0], [1, 0]])
    np.testing.assert_array_equal(polys[0], q)
    np.testing.assert_array_equal(polys[1], 0)
    np.testing.assert_array_equal(polys[2, 0], q[0] + 0.5)
    np.testing.assert_array_equal(polys[2, 1], 0)
    descs = (ImgDesc * 3).from_buffer_copy(buf.numpy()[desc_off:desc_off + 3 * ctypes.sizeof(ImgDesc)].tobytes())
    for i, im in enumerate(images):
        assert (descs[i].h, descs[i].w, descs[i].pitch, descs[i].dst_w) == (6, 10, 30, 10)
        assert descs[i].scale_x == 1.0 and descs[i].scale_y == 1.0
        np.testing.assert_array_equal(buf.numpy()[descs[i].offset:descs[i].offset + 180], im.reshape(-1))


def test_pack_rejects_five_point_polygons():
    with pytest.raises(ValueError):
        _pipe().pack(_images(1), [np.zeros((1, 5, 2))], [[False]])
    with pytest.raises(ValueError):
        _pipe().pack(_images(1), [np.zeros((2, 4, 2))], [[False]])              # tags do not match


def test_pack_padding_boundaries():
    buf, layout = _pipe().pack(_images(2), [[], []], [[], []])                   # G = 0
    assert layout[:2] == (2, 0)
    polys, count, tags = _views(buf, layout)
    assert polys.shape == (2, 0, 4, 2) and tags.shape == (2, 0)
    np.testing.assert_array_equal(count, [0, 0])
    q = np.ones((3, 4, 2))
    buf, layout = _pipe(max_polygons=3).pack(_images(2), [q, q[:1]], [[0, 0, 1], [0]])   # G = max: the first image is full
    assert layout[:2] == (2, 3)
    polys, count, tags = _views(buf, layout)
    np.testing.assert_array_equal(count, [3, 1])
    np.testing.assert_array_equal(tags, [[0, 0, 1], [0, 0, 0]])
    assert polys[0].min() == 1 and polys[1, 1:].max() == 0
    with pytest.raises(ValueError):
        _pipe(max_polygons=2).pack(_images(2), [q, q[:1]], [[0, 0, 1], [0]])
    with pytest.raises(ValueError):
        _pipe(max_polygons=1025)
    full = np.ones((1024, 4, 2))
    buf, layout = _pipe().pack(_images(1), [full], [np.zeros(1024)])
    assert layout[:2] == (1, 1024)
    with pytest.raises(ValueError):
        _pipe().pack(_images(1), [np.ones((1025, 4, 2))], [np.zeros(1025)])


# ---- header ---------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    from megreader_amd import _lib
    ret, args, streamed = _lib.FUNCTIONS["mr_db_targets"]
    assert ret is ctypes.c_int and streamed and len(args) == 19
    assert args[3:7] == [ctypes.c_int] * 4 and args[7:11] == [ctypes.c_double] * 4
    ret, args, streamed = _lib.FUNCTIONS["mr_sizeof_db_record"]
    assert ret is ctypes.c_int and args == [] and not streamed
