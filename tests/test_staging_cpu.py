"""The staging buffers of the three input pipelines (megreader_amd/data/staging.py), host only.

The SHA-256 values, sizes, layouts and plan parameters below are LITERALS recorded from a build of the commit before the three
`pack` methods moved onto the shared helper -- not from the code under test -- for fixed seeded inputs: the staged byte stream
(section order, padding, `offset` fields, table contents, the zero fill of the polygon, count and tag sections) must not move.
Bytes between sections belong to nobody: every case packs twice into one slot with the buffer set to 0xA5 in between, so that
what the packer leaves alone is known.  (`DevicePipeline.pack` needs a device for its charset tables: its hash is pinned in
tests/test_pipeline_gpu.py.)"""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from megreader_amd.data import DetectionAugmenter, DetectionPipeline, QuadCropper
from megreader_amd.data.device_pipeline import ImgDesc
from megreader_amd.data.staging import Sections, Staging, as_quads, check_images


def poisoned(pack):
    staged, _ = pack()
    staged.fill_(0xA5)
    staged, layout = pack()
    return hashlib.sha256(staged.numpy().tobytes()).hexdigest(), int(staged.numel()), layout


# ---- DetectionPipeline.pack: three 8 x 12 images with 2, 0 and 1 quads, mixed tags ---------------------------------------------

def detection_inputs():
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (8, 12, 3)).astype(np.uint8) for _ in range(3)]
    q = np.array([[[1.0, 1.0], [6.5, 1.25], [6.0, 4.0], [1.5, 3.75]], [[7.0, 2.0], [11.0, 2.5], [10.5, 6.0], [7.25, 5.5]]])
    return images, [q, np.zeros((0, 4, 2)), q[1:] - 0.5], [[False, True], [], [True]]


def test_detection_pack_bytes_are_the_parents():
    images, polys, tags = detection_inputs()
    pipe = DetectionPipeline(image_size=(8, 12), device='cpu')
    assert poisoned(lambda: pipe.pack(images, polys, tags)) == (
        "71a60bd94bb80ac771b2e535bff25876eee4c8fe18b7adbb8b2a59d889c735bb", 1424, (3, 2, 864, 992, 1376, 1392))
    pipe = DetectionPipeline(image_size=(8, 12), max_polygons=3, device='cpu')
    assert poisoned(lambda: pipe.pack(images, polys, tags)) == (
        "f751ee7d96f9fb0640c4eda73a3681b3e1ee9caf72653fbe4fa27eaaa7881f1f", 1632, (3, 3, 864, 992, 1568, 1584))


PLAN_PARAMS = [dict(flip=True, angle=10.0, scale=1.5, crop=(2, 1, 12, 8)), dict(flip=False, angle=-7.5, scale=0.75, crop=None),
               dict(flip=False, angle=0.0, scale=2.0, crop=(5, 3, 18, 12))]
#               resized, crop, valid, window, kept, clamp and pixels_inv (float.hex) of the three plans at the parent
PARENT_PLANS = [
    ((12, 18), (2, 1, 12, 8), (12, 8), (1, 0, 11, 8), [0, 1],
     ['0x0.0p+0', '0x1.6000000000000p+3', '0x0.0p+0', '0x1.c000000000000p+2'],
     ['-0x1.5025d085612bap-1', '-0x1.da2cdfd649a0cp-4', '0x1.493af094b8107p+3', '-0x1.da2cdfd649a0cp-4', '0x1.5025d085612bap-1', '0x1.4c4d25c2f3474p+0']),
    ((6, 9), (0, 0, 9, 6), (12, 8), (0, 0, 12, 8), [],
     ['0x1.5555555555554p-3', '0x1.5aaaaaaaaaaabp+3', '0x1.5555555555554p-3', '0x1.b555555555555p+2'],
     ['0x1.fb9ea92ec689ap-1', '-0x1.0b5150f6da2d0p-3', '0x1.01fe8456baf1ep-1', '0x1.0b5150f6da2d0p-3', '0x1.fb9ea92ec689ap-1', '-0x1.603b1f7722e00p-1']),
    ((16, 24), (5, 3, 18, 12), (12, 8), (1, 0, 11, 8), [0],
     ['-0x1.5555555555556p-3', '0x1.6555555555555p+3', '-0x1.5555555555556p-3', '0x1.caaaaaaaaaaabp+2'],
     ['0x1.8000000000000p-1', '0x0.0p+0', '0x1.3000000000000p+1', '0x0.0p+0', '0x1.8000000000000p-1', '0x1.6000000000000p+0']),
]


def test_detection_pack_with_plans_bytes_are_the_parents():
    images, polys, tags = detection_inputs()
    aug = DetectionAugmenter(size=(12, 8))
    plans = [aug.plan(im.shape, p, t, **kw) for im, p, t, kw in zip(images, polys, tags, PLAN_PARAMS)]
    for plan, (resized, crop, valid, window, kept, clamp, pixels_inv) in zip(plans, PARENT_PLANS):
        assert (plan.resized, plan.crop, plan.valid, plan.window, plan.kept.tolist()) == (resized, crop, valid, window, kept)
        assert [float(c).hex() for c in plan.clamp] == clamp and [float(a).hex() for a in plan.pixels_inv] == pixels_inv
    pipe = DetectionPipeline(image_size=(8, 12), device='cpu')
    assert poisoned(lambda: pipe.pack(images, polys, tags, plans=plans)) == (
        "d8d5c62053d65d97e96ccdb229f0bb515df62528069532978d13a922e38cd6ae", 1648, (3, 2, 832, 1216, 1600, 1616, 'warp'))


# ---- QuadCropper.pack: photos of 9 x 14 and 16 x 10 with 2 and 1 quads, one of them with a zero side ---------------------------

@pytest.mark.parametrize("mode,sha,dst_w", [
    ("resize", "8382703550a353fb5621389220ea413d724d0940d4fa8ba15e4d7a79143eb39a", 64),
    ("pad", "424ab3ec05af7cf61802a27e051c1826fafc4376a9664a18a58d5715a1f702d5", 32)])
def test_crop_pack_bytes_are_the_parents(mode, sha, dst_w):
    rng = np.random.RandomState(1)
    photos = [rng.randint(0, 256, (9, 14, 3)).astype(np.uint8), rng.randint(0, 256, (16, 10, 3)).astype(np.uint8)]
    quads = [np.array([[[2.0, 1.0], [11.0, 2.0], [10.5, 6.0], [1.5, 5.0]], [[3.0, 3.0]] * 4]),
             np.array([[[2.0, 2.0], [7.0, 3.0], [6.0, 13.0], [1.0, 12.0]]])]
    cropper = QuadCropper(image_size=(8, 64), mode=mode, device='cpu')
    got, nbytes, lay = poisoned(lambda: cropper.pack(photos, quads))
    assert (got, nbytes) == (sha, 1280)
    assert tuple(lay[:6]) == (2, 2, 864, 912, 1136, 1152) and lay.resident == [] and lay.dropped == [(0, 1)]
    assert [(p.dst_w, p.rotated) for p in lay.plans] == [(dst_w, False), (dst_w, True)]


# ---- the helper itself -------------------------------------------------------------------------------------------------------

def test_sections_are_aligned_and_do_not_overlap():
    descs = (ImgDesc * 3)()                                                     # 120 bytes
    sections = [np.zeros((5, 7, 3), np.uint8), 0, descs, np.arange(3, dtype=np.int64), 7, np.zeros(0, np.int32), 33]
    sizes = [105, 0, 120, 24, 7, 0, 33]
    lay = Sections(sections)
    assert lay.offsets == [0, 112, 112, 240, 272, 288, 288] and lay.total == 321
    assert Sections(sections, pad_end=True).total == 336 and Sections([]).total == 0
    assert all(off % 16 == 0 for off in lay.offsets)
    assert all(a + n <= b for a, n, b in zip(lay.offsets, sizes, lay.offsets[1:] + [lay.total]))
    descs[2].offset, descs[2].scale_y = 1 << 40, 0.1
    staged, views = Staging().stage(0, lay)
    assert staged.dtype.is_floating_point is False and staged.numel() == 321 and [len(v) for v in views] == sizes
    assert bytes(views[2]) == bytes(descs) and views[3].view(np.int64).tolist() == [0, 1, 2]
    host = staged.numpy()
    assert all(np.shares_memory(v, host) for v in views if len(v))
    picture = np.arange(9 * 4 * 3, dtype=np.uint8).reshape(9, 4, 3)[1:8:2, 1:3]           # strided: copied as it reads
    _, views = Staging().stage(0, Sections([picture]))
    np.testing.assert_array_equal(views[0].reshape(4, 2, 3), picture)


def test_slots_grow_and_are_reused():
    staging = Staging()
    a, _ = staging.stage(0, Sections([100]))
    b, _ = staging.stage(0, Sections([40]))                                     # smaller: the same buffer
    assert b.data_ptr() == a.data_ptr() and b.numel() == 40
    c, _ = staging.stage(1, Sections([100]))                                    # another slot: another buffer
    assert c.data_ptr() != a.data_ptr()
    a.fill_(1)
    c.fill_(2)
    assert int(a.sum()) == 100
    d, _ = staging.stage(0, Sections([101]))                                    # larger: reallocated
    assert d.numel() == 101 and staging.buffer(0, 1).numel() >= 101
    assert staging.stage(0, Sections([100]))[0].data_ptr() == d.data_ptr()
    assert staging.stage(1, Sections([5]))[0].data_ptr() == c.data_ptr()
    assert staging.stage(2, Sections([]))[0].numel() == 0


def test_one_image_check_and_one_quad_check():
    good = np.zeros((4, 5, 3), np.uint8)
    check_images([good, good[:, ::2]])
    for bad in (good.astype(np.float32), good[..., :2], good[0], torch.zeros((4, 5, 3), dtype=torch.uint8)):
        with pytest.raises(TypeError, match="images must be uint8 HWC with 3 channels"):
            check_images([good, bad])
    check_images([torch.zeros((4, 5, 3), dtype=torch.uint8)], tensors=True)
    with pytest.raises(TypeError):
        check_images([torch.zeros((4, 5, 3))], tensors=True)
    assert as_quads([], "X takes").shape == (0, 4, 2) and as_quads(torch.zeros(2, 4, 2), "X takes").dtype == np.float64
    assert as_quads(np.zeros((0, 3)), "X takes").shape == (0, 4, 2)
    for bad in (np.zeros((1, 5, 2)), np.zeros((4, 2)), np.zeros((0, 4, 3)), np.zeros((2, 0, 2))):
        with pytest.raises(ValueError, match="X takes quadrilaterals: expected K x 4 x 2 points per image"):
            as_quads(bad, "X takes")
