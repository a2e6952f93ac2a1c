"""mr_quad_crop (csrc/image_sample.hip) and QuadCropper (data/quad_crop.py) against the numpy restatement of
tests/_quad_crop_ref.py (itself checked on the host in tests/test_quad_crop_cpu.py), BIT FOR BIT: every operation of the kernel
is an IEEE basic operation with contraction off -- the two float64 divisions included, which are correctly rounded on both sides
-- so a mismatch is a wrong operation, not a tolerance.  Outputs are pre-filled with NaN where the test owns them: none may
survive.  Bytes of the source buffer that belong to no photo are 255: a read outside a photo changes the result."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _quad_crop_ref as R  # noqa: E402
from megreader_amd._lib import load, ptr, stream_ptr  # noqa: E402
from megreader_amd.data import DevicePipeline, QuadCropper, plan_crop  # noqa: E402
from megreader_amd.data.quad_crop import CropDesc, CropImage  # noqa: E402

MR_ERR_ARG = 1


def pixels(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert not np.isnan(got).any(), "a pre-filled NaN survived"
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, "%d elements differ, first at %s: %r != %r" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def rotated_box(a, b, angle, centre):
    t = math.radians(angle)
    c, s = math.cos(t), math.sin(t)
    base = np.array([[-a / 2, -b / 2], [a / 2, -b / 2], [a / 2, b / 2], [-a / 2, b / 2]], dtype=np.float64)
    return base @ np.array([[c, s], [-s, c]]) + np.asarray(centre, dtype=np.float64)


SHAPES = [(37, 53), (64, 41)]              # pitches 159 and 123 bytes: odd


def case_plans(canvas):
    """[(photo, CropPlan, mode)]: an upright box, one rotated 30 degrees, a tall one that takes the rotation, two hanging over
    the photo's edge (zero border), a 'pad' crop and a trapezoid in 'quad' mode (true division by D)."""
    cases = [(0, [[5, 4], [45, 4], [45, 20], [5, 20]], 'resize', 'min_area_rect'),
             (1, rotated_box(30, 10, 30, (20, 32)), 'resize', 'min_area_rect'),
             (1, [[10, 5], [22, 5], [22, 55], [10, 55]], 'resize', 'min_area_rect'),
             (0, [[-6, -4], [30, -4], [30, 12], [-6, 12]], 'resize', 'min_area_rect'),
             (1, rotated_box(36, 14, -20, (30, 56)), 'resize', 'min_area_rect'),
             (0, [[8, 10], [28, 10], [28, 22], [8, 22]], 'pad', 'min_area_rect'),
             (0, [[12, 5], [48, 8], [50, 30], [10, 24]], 'resize', 'quad')]
    return [(i, plan_crop(SHAPES[i], q, canvas, mode, rectify), mode) for i, q, mode, rectify in cases]


@pytest.mark.parametrize("canvas", [(8, 24), (32, 128)])
def test_bit_exact_parity(canvas):
    photos = [pixels(s, 3 + k) for k, s in enumerate(SHAPES)]
    plans = case_plans(canvas)
    assert plans[2][1].rotated and not plans[0][1].rotated
    assert abs(plans[6][1].h9[6]) > 1e-4 and abs(plans[6][1].h9[7]) > 1e-4
    if canvas == (32, 128):
        assert plans[5][1].dst_w == 64 < canvas[1]
    want = [R.quad_crop_ref(photos[i], plan) for i, plan, _ in plans]
    # the zero border is really read: some valid pixel of the overhanging crops has a tap outside the photo
    for k in (3, 4):
        x, y, _, _ = R.source_points(plans[k][1])
        assert (x < 0).any() or (y < 0).any() or (x > SHAPES[plans[k][0]][1] - 1).any() or (y > SHAPES[plans[k][0]][0] - 1).any()
    # the entry point itself, rows padded by 5 bytes (pitches 164 and 128)
    got = R.device_crop(photos, [(i, plan) for i, plan, _ in plans], canvas, pad=5)
    for k in range(len(plans)):
        same_bits(got[k], want[k])
    # QuadCropper: photo 0 as numpy (staged), photo 1 as a CUDA tensor (used in place)
    cropper = QuadCropper(image_size=canvas)
    resident = torch.from_numpy(photos[1]).cuda()
    staged, layout = cropper.pack([photos[0], resident], None, plans=[(i, plan) for i, plan, _ in plans])
    assert [r[0] for r in layout.resident] == [1] and layout.resident[0][1].data_ptr() == resident.data_ptr()
    out = cropper.upload(staged, layout)
    torch.cuda.synchronize()
    got = out['image'].cpu().numpy()
    for k in range(len(plans)):
        same_bits(got[k], want[k])
    assert out['index'].cpu().tolist() == [i for i, _, _ in plans]
    assert np.array_equal(out['quad'].cpu().numpy(), np.stack([plan.corners for _, plan, _ in plans]))
    # reported, not gated: how far the fused pass is from the reference's two passes on these crops
    dev = np.concatenate([np.abs(want[k][:, :, :plan.dst_w] - R.two_pass_ref(photos[i], plan, mode)[:, :, :plan.dst_w]).ravel()
                          for k, (i, plan, mode) in enumerate(plans)])
    print("two-pass deviation on the %d x %d test crops (random pixels, normalised units): max %.4f mean %.4f"
          % (canvas[0], canvas[1], dev.max(), dev.mean()))


def test_crop_plans_quads_itself_and_drops_zero_sides():
    photos = [pixels(s, 7 + k) for k, s in enumerate(SHAPES)]
    quads = [np.array([[[5, 4], [45, 4], [45, 20], [5, 20]], [[9, 9], [30, 9], [30, 9], [9, 9]]], dtype=np.float64),
             torch.tensor([[[10.0, 5.0], [22.0, 5.0], [22.0, 55.0], [10.0, 55.0]]])]
    cropper = QuadCropper(image_size=(8, 24), mode='pad')
    out = cropper.crop([torch.from_numpy(photos[0]).cuda(), photos[1]], quads)
    torch.cuda.synchronize()
    assert out['dropped'] == [(0, 1)] and out['index'].cpu().tolist() == [0, 1]
    assert out['quad'].cpu().numpy().tolist() == [quads[0][0].tolist(), quads[1][0].tolist()]
    got = out['image'].cpu().numpy()
    same_bits(got[0], R.quad_crop_ref(photos[0], plan_crop(SHAPES[0], quads[0][0], (8, 24), 'pad')))
    same_bits(got[1], R.quad_crop_ref(photos[1], plan_crop(SHAPES[1], quads[1][0].numpy(), (8, 24), 'pad')))


@pytest.mark.parametrize("down", [1, 2])
def test_slice_equivalence_with_the_resize_pipeline(down):
    """An axis-aligned integer box is the numpy slice: at its own size (sx = sy = 1) and at a 2 x downscale the crop must equal
    `DevicePipeline(mode='resize')` of the slice within 1e-4 (the README's float32 parity bar): that kernel follows cv2's float32
    coefficient arithmetic, this one float64 coordinates.  Measured on an MI355X: 0 at both sizes (CHANGELOG.md)."""
    photo = pixels((64, 96), 11)
    x0, y0, w, h = 8, 10, 64, 32
    canvas = (h // down, w // down)
    box = [[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]]
    plan = plan_crop(photo.shape, box, canvas)
    assert (plan.sx, plan.sy) == (float(down), float(down)) and plan.h9.tolist() == [1, 0, x0, 0, 1, y0, 0, 0, 1]
    got = QuadCropper(image_size=canvas).crop([photo], [[box]])['image']
    want = DevicePipeline(image_size=canvas, mode='resize').process([photo[y0:y0 + h, x0:x0 + w]], [''])['image']
    torch.cuda.synchronize()
    diff = float((got - want).abs().max())
    print("slice equivalence at 1/%d: max |diff| = %.3g" % (down, diff))
    assert got.shape == want.shape == (1, 3) + canvas
    assert diff <= 1e-4


def test_no_crops():
    cropper = QuadCropper(image_size=(8, 24))
    out = cropper.crop([pixels((20, 30), 0)], [[]])
    assert out['image'].shape == (0, 3, 8, 24) and out['index'].shape == (0,) and out['quad'].shape == (0, 4, 2)
    assert cropper.crop([], [])['image'].shape == (0, 3, 8, 24)
    assert load().mr_quad_crop(0, 0, 0, 0, 0, 8, 24, 0.0, 0.0, 0.0, 0, stream_ptr()) == 0        # M = 0: nothing to do


def test_partial_block():
    """M * H * W = 3 * 5 * 7 = 105: one partial block; 2 * 9 * 31 = 558: two full blocks and a partial one."""
    photo = pixels((37, 53), 21)
    for canvas, n in (((5, 7), 3), ((9, 31), 2)):
        plans = [(0, plan_crop(photo.shape, rotated_box(30, 10, 15 * k, (26, 18)), canvas)) for k in range(n)]
        got = R.device_crop([photo], plans, canvas)
        for k, (_, plan) in enumerate(plans):
            same_bits(got[k], R.quad_crop_ref(photo, plan))


def big_batch():
    photo = pixels((720, 1280), 31)
    rng = np.random.RandomState(5)
    quads = [rotated_box(rng.uniform(60, 300), rng.uniform(20, 60), rng.uniform(-30, 30),
                         (rng.uniform(100, 1180), rng.uniform(80, 640))) for _ in range(64)]
    return photo, quads


def test_sixty_four_crops_from_one_photo():
    photo, quads = big_batch()
    out = QuadCropper(image_size=(32, 128)).crop([photo], [quads])
    torch.cuda.synchronize()
    got = out['image'].cpu().numpy()
    assert got.shape == (64, 3, 32, 128)
    for k, q in enumerate(quads):
        same_bits(got[k], R.quad_crop_ref(photo, plan_crop(photo.shape, q, (32, 128))))


def test_run_to_run_equality():
    photo, quads = big_batch()
    cropper = QuadCropper(image_size=(32, 128))
    resident = torch.from_numpy(photo).cuda()
    a = cropper.crop([resident], [quads])['image'].clone()
    b = cropper.crop([resident], [quads])['image']
    assert torch.equal(a, b)


def test_argument_errors():
    lib = load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for i, m, h, w in ((-1, 1, 4, 4), (1, -1, 4, 4), (1, 1, 0, 4), (1, 1, 4, -3), (0, 1, 4, 4), (1, 1 << 20, 64, 64)):
        assert lib.mr_quad_crop(ptr(buf), ptr(buf), i, ptr(buf), m, h, w, 0.0, 0.0, 0.0, ptr(buf), stream_ptr()) == MR_ERR_ARG
        assert b"mr_quad_crop" in lib.mr_last_error()
    for null in range(4):
        p = [ptr(buf)] * 4
        p[null] = 0
        assert lib.mr_quad_crop(p[0], p[1], 1, p[2], 1, 4, 4, 0.0, 0.0, 0.0, p[3], stream_ptr()) == MR_ERR_ARG
    assert lib.mr_sizeof_crop_image() == ctypes.sizeof(CropImage) == 24
    assert lib.mr_sizeof_crop_desc() == ctypes.sizeof(CropDesc) == 112
    with pytest.raises(TypeError):
        QuadCropper(image_size=(8, 24)).crop([np.zeros((4, 4, 3), np.float32)], [[]])
    with pytest.raises(ValueError):
        QuadCropper(image_size=(8, 24)).crop([pixels((9, 9), 0)], [np.zeros((1, 5, 2))])
    with pytest.raises(NotImplementedError):
        QuadCropper(mode='keep_ratio')


def test_out_of_range_image_index():
    """Refused on the host wherever the host can see it -- by `QuadCropper.pack`, and by the entry point when the descriptor table
    lies in pinned host memory -- and by the kernel otherwise: such a crop is the zero pixel, nothing is read."""
    photo = pixels((37, 53), 41)
    plan = plan_crop(photo.shape, [[5, 4], [45, 4], [45, 20], [5, 20]], (8, 24))
    cropper = QuadCropper(image_size=(8, 24))
    for bad in (-1, 1):
        with pytest.raises(ValueError):
            cropper.pack([photo], None, plans=[(bad, plan)])
    lib = load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    descs = (CropDesc * 2)()
    plan.fill(descs[0], 0)
    plan.fill(descs[1], 1)
    pinned = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).pin_memory()
    out = torch.zeros((2, 3, 8, 24), dtype=torch.float32, device="cuda")
    assert lib.mr_quad_crop(ptr(buf), ptr(buf), 1, ptr(pinned), 2, 8, 24, 0.0, 0.0, 0.0, ptr(out), stream_ptr()) == MR_ERR_ARG
    assert b"names photo 1 of 1" in lib.mr_last_error()
    got = R.device_crop([photo], [(0, plan), (0, plan), (0, plan)], (8, 24), images=[0, 7, -1])
    same_bits(got[0], R.quad_crop_ref(photo, plan))
    zero = np.broadcast_to(R.zero_pixel()[:, None, None], (3, 8, 24)).copy()
    same_bits(got[1], zero)
    same_bits(got[2], zero)
