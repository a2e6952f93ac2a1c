"""mr_warp_normalize (csrc/image_sample.hip) against the numpy restatement of tests/_db_augment_ref.py (itself checked on the
host in tests/test_db_augment_cpu.py), BIT FOR BIT: every operation of the kernel is an IEEE basic operation with contraction
off, so a mismatch is a wrong operation order, not a tolerance.  Outputs are pre-filled with NaN: none may survive.  Bytes of
the source buffer that belong to no window are 255: a read outside a window changes the result."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _db_augment_ref as R  # noqa: E402
from megreader_amd._lib import call, load, ptr, stream_ptr  # noqa: E402
from megreader_amd.data import DetectionAugmenter, WarpDesc  # noqa: E402
from megreader_amd.data.device_pipeline import ImgDesc  # noqa: E402

MR_ERR_ARG = 1


def pixels(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert not np.isnan(got).any(), "a pre-filled NaN survived"
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, "%d elements differ, first at %s: %r != %r" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def normalised(hwc):
    """uint8 [H, W, 3] -> f32 [3, H, W] as normalize_image.py does."""
    v = (hwc.astype(np.float64) - np.array(R.RGB_MEAN)).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def check(sources, plans, canvas, **kw):
    got = R.device_warp(sources, plans, canvas, **kw)
    for i, (src, plan) in enumerate(zip(sources, plans)):
        same_bits(got[i], R.warp_normalize_ref(src, plan, canvas, window=(kw.get('windows') or [None] * len(plans))[i])['image'])
    return got


def resize_normalize(src, H, W, dst_w):
    """mr_resize_normalize at identity scale (mode "pad" when dst_w < W)."""
    dev = torch.device("cuda")
    d = ImgDesc()
    d.offset, d.h, d.w, d.pitch, d.dst_w, d.scale_x, d.scale_y = 0, src.shape[0], src.shape[1], src.shape[1] * 3, dst_w, 1.0, 1.0
    d_src = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(d), dtype=np.uint8).copy()).to(dev)
    out = torch.full((1, 3, H, W), float('nan'), dtype=torch.float32, device=dev)
    call("mr_resize_normalize", ptr(d_src), ptr(d_desc), 1, H, W, R.RGB_MEAN[0], R.RGB_MEAN[1], R.RGB_MEAN[2], ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


def test_identity_equals_resize_normalize():
    H, W = 64, 96
    src = pixels((H, W), 0)
    plan = DetectionAugmenter(size=(W, H)).plan((H, W))
    got = check([src], [plan], (H, W))[0]
    same_bits(got, resize_normalize(src, H, W, W))
    same_bits(got, normalised(src))


def test_padding_equals_resize_normalize_in_mode_pad():
    H, W = 64, 96
    src = pixels((H, 80), 1)                                           # valid 80 x 64 of the 96 x 64 canvas
    plan = DetectionAugmenter(size=(W, H)).plan((H, 80))
    assert plan.valid == (80, H)
    got = check([src], [plan], (H, W))[0]
    same_bits(got, resize_normalize(src, H, W, 80))
    low = DetectionAugmenter(size=(W, H)).plan((30, 96))                # valid 96 x 30: the rows below are padding
    assert low.valid == (96, 30)
    got = check([pixels((30, 96), 2)], [low], (H, W))[0]
    same_bits(got[:, 30:], np.broadcast_to(R.zero_pixel()[:, None, None], (3, H - 30, W)).copy())


def test_pure_flip():
    H, W = 64, 96
    src = pixels((H, W), 3)
    got = check([src], [DetectionAugmenter(size=(W, H)).plan((H, W), flip=True)], (H, W))[0]
    same_bits(got, normalised(src[:, ::-1]))


def test_integer_translation_is_the_slice():
    H, W = 64, 96
    src = pixels((80, 120), 4)
    plan = DetectionAugmenter(size=(W, H)).plan((80, 120), crop=(10, 7, W, H))
    assert plan.valid == (W, H)
    got = check([src], [plan], (H, W))[0]
    same_bits(got, normalised(src[7:7 + H, 10:10 + W]))


@pytest.mark.parametrize("k", range(7))
def test_case_plans_on_random_pixels(k):
    check([pixels(R.CASE_SHAPE, 10 + k)], [R.case_plans()[k]], R.CASE_CANVAS)


@pytest.mark.parametrize("canvas", [(1, 1), (5, 7), (64, 96)])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (37, 53)])
def test_canvas_and_source_sizes(canvas, shape):
    """Canvases 1 x 1, 5 x 7 (one partial block) and 64 x 96 (24 blocks; neither a multiple of 256 threads nor, per row, of
    a wavefront); sources down to one pixel.  Plans: the seven of the consistency case for this shape, four sampled ones and the validation resize."""
    src = pixels(shape, 20 + shape[0])
    size = (canvas[1], canvas[0])
    aug = DetectionAugmenter(size=size, seed=5)
    quad = np.array([[[0.2, 0.2], [0.7, 0.25], [0.65, 0.6], [0.15, 0.55]]]) * (shape[1], shape[0])
    plans = R.case_plans(shape, canvas, quad, [False]) + [aug.sample(shape, quad, [False]) for _ in range(4)]
    plans.append(DetectionAugmenter.resize_to(size[0], size[1], shape))
    check([src] * len(plans), plans, canvas)


def test_width_not_a_multiple_of_four():
    canvas = (33, 98)                                                    # odd height, rows that straddle wavefronts
    plans = R.case_plans(R.CASE_SHAPE, canvas)
    check([pixels(R.CASE_SHAPE, 30)] * len(plans), plans, canvas)


def test_three_sources_in_one_call():
    canvas = (64, 96)
    shapes = [(48, 80), (37, 53), (90, 61)]
    aug = DetectionAugmenter(size=(96, 64))
    plans = [aug.plan(shapes[0], flip=True, angle=-10.0, scale=0.5),
             aug.plan(shapes[1], angle=7.0, scale=3.0, crop=R.middle_crop(shapes[1], 3.0)),
             aug.plan(shapes[2], angle=3.0, scale=1.3)]
    check([pixels(s, 40 + i) for i, s in enumerate(shapes)], plans, canvas)


def test_padded_pitch():
    plans = R.case_plans()[3:6]
    check([pixels(R.CASE_SHAPE, 50)] * 3, plans, R.CASE_CANVAS, pad=5)


def test_window_upload_equals_full_upload():
    src = pixels(R.CASE_SHAPE, 60)
    plans = R.case_plans()
    assert any(p.window != (0, 0, 80, 48) for p in plans)
    part = check([src] * 7, plans, R.CASE_CANVAS)
    full = check([src] * 7, plans, R.CASE_CANVAS, windows=[(0, 0, 80, 48)] * 7)
    same_bits(part, full)


def test_no_images_and_bad_shapes():
    lib = load()
    assert lib.mr_warp_normalize(0, 0, 0, 64, 96, 0.0, 0.0, 0.0, 0, stream_ptr()) == 0          # N = 0: nothing to do
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for n, h, w in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, -3)):
        assert lib.mr_warp_normalize(ptr(buf), ptr(buf), n, h, w, 0.0, 0.0, 0.0, ptr(buf), stream_ptr()) == MR_ERR_ARG
        assert b"mr_warp_normalize" in lib.mr_last_error()
    assert lib.mr_warp_normalize(0, ptr(buf), 1, 4, 4, 0.0, 0.0, 0.0, ptr(buf), stream_ptr()) == MR_ERR_ARG
    assert lib.mr_sizeof_warp_desc() == ctypes.sizeof(WarpDesc) == 128
