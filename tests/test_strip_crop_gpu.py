"""`mr_strip_crop` (csrc/image_sample.hip) against its restatement tests/_strip_crop_ref.py BIT FOR BIT, `mr_quad_crop` beside it
where the strip is a box, and `StripCropper` over it."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _quad_crop_ref as Q  # noqa: E402
import _strip_crop_ref as S  # noqa: E402
from megreader_amd._lib import load, ptr, stream_ptr  # noqa: E402
from megreader_amd.data.quad_crop import plan_crop  # noqa: E402
from megreader_amd.data.strip_crop import StripCropper, plan_strip  # noqa: E402
from megreader_amd.structure.ribbon import Ribbon  # noqa: E402

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _photos():
    g = np.random.default_rng(11)
    photos = (g.integers(0, 256, (90, 120, 3), dtype=np.uint8), g.integers(0, 256, (87, 123, 3), dtype=np.uint8))
    for p in photos:
        p.setflags(write=False)
    return photos


def _arc(centre, radius, half, span, knots):
    """A ribbon of `knots` rulings on an arch about `centre`."""
    angles = np.radians(np.linspace(-span / 2.0, span / 2.0, knots))
    top = [(centre[0] + (radius + half) * math.sin(a), centre[1] - (radius + half) * math.cos(a)) for a in angles]
    bot = [(centre[0] + (radius - half) * math.sin(a), centre[1] - (radius - half) * math.cos(a)) for a in angles]
    return Ribbon(top, bot)


def _ribbons():
    """Six strips over the two photos: knots 2, 5 and 18, one partly outside its photo, one tall and short one (mode 'pad' leaves
    dst_w < W)."""
    return [(0, Ribbon.from_box([[10.0, 20.0], [100.0, 32.0], [97.0, 54.0], [7.0, 42.0]])),
            (0, _arc((60.0, 80.0), 50.0, 9.0, 100.0, 5)),
            (1, _arc((62.0, 85.0), 55.0, 11.0, 120.0, 18)),
            (1, _arc((100.0, 40.0), 45.0, 10.0, 150.0, 9)),                  # runs out of the photo on the right and at the top
            (0, Ribbon([[30.0, 60.0], [50.0, 56.0], [70.0, 60.0]], [[30.0, 84.0], [50.0, 80.0], [70.0, 84.0]])),   # 40 x 24
            (1, Ribbon.from_box([[40.0, 5.0], [58.0, 5.0], [58.0, 80.0], [40.0, 80.0]]))]                          # vertical


@pytest.mark.parametrize("canvas,mode", [((32, 128), 'resize'), ((32, 128), 'pad'), ((33, 70), 'resize'), ((33, 70), 'pad')])
def test_kernel_equals_the_restatement_bit_for_bit(canvas, mode):
    photos = _photos()
    plans = [(i, plan_strip(photos[i].shape, r, canvas, mode)) for i, r in _ribbons()]
    assert sorted(set(p.ribbon.knots for _, p in plans)) == [2, 3, 5, 9, 18]
    if mode == 'pad':
        assert any(p.dst_w < canvas[1] for _, p in plans)
    got, guards = S.device_strips(photos, plans, canvas, pad=5)
    assert (guards == -7.0).all()
    for m, (i, plan) in enumerate(plans):
        want = S.strip_crop_ref(photos[i], plan)
        assert got[m].tobytes() == want.tobytes(), (m, np.argwhere(got[m] != want)[:4].tolist())
        if plan.dst_w < canvas[1]:
            assert (got[m][:, :, plan.dst_w:] == S.zero_pixel()[:, None, None]).all()
    # the strip that leaves its photo reads zeros there, not the bytes beside the photo (255 in the packed buffer)
    x, y, _ = S.source_points(plans[3][1])
    outside = (x < -1.0) | (x > 123.0) | (y < -1.0)
    assert outside.any() and (got[3][:, outside] == S.zero_pixel()[:, None]).all()


def test_a_box_strip_is_the_quad_crop_and_a_bad_image_index_gives_the_zero_row():
    photos = _photos()
    quad = [[10.0, 20.0], [100.0, 20.0], [100.0, 50.0], [10.0, 50.0]]           # upright, 90 x 30 onto 128 x 32: the two maps meet in the same taps and fractions
    strip = plan_strip(photos[0].shape, Ribbon.from_box(quad), (32, 128), 'resize')
    got, guards = S.device_strips(photos, [(0, strip), (0, strip), (1, strip)], (32, 128), images=[0, 2, -1])
    crop = Q.device_crop(photos, [(0, plan_crop(photos[0].shape, quad, (32, 128), 'resize'))], (32, 128))
    assert got[0].tobytes() == crop[0].tobytes() and (guards == -7.0).all()
    for m in (1, 2):
        assert (got[m] == S.zero_pixel()[:, None, None]).all()


def test_resident_photo_with_a_negative_offset_and_no_launch_for_no_crops():
    photos = _photos()
    plans = [(i, plan_strip(photos[i].shape, r, (32, 128), 'resize')) for i, r in _ribbons()]
    got, guards = S.device_strips(photos, plans, (32, 128), resident=[0])           # photo 0 in front of src: a negative offset
    assert (guards == -7.0).all()
    for m, (i, plan) in enumerate(plans):
        assert got[m].tobytes() == S.strip_crop_ref(photos[i], plan).tobytes(), m
    cropper = StripCropper(image_size=(32, 128))
    resident = torch.from_numpy(np.array(photos[1])).to(DEV)
    ribbons = [[r for i, r in _ribbons() if i == 0], [r for i, r in _ribbons() if i == 1]]
    staged, layout = cropper.pack([photos[0], resident], ribbons)
    batch = cropper.upload(staged, layout)
    torch.cuda.synchronize()
    assert batch['index'].tolist() == [0, 0, 0, 1, 1, 1] and batch['dropped'] == []
    order = [(i, r) for i, r in _ribbons() if i == 0] + [(i, r) for i, r in _ribbons() if i == 1]
    for m, (i, r) in enumerate(order):
        want = S.strip_crop_ref(photos[i], plan_strip(photos[i].shape, r, (32, 128), 'resize'))
        assert batch['image'][m].cpu().numpy().tobytes() == want.tobytes(), m
    # M = 0: MR_OK with null pointers, nothing is launched; a zero-length ribbon is dropped by the cropper
    assert load().mr_strip_crop(0, 0, 0, 0, 0, 32, 128, 0.0, 0.0, 0.0, 0, stream_ptr()) == 0
    flat = Ribbon([[5.0, 5.0], [5.0, 5.0]], [[5.0, 9.0], [5.0, 9.0]])
    empty = cropper.crop([photos[0]], [[flat]])
    assert empty['image'].shape == (0, 3, 32, 128) and empty['dropped'] == [(0, 0)]
    t = torch.zeros(64, device=DEV)
    assert load().mr_strip_crop(ptr(t), ptr(t), 1, ptr(t), 1, 0, 128, 0.0, 0.0, 0.0, ptr(t), stream_ptr()) == 1    # MR_ERR_ARG
