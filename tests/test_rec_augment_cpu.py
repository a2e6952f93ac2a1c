"""The recognition augmentation on the host (no GPU): the planner megreader_amd/data/recognition_augment.py -- determinism,
independent streams, ranges, sign conventions, kernels, knots, the struct's layout -- and the restatement tests/_rec_augment_ref.py
at the identity descriptor against the quad crop's."""
import ctypes

import numpy as np
import pytest

import _quad_crop_ref as Q
import _rec_augment_ref as R
from megreader_amd._lib import STRUCTS
from megreader_amd.data.quad_crop import CropDesc, CropPlan, plan_crop
from megreader_amd.data.recognition_augment import (AUG_DTYPE, DRAWS, KNOTS, MAX_ERASE, N_DRAWS, AugDesc, RecognitionAugmenter,
                                                    apply_map, gaussian_kernels, kernels_f32, knot_displacement, motion_kernels,
                                                    smooth_knots)

CANVAS = (32, 128)
SHAPES = [(23, 61), (40, 150), (31, 97, 3), (64, 48), (17, 300), (32, 128)]


def stored_plan(shape, canvas, dst_w=None):
    """The `CropPlan` that reads a stored crop of `shape` whole: what the identity descriptor of a shape is compared with."""
    H, W = canvas
    dst_w = W if dst_w is None else dst_w
    return CropPlan(shape=tuple(shape[:2]), frame=tuple(shape[:2]), canvas=(H, W), dst_w=dst_w,
                    sx=1.0 / (float(dst_w) / float(shape[1])), sy=1.0 / (float(H) / float(shape[0])), cu1=float(shape[1] - 1),
                    cv1=float(shape[0] - 1), h9=np.eye(3).reshape(9))


@pytest.mark.parametrize("canvas", [(19, 70), (33, 65)])
def test_identity_restatement_equals_the_quad_crop_restatement(canvas):
    rng = np.random.RandomState(3)
    aug = RecognitionAugmenter()
    crop = rng.randint(0, 256, (23, 61, 3)).astype(np.uint8)
    photo = rng.randint(0, 256, (120, 200, 3)).astype(np.uint8)
    quad_plan = plan_crop(photo.shape, [[30.5, 20.0], [150.0, 35.5], [145.0, 70.0], [25.0, 55.0]], canvas, 'resize', 'quad')
    pad_plan = plan_crop(photo.shape, [[30, 20], [90, 26], [88, 60], [28, 54]], canvas, 'pad')
    assert pad_plan.dst_w < canvas[1]
    for source, item, plan in ((crop, crop.shape, stored_plan(crop.shape, canvas)), (photo, quad_plan, quad_plan),
                               (photo, pad_plan, pad_plan)):
        d = aug.identity(item, canvas, 'resize')[0]
        want = Q.quad_crop_ref(source, plan)
        got = R.augment_ref(d, [source], *canvas)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_struct_layout():
    assert ctypes.sizeof(AugDesc) == 560 == AUG_DTYPE.itemsize
    assert [n for n, _ in AugDesc._fields_] == [n for n, _ in STRUCTS["mr_aug_desc"]]
    for name, ctype in STRUCTS["mr_aug_desc"]:
        assert AUG_DTYPE.fields[name][1] == getattr(AugDesc, name).offset, name
        assert AUG_DTYPE.fields[name][0].itemsize == ctypes.sizeof(ctype), name
    want = dict(image=0, row=4, dst_w=8, quant=12, blur=16, n_erase=20, seed=24, reserved=28, sx=32, sy=40, cu0=48, cu1=56, cv0=64,
                cv1=72, g=80, h=152, dx=224, dy=260, m=296, b=332, k=344, noise_amp=444, erase=448, erase_col=512)
    assert {n: getattr(AugDesc, n).offset for n in want} == want
    for name in ("sx", "sy", "cu0", "cu1", "cv0", "cv1", "g", "h"):
        assert getattr(AugDesc, name).offset % 8 == 0
    assert (KNOTS, MAX_ERASE) == (9, 4) and N_DRAWS == sum(c for _, c in DRAWS)
    assert ctypes.sizeof(CropDesc) == 112                       # the struct the identity consequence refers to


def test_determinism_per_seed_and_index():
    a, b = RecognitionAugmenter(seed=5, p=0.7), RecognitionAugmenter(seed=5, p=0.7)
    t0, r0 = a.sample(SHAPES, CANVAS, 'pad', 3)
    t1, r1 = b.sample(SHAPES, CANVAS, 'pad', 3)
    assert t0.tobytes() == t1.tobytes() and np.array_equal(r0, r1)
    assert a.sample(SHAPES, CANVAS, 'pad', 3)[0].tobytes() == t0.tobytes()          # no state between calls
    assert a.sample(SHAPES, CANVAS, 'pad', 4)[0].tobytes() != t0.tobytes()
    assert RecognitionAugmenter(seed=6, p=0.7).sample(SHAPES, CANVAS, 'pad', 3)[0].tobytes() != t0.tobytes()


def test_streams_are_independent_of_other_settings_and_of_the_batch():
    base = RecognitionAugmenter(seed=1, p=1.0)
    other = RecognitionAugmenter(seed=1, p=1.0, rotate=(-30, 30), gaussian_sigma=(0.5, 0.6), erase_prob=1.0, pixelate_prob=1.0)
    d0, d1 = base.draw(6, CANVAS, [128] * 6, 2), other.draw(6, CANVAS, [128] * 6, 2)
    assert not np.array_equal(d0["rotate"], d1["rotate"]) and not np.array_equal(d0["sigma"], d1["sigma"])
    for name in ("shear", "scale", "translate", "perspective", "dx", "dy", "contrast", "brightness", "channel_gain", "gray",
                 "invert", "motion", "motion_length", "motion_angle", "noise", "seed", "erase_col"):
        assert np.array_equal(d0[name], d1[name]), name
    # a sample's values depend on its own position, not on how many samples follow or what they are
    t_all, _ = base.sample(SHAPES, CANVAS, 'resize', 2)
    t_two, _ = base.sample(SHAPES[:2], CANVAS, 'resize', 2)
    assert t_all[:2].tobytes() == t_two.tobytes()
    changed = [SHAPES[0], (50, 77)] + SHAPES[2:]
    t_chg, _ = base.sample(changed, CANVAS, 'resize', 2)
    keep = [0, 2, 3, 4, 5]
    assert t_chg[keep].tobytes() == t_all[keep].tobytes()


def test_p_zero_and_one():
    t, rows = RecognitionAugmenter(p=0.0).sample(SHAPES, CANVAS, 'resize', 0)
    assert len(t) == 0 and len(rows) == 0 and t.dtype == AUG_DTYPE
    t, rows = RecognitionAugmenter(p=1.0).sample(SHAPES, CANVAS, 'resize', 0)
    assert rows.tolist() == list(range(len(SHAPES))) and t["row"].tolist() == rows.tolist() and t["image"].tolist() == rows.tolist()
    t, rows = RecognitionAugmenter(p=0.5, seed=2).sample(SHAPES * 20, CANVAS, 'resize', 0)
    assert 0 < len(rows) < len(SHAPES) * 20 and np.array_equal(t["row"], rows) and (np.diff(rows) > 0).all()
    t, rows = RecognitionAugmenter(p=1.0).sample(SHAPES, CANVAS, 'resize', 0, images=[5, 4, 3, 2, 1, 0])
    assert t["image"].tolist() == [5, 4, 3, 2, 1, 0]


def test_every_drawn_value_lies_inside_its_range():
    aug = RecognitionAugmenter(seed=9, p=1.0, gray_prob=0.5, invert_prob=0.5, motion_prob=0.5, pixelate_prob=0.5, erase_prob=0.5,
                               erase_count=(1, 4))
    n, (H, W) = 400, CANVAS
    shapes = [SHAPES[k % len(SHAPES)] for k in range(n)]
    d = aug.draw(n, CANVAS, [W] * n, 1)
    for name, (lo, hi) in (("rotate", aug.rotate), ("shear", aug.shear), ("scale", aug.scale), ("contrast", aug.contrast),
                           ("brightness", aug.brightness), ("channel_gain", aug.channel_gain), ("sigma", aug.gaussian_sigma),
                           ("motion_length", aug.motion_length), ("noise", aug.noise), ("motion_angle", (0.0, 180.0))):
        assert (d[name] >= lo).all() and (d[name] <= hi).all() and d[name].std() > 0, name
    for name, amp in (("translate", aug.translate), ("perspective", aug.perspective), ("dx", aug.stretch * H),
                      ("dy", aug.distort * H)):
        assert (np.abs(d[name]) <= amp).all() and (d[name] < 0).any() and (d[name] > 0).any(), name
    assert set(np.unique(d["pixelate"])) == {1, 2, 3}
    assert set(np.unique(d["n_erase"])) == {0, 1, 2, 3, 4}
    for name in ("gray", "invert", "motion", "apply"):
        assert d[name].dtype == bool and d[name].any()
    assert not d["gray"].all() and not d["motion"].all()
    t, _ = aug.sample(shapes, CANVAS, 'resize', 1)
    assert (t["quant"] >= 1).all() and (t["n_erase"] >= 0).all() and (t["n_erase"] <= 4).all() and (t["dst_w"] == W).all()
    assert (t["noise_amp"] >= 0).all() and (t["noise_amp"] <= np.float32(16.0)).all()
    assert (t["erase_col"] >= 0).all() and (t["erase_col"] <= 255).all()
    e = t["erase"].reshape(n, 4, 4)
    side_lo, side_hi = max(round(aug.erase_size[0] * H) - 1, 1), round(aug.erase_size[1] * H) + 1
    assert ((e[..., 1] - e[..., 0]) >= side_lo).all() and ((e[..., 1] - e[..., 0]) <= side_hi).all()
    assert ((e[..., 3] - e[..., 2]) >= side_lo).all() and ((e[..., 3] - e[..., 2]) <= side_hi).all()
    assert (e[..., 0] < 0).any() and (e[..., 1] > W).any()              # rectangles hang over the edges
    assert t["reserved"].tolist() == [0] * n
    # the clamp of a stored crop is its replicated border
    hw = np.array([s[:2] for s in shapes], dtype=np.float64)
    assert np.array_equal(t["cu0"], np.zeros(n)) and np.array_equal(t["cu1"], hw[:, 1] - 1)
    assert np.array_equal(t["cv0"], np.zeros(n)) and np.array_equal(t["cv1"], hw[:, 0] - 1)


def test_quad_crops_get_context_around_the_word_and_the_plans_map():
    plan = plan_crop((120, 200), [[30, 20], [150, 35], [145, 70], [25, 55]], CANVAS, 'resize', 'quad')
    aug = RecognitionAugmenter(p=1.0, context=0.25)
    t, rows = aug.sample([plan, (40, 150)], CANVAS, 'resize', 0, images=[7, 1])
    Hr, Wr = plan.frame
    assert t["cu0"][0] == -0.25 * Hr and t["cu1"][0] == Wr - 1 + 0.25 * Hr
    assert t["cv0"][0] == -0.25 * Hr and t["cv1"][0] == Hr - 1 + 0.25 * Hr
    assert np.array_equal(t["h"][0], plan.h9) and np.array_equal(t["h"][1], np.eye(3).reshape(9))
    assert (t["sx"][0], t["sy"][0], t["dst_w"][0]) == (plan.sx, plan.sy, plan.dst_w)
    assert t["cu0"][1] == 0.0 and t["cu1"][1] == 149.0 and t["image"].tolist() == [7, 1]
    with pytest.raises(ValueError):
        aug.sample([plan], (32, 100), 'resize', 0)


def test_rotation_and_translation_follow_the_documented_signs():
    aug = RecognitionAugmenter()
    n = 41
    TL, TR, BR, BL = (-0.5, -0.5), (n - 0.5, -0.5), (n - 0.5, n - 0.5), (-0.5, n - 0.5)
    g = aug.plan((n, n), (n, n), rotate=90.0)[0]["g"]
    # +90 degrees is clockwise on screen: the content at TL appears at TR, so the OUTPUT corner TR reads the SOURCE corner TL
    for out, src in ((TR, TL), (BR, TR), (BL, BR), (TL, BL)):
        assert np.allclose(apply_map(g, out), src, atol=1e-9)
    right_of_centre = ((n - 1) / 2 + 10.0, (n - 1) / 2)
    g5 = aug.plan((n, n), (n, n), rotate=5.0)[0]["g"]
    assert apply_map(np.linalg.inv(g5.reshape(3, 3)).reshape(9), right_of_centre)[1] > (n - 1) / 2       # moves DOWNWARDS
    # a translation by (+tx, +ty) Hr moves the content right and down: the output at p shows the source at p - t
    g = aug.plan((20, 60), CANVAS, translate=(0.25, -0.1))[0]["g"]
    assert np.allclose(apply_map(g, (30.0, 10.0)), (30.0 - 0.25 * 20, 10.0 + 0.1 * 20), atol=1e-9)
    # scale > 1 enlarges: the output reads nearer to the centre; shear > 0 moves what is below the centre to the right
    g = aug.plan((21, 61), CANVAS, scale=2.0)[0]["g"]
    assert np.allclose(apply_map(g, (30.0 + 8, 10.0 + 4)), (30.0 + 4, 10.0 + 2), atol=1e-9)
    g = aug.plan((21, 61), CANVAS, shear=0.5)[0]["g"]
    assert np.allclose(apply_map(g, (30.0 + 2, 10.0 + 4)), (30.0, 10.0 + 4), atol=1e-9)
    # perspective: the displaced corner of the output shows the source's corner
    g = aug.plan((20, 60), CANVAS, perspective=((0.1, 0.2), (0, 0), (0, 0), (0, 0)))[0]["g"]
    assert np.allclose(apply_map(g, (-0.5 + 2.0, -0.5 + 4.0)), (-0.5, -0.5), atol=1e-9)
    assert np.allclose(apply_map(g, (59.5, 19.5)), (59.5, 19.5), atol=1e-9)
    # nothing moves: exactly the identity
    assert np.array_equal(aug.plan((20, 60), CANVAS)[0]["g"], np.eye(3).reshape(9))


def test_kernels_sum_to_one():
    sig = np.concatenate([np.linspace(0.0, 1.2, 60), [0.05, 0.1, 0.1001, 3.0]])
    lengths, angles = np.meshgrid(np.linspace(1.0, 5.0, 9), np.linspace(0.0, 180.0, 37))
    for k64 in (gaussian_kernels(sig), motion_kernels(lengths.reshape(-1), angles.reshape(-1))):
        k = kernels_f32(k64)
        assert k.dtype == np.float32 and k.shape == (len(k64), 25) and (k >= 0).all()
        assert np.abs(k.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
        assert np.abs(k - k64.reshape(-1, 25)).max() < 1e-6
    ident = np.zeros(25, dtype=np.float32)
    ident[12] = 1
    assert np.array_equal(kernels_f32(gaussian_kernels([0.0, 0.1]))[0], ident)
    g = gaussian_kernels([0.8])[0]
    assert np.allclose(g, g.T) and np.allclose(g, g[::-1, ::-1]) and g[2, 2] == g.max()
    horizontal, vertical = motion_kernels([5.0, 5.0], [0.0, 90.0])
    assert np.allclose(horizontal[2], 0.2) and np.allclose(horizontal.sum(), 1.0) and np.allclose(vertical[:, 2], 0.2)
    diag = motion_kernels([5.0], [45.0])[0]                 # rows are v, y down: +45 degrees runs from top-left to bottom-right
    assert diag[0, 0] > 0 and diag[4, 4] > 0 and diag[0, 4] == 0 and diag[4, 0] == 0
    t, _ = RecognitionAugmenter(p=1.0, motion_prob=0.5, seed=4).sample([(32, 100)] * 200, CANVAS, 'resize', 0)
    assert np.abs(t["k"].astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
    assert set(np.unique(t["blur"])) <= {0, 1} and (t["blur"] == 1).any()


def test_knots():
    raw = np.arange(9, dtype=np.float64)[None] ** 2
    s = smooth_knots(raw)[0]
    assert s[0] == 0.75 * 0 + 0.25 * 1 and s[8] == 0.25 * 49 + 0.75 * 64 and s[4] == 0.25 * 9 + 0.5 * 16 + 0.25 * 25
    knots = np.array([1.0, -2.0, 3.0, 0.5, 0.0, -1.0, 2.0, 4.0, -3.0])
    dst_w = 70
    step = dst_w / 8.0
    # at the two outermost pixel centres: inside the first and the last interval, linear between their knots
    assert np.isclose(knot_displacement(knots, 0.5, dst_w), 1.0 + (-2.0 - 1.0) * (0.5 / step))
    assert np.isclose(knot_displacement(knots, dst_w - 0.5, dst_w), 4.0 + (-3.0 - 4.0) * ((dst_w - 0.5 - 7 * step) / step))
    for j in range(9):
        assert np.isclose(knot_displacement(knots, j * step, dst_w), knots[j])
    # ... and that is what the restatement does with them: a dy of one frame row on a photo that is a ramp in y
    H, W = 16, 70
    photo = np.repeat((np.arange(40, dtype=np.uint8) * 5)[:, None, None], 70 * 3, axis=1).reshape(40, 70, 3)
    aug = RecognitionAugmenter()
    dy = np.full(9, 2.0)
    dy[5:] = -1.0
    d = aug.plan(photo.shape, (H, W), dy=dy)[0]
    col = R.comp_ref(d, photo, H, W)
    sy = 40 / 16
    v = 6
    for u in (0, 30, 69):
        disp = float(knot_displacement(dy, u + 0.5, W))
        assert np.isclose(col[v, u, 0], 5 * ((v + 0.5 + disp) * sy - 0.5), atol=1e-3)


def test_colour_map_composition():
    aug = RecognitionAugmenter()
    d = aug.plan((8, 8), (8, 8), contrast=1.5, brightness=10.0, channel_gain=(1.0, 0.5, 2.0), invert=True)[0]
    x = np.array([100.0, 50.0, 200.0])
    want = 255.0 - np.array([1.0, 0.5, 2.0]) * (1.5 * (x - 127.5) + 127.5 + 10.0)
    assert np.allclose(d["m"].reshape(3, 3) @ x + d["b"], want, atol=1e-3)
    d = aug.plan((8, 8), (8, 8), gray=True)[0]
    luma = 0.114 * x[0] + 0.587 * x[1] + 0.299 * x[2]
    assert np.allclose(d["m"].reshape(3, 3) @ x + d["b"], [luma] * 3, atol=1e-3)
    d = aug.identity((8, 8), (8, 8))[0]
    assert np.array_equal(d["m"], np.eye(3, dtype=np.float32).reshape(9)) and np.array_equal(d["b"], np.zeros(3, dtype=np.float32))
    assert d["quant"] == 1 and d["blur"] == 0 and d["n_erase"] == 0 and d["noise_amp"] == 0
    assert not d["dx"].any() and not d["dy"].any()


def test_argument_errors():
    for kw in (dict(p=1.5), dict(p=-0.1), dict(rotate=(5, -5)), dict(scale=(0.0, 1.0)), dict(translate=-1.0),
               dict(gaussian_sigma=(-1.0, 1.0)), dict(motion_length=(3, 7)), dict(pixelate=(0, 2)), dict(erase_count=(1, 5)),
               dict(gray_prob=2.0), dict(noise=(1.0, float('nan'))), dict(seed=-1), dict(contrast=(-0.5, 1.0))):
        with pytest.raises(ValueError):
            RecognitionAugmenter(**kw)
    aug = RecognitionAugmenter()
    with pytest.raises(NotImplementedError):
        aug.sample(SHAPES, CANVAS, 'keep_ratio', 0)
    with pytest.raises(ValueError):
        aug.sample([(0, 10)], CANVAS, 'resize', 0)
    with pytest.raises(ValueError):
        aug.sample(SHAPES, (0, 128), 'resize', 0)
    with pytest.raises(ValueError):
        aug.plan((8, 8), (8, 8), erase=[((0, 1, 0, 1), (0, 0, 0))] * 5)
    with pytest.raises(ValueError):
        aug.plan((8, 8), (8, 8), dx=(0.0,) * 8)
    with pytest.raises(ValueError):
        aug.plan((8, 8), (8, 8), pixelate=0)
    assert aug.plan((8, 8), (8, 8), seed=0xFFFFFFFF)[0]["seed"] == -1
