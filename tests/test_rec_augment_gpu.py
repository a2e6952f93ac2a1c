"""mr_rec_augment (csrc/rec_augment.hip) against the numpy restatement of its header rule (tests/_rec_augment_ref.py), BIT FOR BIT:
every operation of the rule is an IEEE basic operation with contraction off (the float64 divisions of the two maps and the float32
division by 255 are correctly rounded on both sides), so a mismatch is a wrong operation, not a tolerance.  dst lies between guard
bytes and holds NaN bits before every call; every byte around the photos is 255.  The canvases, 19 x 70 and 33 x 65, cross the
16 x 64 tile in both directions by a few pixels, so the blur reads its halo across tile edges and beyond the canvas."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _quad_crop_ref as Q  # noqa: E402
import _rec_augment_ref as R  # noqa: E402
from megreader_amd._lib import call, load, stream_ptr  # noqa: E402
from megreader_amd.data.quad_crop import CropPlan, plan_crop  # noqa: E402
from megreader_amd.data.recognition_augment import AUG_DTYPE, RecognitionAugmenter  # noqa: E402

MR_ERR_ARG = 1
MEAN = R.RGB_MEAN
AUG = RecognitionAugmenter()
_rng = np.random.RandomState(17)
SMALL = _rng.randint(0, 256, (23, 61, 3)).astype(np.uint8)
WIDE = _rng.randint(0, 256, (40, 150, 3)).astype(np.uint8)
PHOTO = _rng.randint(0, 256, (120, 200, 3)).astype(np.uint8)
PHOTOS = [SMALL, WIDE, PHOTO]
CASES = [((19, 70), 0), ((33, 65), 1)]                      # (canvas, stored crop)
QUAD = [[30.5, 20.0], [150.0, 35.5], [145.0, 70.0], [25.0, 55.0]]

JITTER = dict(rotate=4.0, shear=0.15, scale=1.08, translate=(0.04, -0.06),
              perspective=((0.05, -0.03), (-0.04, 0.06), (0.02, 0.02), (-0.06, -0.05)))
KNOTS = dict(dx=(1.5, -2.0, 0.5, 2.5, -1.0, 0.0, -2.5, 1.0, -0.5), dy=(-1.0, 1.5, 2.0, -2.0, 0.5, -0.5, 1.0, -1.5, 2.5))
COLOUR = dict(contrast=1.3, brightness=-12.0, channel_gain=(0.9, 1.1, 1.0), gray=True, invert=True)
EFFECTS = {
    "jitter": JITTER,
    "knots": KNOTS,
    "colour": COLOUR,
    "gaussian": dict(sigma=0.9),
    "motion": dict(motion=(4.3, 30.0)),
    "sharpen": dict(kernel=[0, 0, 0, 0, 0, 0, 0, -0.5, 0, 0, 0, -0.5, 3, -0.5, 0, 0, 0, -0.5, 0, 0, 0, 0, 0, 0, 0]),
    "noise": dict(noise=12.0, seed=0x9ABCDEF0),
    "quant2": dict(pixelate=2),
    "quant3": dict(pixelate=3, rotate=-3.0),
    "erase1": dict(erase=[((5, 20, 3, 11), (255.0, 0.0, 17.5))]),
    "erase4": dict(erase=[((-4, 6, -2, 9), (1.0, 2.0, 3.0)), ((60, 90, 10, 40), (200.0, 100.0, 50.0)),     # two hang over the edges
                          ((10, 40, 8, 12), (0.0, 0.0, 0.0)), ((30, 35, 0, 33), (90.5, 91.5, 92.5))]),       # the last two overlap
    "all": dict(JITTER, **KNOTS, **COLOUR, motion=(5.0, 120.0), noise=9.0, seed=77, pixelate=2,
                erase=[((12, 30, 4, 15), (10.0, 250.0, 128.0)), ((50, 80, -3, 6), (128.0, 128.0, 128.0))]),
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def table_of(descs):
    t = np.concatenate(descs).astype(AUG_DTYPE)
    t["row"] = np.arange(len(t))
    return t


def check(table, N, canvas, photos=PHOTOS, **kw):
    got = R.run_kernel(photos, table, N, *canvas, **kw)
    want = R.batch_ref(table, photos if kw.get("n_images") is None else photos[:kw["n_images"]], N, *canvas)
    for n in range(N):
        assert np.array_equal(got[n], want[n]), "row %d: %d elements differ" % (n, int((got[n] != want[n]).sum()))
    return got


@pytest.mark.parametrize("canvas,image", CASES)
def test_identity_descriptor_equals_mr_quad_crop(canvas, image):
    crop = PHOTOS[image]
    H, W = canvas
    stored = CropPlan(shape=crop.shape[:2], frame=crop.shape[:2], canvas=canvas, dst_w=W, sx=1.0 / (float(W) / crop.shape[1]),
                      sy=1.0 / (float(H) / crop.shape[0]), cu1=float(crop.shape[1] - 1), cv1=float(crop.shape[0] - 1),
                      h9=np.eye(3).reshape(9))
    quad = plan_crop(PHOTO.shape, QUAD, canvas, 'resize', 'quad')
    padded = plan_crop(PHOTO.shape, [[30, 20], [90, 26], [88, 60], [28, 54]], canvas, 'pad')
    assert padded.dst_w < W
    want = Q.device_crop(PHOTOS, [(image, stored), (2, quad), (2, padded)], canvas)
    table = table_of([AUG.identity(crop.shape, canvas, image=image), AUG.identity(quad, canvas, image=2),
                      AUG.identity(padded, canvas, image=2)])
    got = check(table, 3, canvas)
    assert np.array_equal(got, bits(want))


@pytest.mark.parametrize("canvas,image", CASES)
def test_each_effect_alone_and_all_together(canvas, image):
    names = list(EFFECTS)
    table = table_of([AUG.plan(PHOTOS[image].shape, canvas, image=image, **EFFECTS[k]) for k in names])
    got = R.run_kernel(PHOTOS, table, len(names), *canvas, pad=5)
    want = R.batch_ref(table, PHOTOS, len(names), *canvas)
    plain = R.augment_ref(AUG.identity(PHOTOS[image].shape, canvas, image=image)[0], PHOTOS, *canvas).view(np.uint32)
    for n, name in enumerate(names):
        assert np.array_equal(got[n], want[n]), "%s: %d elements differ" % (name, int((got[n] != want[n]).sum()))
        assert not np.array_equal(want[n], plain), "%s changes nothing: the case tests nothing" % name


@pytest.mark.parametrize("canvas", [c for c, _ in CASES])
def test_pad_columns_and_no_blur_bleeding_from_them(canvas):
    H, W = canvas
    padded = plan_crop(PHOTO.shape, [[30, 20], [90, 26], [88, 60], [28, 54]], canvas, 'pad')
    table = table_of([AUG.plan(padded, canvas, image=2, sigma=1.1, **JITTER), AUG.plan(padded, canvas, image=2, motion=(5.0, 0.0))])
    table["dst_w"][1] = 17                                   # a valid region that ends inside the first tile
    got = check(table, 2, canvas)
    zero = bits(Q.zero_pixel(MEAN))
    for n, wv in ((0, padded.dst_w), (1, 17)):
        assert wv < W and (got[n][:, :, wv:] == zero[:, None, None]).all()
        # the last valid column is a blur of valid columns only: replicating the border, not mixing the zero canvas in
        assert (got[n][:, :, wv - 1] != zero[:, None]).any()


@pytest.mark.parametrize("canvas,image", CASES)
def test_horizon_and_taps_outside_the_photo(canvas, image):
    H, W = canvas
    behind = AUG.plan(PHOTOS[image].shape, canvas, image=image, sigma=0.8)
    behind["g"][0][6] = -1.0 / (0.6 * PHOTOS[image].shape[1])         # D = 1 - cx / (0.6 Wr): <= 0 on the right of the frame
    corner = plan_crop(PHOTO.shape, [[2, 1], [80, 3], [79, 30], [1, 28]], canvas, 'resize', 'quad')
    outside = RecognitionAugmenter(context=0.5).plan(corner, canvas, image=2, translate=(0.3, 0.3), motion=(3.0, 60.0))
    assert outside["cu0"][0] < 0 and outside["cv0"][0] < 0
    got = check(table_of([behind, outside]), 2, canvas)
    zero = bits(Q.zero_pixel(MEAN))
    assert (got[0][:, :, -3:] == zero[:, None, None]).all() and (got[0][:, :, :8] != zero[:, None, None]).any()
    assert (got[1][:, :2, :2] == zero[:, None, None]).all()            # the photo's outside reads 0, not a replicated edge


def test_fewer_descriptors_than_rows_and_none():
    canvas = (19, 70)
    table = table_of([AUG.plan(SMALL.shape, canvas, image=0, **EFFECTS["all"]), AUG.plan(WIDE.shape, canvas, image=1, **KNOTS)])
    table["row"] = [3, 1]
    got = check(table, 5, canvas)
    for n in (0, 2, 4):
        assert (got[n] == R.NAN_BITS).all()
    got = R.run_kernel(PHOTOS, table[:0], 5, *canvas)                  # M == 0: nothing is launched, nothing written
    assert (got == R.NAN_BITS).all()
    assert load().mr_rec_augment(0, 0, 0, 0, 0, 0, 19, 70, 0.0, 0.0, 0.0, 0, stream_ptr()) == 0


def test_photo_in_another_allocation_with_a_padded_pitch():
    canvas = (33, 65)
    table = table_of([AUG.plan(WIDE.shape, canvas, image=1, **EFFECTS["all"]), AUG.plan(SMALL.shape, canvas, image=0, **JITTER)])
    check(table, 2, canvas, pad=7, shift=1 << 20)                      # every table offset is negative


def test_tables_in_device_memory_are_cut_to_their_limits():
    canvas = (19, 70)
    t = table_of([AUG.plan(SMALL.shape, canvas, image=0, **EFFECTS["erase4"]) for _ in range(6)])
    t["image"][0], t["image"][1] = 3, -1                               # no such photo: the normalised zero pixel everywhere
    t["n_erase"][2], t["quant"][2] = 7, 0                              # cut to 4, treated as 1
    t["n_erase"][3], t["quant"][3] = -5, -2
    t["dst_w"][4] = 500                                                # cut to W
    t["dst_w"][5] = -3                                                 # nothing valid
    got = check(t, 8, canvas)
    zero = bits(Q.zero_pixel(MEAN))
    for n in (0, 1, 5):
        assert (got[n] == zero[:, None, None]).all()
    t["row"][0], t["row"][1] = 8, -1                                   # rows that do not exist: nothing is written for them
    t["image"][0] = 0
    got = check(t, 8, canvas)
    assert (got[0] == R.NAN_BITS).all() and (got[1] == R.NAN_BITS).all()
    assert np.array_equal(got[2], got[4]) and not np.array_equal(got[2], got[3])   # cut to the limits the plan had anyway
    one = t[2:3].copy()
    one["row"] = 0
    got = check(one, 1, canvas, n_images=0)                            # I == 0: every index is out of range
    assert (got[0] == zero[:, None, None]).all()


def test_alone_and_inside_a_batch_and_run_to_run():
    canvas = (33, 65)
    descs = [AUG.plan(PHOTOS[k % 2].shape, canvas, image=k % 2, **EFFECTS[name])
             for k, name in enumerate(("jitter", "all", "motion", "noise", "quant3"))]
    batch = table_of(descs)
    got = R.run_kernel(PHOTOS, batch, 5, *canvas)
    again = R.run_kernel(PHOTOS, batch, 5, *canvas)
    assert np.array_equal(got, again)
    alone = table_of([descs[1]])
    assert np.array_equal(R.run_kernel(PHOTOS, alone, 1, *canvas)[0], got[1])
    alone["row"] = 4                                                    # ... and wherever it lands
    assert np.array_equal(R.run_kernel(PHOTOS, alone, 5, *canvas)[4], got[1])


def test_argument_errors_write_nothing():
    lib = load()
    H, W = 19, 70
    table = table_of([AUG.plan(SMALL.shape, (H, W), image=0, **JITTER), AUG.plan(WIDE.shape, (H, W), image=1, sigma=1.0)])
    host, images = R.pack_photos(PHOTOS)
    d_src = torch.from_numpy(host).cuda()
    d_images = torch.from_numpy(np.frombuffer(bytes(images), dtype=np.uint8).copy()).cuda()
    d_table = torch.from_numpy(np.frombuffer(table.tobytes(), dtype=np.uint8).copy()).cuda()
    dst = torch.full((4, 3, H, W), float('nan'), dtype=torch.float32, device="cuda")

    def run(descs=None, **kw):
        a = dict(src=d_src.data_ptr(), images=d_images.data_ptr(), I=3, descs=d_table.data_ptr() if descs is None else descs,
                 M=2, N=4, H=H, W=W, dst=dst.data_ptr())
        a.update(kw)
        return lib.mr_rec_augment(a["src"], a["images"], a["I"], a["descs"], a["M"], a["N"], a["H"], a["W"], MEAN[0], MEAN[1],
                                  MEAN[2], a["dst"], stream_ptr())

    for kw in (dict(src=0), dict(images=0), dict(descs=0), dict(dst=0), dict(I=-1), dict(M=-1), dict(N=-1), dict(H=0), dict(W=0),
               dict(H=-4), dict(M=(1 << 31) - 1, H=32, W=128)):                         # more than INT_MAX tiles
        assert run(**kw) == MR_ERR_ARG, kw
        assert b"mr_rec_augment" in lib.mr_last_error()

    keep = []                                            # a pinned table lives until the device has read it

    def pinned_run(change):
        t = table.copy()
        change(t)
        keep.append(torch.from_numpy(np.frombuffer(t.tobytes(), dtype=np.uint8).copy()).pin_memory())
        return run(descs=keep[-1].data_ptr())

    def setter(field, k, value):
        def change(t):
            t[field][k] = value
        return change
    for change in (setter("row", 1, 0), setter("row", 0, 4), setter("row", 1, -1), setter("image", 0, 3), setter("image", 1, -1),
                   setter("n_erase", 0, 5), setter("n_erase", 1, -1), setter("dst_w", 0, 0), setter("dst_w", 1, W + 1)):
        assert pinned_run(change) == MR_ERR_ARG
        assert b"mr_rec_augment" in lib.mr_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()
    assert pinned_run(lambda t: None) == 0                                               # the same table unchanged is accepted
    torch.cuda.synchronize()
    want = R.batch_ref(table, PHOTOS, 4, H, W)
    got = bits(dst.cpu().numpy())
    assert np.array_equal(got[:2], want[:2]) and np.isnan(dst[2:].cpu().numpy()).all()
    assert lib.mr_sizeof_aug_desc() == 560 == AUG_DTYPE.itemsize


def test_replay_from_a_captured_graph():
    H, W = 33, 65
    first = table_of([AUG.plan(WIDE.shape, (H, W), image=1, **EFFECTS["all"]), AUG.plan(SMALL.shape, (H, W), image=0, **KNOTS)])
    second = table_of([AUG.plan(SMALL.shape, (H, W), image=0, sigma=1.0, **JITTER), AUG.plan(WIDE.shape, (H, W), image=1, noise=5.0)])
    host, images = R.pack_photos(PHOTOS)
    d_src = torch.from_numpy(host).cuda()
    d_images = torch.from_numpy(np.frombuffer(bytes(images), dtype=np.uint8).copy()).cuda()
    d_table = torch.from_numpy(np.frombuffer(first.tobytes(), dtype=np.uint8).copy()).cuda()
    dst = torch.zeros((2, 3, H, W), dtype=torch.float32, device="cuda")
    args = (d_src.data_ptr(), d_images.data_ptr(), 3, d_table.data_ptr(), 2, 2, H, W, MEAN[0], MEAN[1], MEAN[2], dst.data_ptr())
    call("mr_rec_augment", *args)                                                        # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call("mr_rec_augment", *args)
    for table in (second, first):                                                        # new contents of the same buffer
        d_table.copy_(torch.from_numpy(np.frombuffer(table.tobytes(), dtype=np.uint8).copy()))
        dst.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(dst.cpu().numpy()), R.batch_ref(table, PHOTOS, 2, H, W))
