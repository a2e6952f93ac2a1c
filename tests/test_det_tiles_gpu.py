"""mr_tile_sample and mr_tile_stitch (csrc/det_tiles.hip) bit for bit against their numpy restatements (tests/_det_tiles_ref.py),
the sampled tiles also against the windows of mr_resize_normalize on the whole canvas, and the invariant they exist for: a
detector of bounded reach run on tiles and stitched equals the detector run on the whole canvas."""
import ctypes

import numpy as np
import pytest
import torch

import _det_tiles_ref as R
from megreader_amd import DetectionTiler, _lib
from megreader_amd.data import DevicePipeline
from megreader_amd.data.detection_tiles import StitchLevel, StitchPhoto, TileDesc
from megreader_amd.data.device_pipeline import RGB_MEAN
from megreader_amd.data.quad_crop import CropImage

pytestmark = pytest.mark.gpu

TH, TW, HALO = 16, 24, (4, 4)
GUARD = 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def photos_np():
    rng = np.random.RandomState(11)
    return [rng.randint(0, 256, (37, 53, 3)).astype(np.uint8), rng.randint(0, 256, (64, 41, 3)).astype(np.uint8)]


def padded(photo):
    """The photo as a CUDA tensor whose rows are 7 pixels longer than the photo's."""
    h, w = photo.shape[:2]
    wide = torch.full((h, w + 7, 3), 255, dtype=torch.uint8, device="cuda")
    wide[:, :w] = torch.from_numpy(photo).cuda()
    view = wide[:, :w]
    assert view.stride() == (3 * (w + 7), 3, 1)
    return view


def on_device(table):
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()


def whole_on_device(photo, hc, wc):
    return DevicePipeline(image_size=(hc, wc), mode='resize').process([photo], [''])['image'][0].cpu().numpy()


def test_sampled_tiles_equal_the_restatement_and_the_windows_of_the_whole_canvas():
    photos = photos_np()
    tiler = DetectionTiler(tile=(TH, TW), halo=HALO, scales=(1.0, 0.5, 1.7), align=1)
    out = tiler.sample([photos[0], padded(photos[1])])
    plan, got = out['plan'], out['tiles'].cpu().numpy()
    assert [lv.canvas for lv in plan.levels[0]] == [(37, 53), (19, 27), (63, 90)]        # 1.0: the copy shortcut
    assert got.shape == (plan.T, 3, TH, TW)
    want = R.tile_sample_ref(photos, R.entries(plan.tile_descs(), plan.T), TH, TW)
    assert np.array_equal(bits(got), bits(want))
    whole = {(i, l): whole_on_device(photos[i], *lv.canvas) for i, levels in enumerate(plan.levels) for l, lv in enumerate(levels)}
    overhang = 0
    for t, (i, l, _, _, x0, y0) in enumerate(plan.tiles):
        win = whole[(i, l)][:, y0:y0 + TH, x0:x0 + TW]
        ref = np.zeros((3, TH, TW), dtype=np.float32)
        ref[:, :win.shape[1], :win.shape[2]] = win
        overhang += ref[0].size - win[0].size
        assert np.array_equal(bits(got[t]), bits(ref)), (t, i, l)
    assert overhang > 0


def hand_made_tiles():
    """Descriptors no planner makes: a 10 x 15 canvas overhung at both ends of both axes, photo indices out of range, a canvas
    without pixels, and two ordinary windows -- an odd number, so the last block is partial."""
    photos = photos_np()
    rows = [(0, -4, -3, 15, 10), (1, -2, 5, 21, 32), (2, 0, 0, 20, 20), (-1, 0, 0, 20, 20), (0, 0, 0, 0, 0), (1, 8, 40, 41, 64),
            (0, 30, 30, 53, 37)]
    descs = (TileDesc * len(rows))()
    for d, (image, x0, y0, wc, hc) in zip(descs, rows):
        d.image, d.x0, d.y0, d.wc, d.hc = image, x0, y0, wc, hc
        if 0 <= image < 2 and wc > 0:
            h, w = photos[image].shape[:2]
            d.scale_x, d.scale_y = 1.0 / (float(wc) / float(w)), 1.0 / (float(hc) / float(h))
    return photos, descs


def test_tile_sample_at_the_c_abi_overhang_bad_index_guards_and_no_tiles():
    lib = _lib.load()
    photos, descs = hand_made_tiles()
    T = len(descs)
    src = torch.cat([torch.from_numpy(p.reshape(-1)) for p in photos]).cuda()
    table = (CropImage * 2)()
    at = 0
    for e, p in zip(table, photos):
        e.offset, e.pitch, e.h, e.w = at, p.shape[1] * 3, p.shape[0], p.shape[1]
        at += p.size
    table_d, descs_d = on_device(table), on_device(descs)
    n = T * 3 * TH * TW
    buf = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device="cuda")
    dst = buf[GUARD:GUARD + n]
    dst.fill_(float('nan'))
    stream = torch.cuda.current_stream().cuda_stream
    args = (RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2])
    assert lib.mr_tile_sample(src.data_ptr(), table_d.data_ptr(), 2, descs_d.data_ptr(), 0, TH, TW, *args, dst.data_ptr(), stream) == 0
    assert lib.mr_tile_sample(None, None, 0, None, 0, TH, TW, *args, None, stream) == 0                  # T == 0: no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())
    assert lib.mr_tile_sample(src.data_ptr(), table_d.data_ptr(), 2, descs_d.data_ptr(), T, TH, TW, *args, dst.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(T, 3, TH, TW)
    assert not np.isnan(got).any()
    assert bool((buf[:GUARD] == 7.0).all()) and bool((buf[GUARD + n:] == 7.0).all())
    want = R.tile_sample_ref(photos, R.entries(descs), TH, TW)
    assert np.array_equal(bits(got), bits(want))
    assert not got[2].any() and not got[3].any() and not got[4].any()            # out-of-range photos, an empty canvas: 0.0f
    assert (T * TH * TW) % 256 != 0                                              # the last block was partial
    inside = np.zeros((TH, TW), dtype=bool)
    inside[3:13, 4:19] = True                                                    # the 10 x 15 canvas seen from (-4, -3)
    assert (got[0] != 0)[:, inside].all() and not got[0][:, ~inside].any()
    for bad in ((None, table_d.data_ptr(), 2, descs_d.data_ptr(), T, TH, TW), (src.data_ptr(), table_d.data_ptr(), 2, None, T, TH, TW),
                (src.data_ptr(), table_d.data_ptr(), 2, descs_d.data_ptr(), T, 0, TW),
                (src.data_ptr(), table_d.data_ptr(), -1, descs_d.data_ptr(), T, TH, TW),
                (src.data_ptr(), table_d.data_ptr(), 2, descs_d.data_ptr(), 1 << 20, 32, 32)):     # T*th*tw*3 >= 2^31
        assert lib.mr_tile_sample(*bad, *args, dst.data_ptr(), stream) == 1, bad
        assert b"mr_tile_sample" in lib.mr_last_error()
    assert lib.mr_tile_sample(src.data_ptr(), table_d.data_ptr(), 2, descs_d.data_ptr(), T, TH, TW, *args, None, stream) == 1
    assert lib.mr_sizeof_tile_desc() == ctypes.sizeof(TileDesc) == 40
    assert lib.mr_sizeof_stitch_level() == ctypes.sizeof(StitchLevel) == 40
    assert lib.mr_sizeof_stitch_photo() == ctypes.sizeof(StitchPhoto) == 32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fuse", ['max', 'mean'])
@pytest.mark.parametrize("scales", [(1.0,), ('fit', 1.0), (0.5, 1.0, 2.0)])
def test_stitched_maps_equal_the_restatement(scales, fuse, dtype):
    tiler = DetectionTiler(tile=(TH, TW), halo=HALO, scales=scales, fuse=fuse, align=4)
    plan = tiler.plan([(37, 53), (64, 41)])
    assert plan.sizes == ([(36, 52), (64, 40)] if max(s for s in scales if s != 'fit') == 1.0 else [(76, 108), (128, 84)])
    torch.manual_seed(7)
    maps = torch.rand((plan.T, 1, TH, TW), device="cuda").to(dtype)
    buf = torch.full((plan.total + 2 * GUARD,), 7.0, dtype=torch.float32, device="cuda")
    body = buf[GUARD:GUARD + plan.total]
    body.fill_(float('nan'))
    views = tiler.stitch(plan, maps, out=body)
    first = body.cpu().numpy().copy()
    assert not np.isnan(first).any()                                             # every pixel of every fused map was written
    assert bool((buf[:GUARD] == 7.0).all()) and bool((buf[GUARD + plan.total:] == 7.0).all())
    levels, photos, _ = plan.stitch_tables()
    want = R.tile_stitch_ref(maps.float().cpu().numpy(), TH, TW, HALO, R.entries(levels), R.entries(photos, 2), fuse,
                             np.full(plan.total, np.nan, dtype=np.float32))
    assert np.array_equal(bits(first), bits(want))
    assert [tuple(v.shape) for v in views] == [(1, 1) + s for s in plan.sizes]
    assert np.array_equal(bits(views[1].cpu().numpy().reshape(-1)), bits(want[plan.offsets[1]:]))
    body.fill_(float('nan'))
    tiler.stitch(plan, maps, out=body)
    assert np.array_equal(bits(body.cpu().numpy()), bits(first))                 # run to run


def test_tile_stitch_argument_errors():
    lib = _lib.load()
    tiler = DetectionTiler(tile=(TH, TW), halo=HALO, scales=(1.0,), align=4)
    plan = tiler.plan([(37, 53)])
    levels, photos, max_pixels = plan.stitch_tables()
    lv, ph = on_device(levels), on_device(photos)
    maps = torch.zeros((plan.T, TH, TW), device="cuda")
    out = torch.full((plan.total,), float('nan'), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(dtype=0, maps=maps.data_ptr(), T=plan.T, th=TH, tw=TW, hy=4, hx=4, levels=lv.data_ptr(), L=1, photos=ph.data_ptr(),
                P=1, max_pixels=max_pixels, fuse=0, out=out.data_ptr(), out_elems=plan.total)
    for change, code in ((dict(maps=None), 1), (dict(levels=None), 1), (dict(photos=None), 1), (dict(out=None), 1),
                         (dict(th=0), 1), (dict(hy=8), 1), (dict(hx=12), 1), (dict(hx=-1), 1), (dict(fuse=2), 1),
                         (dict(max_pixels=0), 1), (dict(T=-1), 1), (dict(T=1 << 20, th=64, tw=64), 1), (dict(dtype=5), 2)):
        assert lib.mr_tile_stitch(*dict(good, **change).values(), stream) == code, change
        assert b"mr_tile_stitch" in lib.mr_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                          # nothing was written
    assert lib.mr_tile_stitch(*dict(good, P=0, photos=None, levels=None, out=None).values(), stream) == 0       # no launch
    short = dict(good, out_elems=plan.total - 1)                                 # a map that does not fit is skipped
    assert lib.mr_tile_stitch(*short.values(), stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert lib.mr_tile_stitch(*good.values(), stream) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    with pytest.raises(ValueError):
        tiler.stitch(plan, torch.zeros((plan.T, 1, TH, TW + 1), device="cuda"))


# ---- the invariant --------------------------------------------------------------------------------------------------------
SHAPE, TILE, REACH = (83, 131), (32, 48), 8
WEIGHTS = [[0.25, -0.5, 0.125], [0.75, 1.0, -0.375], [-0.625, 0.5, 0.0625]]


def pointwise(x):
    return torch.sigmoid(x[:, :1])


def three_by_three(x):
    """A 3 x 3 filter of channel 0 from zero-padded shifted slices, multiplied and added one by one in a fixed order (not conv2d,
    whose algorithm may change with the shape), then sigmoid: reach 1, zero padding, equivariant under every shift."""
    c = x[:, :1]
    H, W = c.shape[2:]
    p = torch.nn.functional.pad(c, (1, 1, 1, 1))
    acc = None
    for dy in range(3):
        for dx in range(3):
            term = p[:, :, dy:dy + H, dx:dx + W] * WEIGHTS[dy][dx]
            acc = term if acc is None else acc + term
    return torch.sigmoid(acc)


@pytest.fixture(scope="module")
def scene():
    photo = np.random.RandomState(19).randint(0, 256, SHAPE + (3,)).astype(np.uint8)
    whole = DevicePipeline(image_size=SHAPE, mode='resize').process([photo], [''])['image']
    return photo, whole


@pytest.mark.parametrize("stub", [pointwise, three_by_three])
def test_a_tiled_detector_equals_the_detector_on_the_whole_canvas(scene, stub):
    photo, whole = scene
    tiler = DetectionTiler(tile=TILE, halo=(REACH, REACH), scales=(1.0,), align=1)
    fused = tiler.detect(stub, [photo], batch=8)
    assert len(fused) == 1 and fused[0].shape == (1, 1) + SHAPE and fused[0].dtype == torch.float32
    assert tiler.plan([SHAPE]).T == 5 * 4                                        # many tiles, chunks of 8, 8 and 4
    assert np.array_equal(bits(fused[0].cpu().numpy()), bits(stub(whole).cpu().numpy()))


def test_without_a_halo_the_three_by_three_detector_differs_on_core_borders(scene):
    photo, whole = scene
    tiler = DetectionTiler(tile=TILE, halo=(0, 0), scales=(1.0,), align=1)
    got = tiler.detect(three_by_three, [photo])[0].cpu().numpy()[0, 0]
    want = three_by_three(whole).cpu().numpy()[0, 0]
    differs = bits(got) != bits(want)
    assert differs.any()                                                         # the test above can fail
    rows = np.zeros(SHAPE[0], dtype=bool)
    cols = np.zeros(SHAPE[1], dtype=bool)
    for k in range(1, 3):                                                        # tiles of 32 x 48 side by side: borders at k * side
        rows[[k * TILE[0] - 1, k * TILE[0]]] = True
        cols[[k * TILE[1] - 1, k * TILE[1]]] = True
    assert not differs[~rows][:, ~cols].any()                                    # ... and only there


def test_a_detector_whose_map_is_not_tile_sized_is_refused(scene):
    tiler = DetectionTiler(tile=TILE, halo=(REACH, REACH), scales=(1.0,), align=1)
    with pytest.raises(ValueError) as e:
        tiler.detect(lambda x: x[:, :1, ::4, ::4], [scene[0]])
    assert "tile-sized" in str(e.value)
