"""mr_db_targets (csrc/db_targets.hip) against the float64 restatement of tests/_db_targets_ref.py (itself checked against
hand-computed answers in tests/test_db_targets_cpu.py).

Comparison: `ignore_out` and `dist` exactly; `gt`, `mask` and `thresh_mask` exactly, except at pixels where the
restatement's own decision margin is below 1e-9 relative to max(1, D^2) -- and every case asserts that there is NO such
pixel (the seeds and the coordinates of the targeted quads were chosen on the CPU so that the restatement reports none);
`thresh_map` within 2e-7: two float32 ulps below 1 are 1.2e-7 -- one for a last-bit difference of the device's float64
sqrt or divide in front of the rounding to float32, one for the float32 multiply-add behind it.  The outputs are filled
with NaN before every call: none may survive."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _db_targets_ref as R  # noqa: E402
from megreader_amd._lib import call, load, ptr, stream_ptr  # noqa: E402

MR_ERR_UNSUPPORTED = 4
MAPS = ('gt', 'mask', 'thresh_map', 'thresh_mask')


def device_targets(polys, count, tags, H, W, min_text_size=8.0, shrink_ratio=0.4, thresh_min=0.3, thresh_max=0.7):
    dev = torch.device("cuda")
    polys = np.ascontiguousarray(polys, dtype=np.float64)
    N, G = polys.shape[:2]
    d_polys = torch.from_numpy(polys).to(dev)
    d_count = torch.tensor(list(count), dtype=torch.int32, device=dev)
    d_tags = torch.from_numpy(np.ascontiguousarray(tags, dtype=np.int32).reshape(N, G)).to(dev)
    records = torch.zeros((max(N * G * load().mr_sizeof_db_record(), 8),), dtype=torch.uint8, device=dev)
    ignore = torch.full((N, G), -7, dtype=torch.int32, device=dev)
    dist = torch.full((N, G), float('nan'), dtype=torch.float64, device=dev)
    out = {'gt': torch.full((N, 1, H, W), float('nan'), device=dev)}
    for k in MAPS[1:]:
        out[k] = torch.full((N, H, W), float('nan'), device=dev)
    call("mr_db_targets", ptr(d_polys), ptr(d_count), ptr(d_tags), N, G, H, W, float(min_text_size), float(shrink_ratio),
         float(thresh_min), float(thresh_max), ptr(records), ptr(ignore), ptr(dist), ptr(out['gt']), ptr(out['mask']),
         ptr(out['thresh_map']), ptr(out['thresh_mask']))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['ignore_out'], res['dist'] = ignore.cpu().numpy(), dist.cpu().numpy()
    return res


def compare(got, ref, count):
    for n, c in enumerate(count):                       # slots past the count: flag 0, distance 0
        assert (got['ignore_out'][n, c:] == 0).all() and (got['dist'][n, c:] == 0).all()
    np.testing.assert_array_equal(got['ignore_out'], ref['ignore_out'])
    np.testing.assert_array_equal(got['dist'], ref['dist'])
    for k in MAPS:
        assert not np.isnan(got[k]).any(), "%s: a pre-filled NaN survived" % k
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float32
    skipped = {k: int(v.sum()) for k, v in ref['skip'].items()}
    assert skipped == {'gt': 0, 'mask': 0, 'thresh_mask': 0}, "pixels without a decision margin: %s" % skipped
    for k in ('gt', 'mask', 'thresh_mask'):
        bad = np.argwhere(got[k].reshape(ref['skip'][k].shape) != ref[k].reshape(ref['skip'][k].shape))
        assert len(bad) == 0, "%s differs at %d pixels, first (n, y, x) = %s" % (k, len(bad), bad[0])
    err = float(np.abs(got['thresh_map'].astype(np.float64) - ref['thresh_map']).max())
    print("thresh_map max |diff| %.3e" % err)
    assert err <= 2e-7


# ---- hand cases (tests/test_db_targets_cpu.py), on the device -------------------------------------------------------------

def test_hand_rectangle():
    H, W = 48, 64
    polys = np.array([[[[10, 10], [50, 10], [50, 30], [10, 30]]]], dtype=np.float64)
    got = device_targets(polys, [1], [[0]], H, W)
    assert got['dist'][0, 0] == 5.6 and got['ignore_out'][0, 0] == 0
    expect = np.zeros((H, W), dtype=np.float32)
    expect[16:25, 16:45] = 1
    np.testing.assert_array_equal(got['gt'][0, 0], expect)
    tm = got['thresh_mask'][0]
    assert tm[6, 7] == 1 and tm[7, 6] == 1 and tm[6, 6] == 0 and tm[34, 54] == 0 and tm[33, 54] == 1
    assert tm.sum() == 21 * 51 + 2 * sum(41 + 2 * int(np.sqrt(5.6 ** 2 - k * k)) for k in range(1, 6))
    f = np.float32
    th = got['thresh_map'][0]
    assert abs(float(th[10, 30]) - 0.7) <= 1.2e-7 and abs(float(th[20, 10]) - 0.7) <= 1.2e-7
    assert th[20, 30] == f(0.3) and th[4, 30] == f(0.3) and th[0, 0] == f(0.3)
    assert abs(float(th[7, 30]) - (0.3 + 0.4 * (1 - 3 / 5.6))) <= 2e-7
    assert got['mask'].min() == 1
    compare(got, R.db_targets_ref(polys, [1], [[0]], H, W), [1])


def test_hand_other_cases():
    H, W = 48, 64
    quad = [[12.3, 9.1], [48.7, 13.4], [46.2, 33.9], [9.8, 29.5]]
    polys = np.array([[quad], [[quad[0], quad[3], quad[2], quad[1]]],                     # clockwise / counter-clockwise
                      [[[10.5, 10.5], [40.5, 10.5], [40.5, 17.5], [10.5, 17.5]]],        # a side below 8
                      [[[40, -10], [90, -10], [90, 20], [40, 20]]]], dtype=np.float64)   # over the border
    count, tags = [1, 1, 1, 1], np.zeros((4, 1), dtype=np.int32)
    got = device_targets(polys, count, tags, H, W)
    for k in MAPS:
        np.testing.assert_array_equal(got[k][0], got[k][1])
    assert got['ignore_out'][:, 0].tolist() == [0, 0, 1, 0]
    assert got['gt'][2].sum() == 0 and got['thresh_mask'][2].sum() == 0 and got['mask'][2].sum() == H * W - 8 * 31
    assert got['dist'][3, 0] == 0.84 * (23 * 20) / (2 * 23 + 2 * 20)
    compare(got, R.db_targets_ref(polys, count, tags, H, W), count)


# ---- random quads -----------------------------------------------------------------------------------------------------------

def random_quads(rng, k, H, W):
    """Rotated, jittered rectangles; some reach over the border, some sides fall below min_text_size."""
    cx, cy = rng.uniform(-4, W + 4, k), rng.uniform(-4, H + 4, k)
    hw, hh = rng.uniform(6, 0.3 * W, k), rng.uniform(4, 14, k)
    th = rng.uniform(-np.pi, np.pi, k)
    corners = np.stack([np.stack([-hw, -hh], -1), np.stack([hw, -hh], -1), np.stack([hw, hh], -1), np.stack([-hw, hh], -1)], 1)
    rot = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], 1)      # [k, 2, 2]
    pts = np.einsum('kij,kvj->kvi', rot, corners) + np.stack([cx, cy], -1)[:, None, :]
    pts = pts + rng.uniform(-2, 2, pts.shape)
    flip = rng.rand(k) < 0.5                                                               # both orientations
    pts[flip] = pts[flip][:, [0, 3, 2, 1]]
    return pts, (rng.rand(k) < 0.2).astype(np.int32)


@functools.lru_cache(maxsize=None)
def random_case(H, W, counts, seed, ratio):
    rng = np.random.RandomState(seed)
    G = max(counts)
    polys = np.zeros((len(counts), G, 4, 2))
    tags = np.zeros((len(counts), G), dtype=np.int32)
    for n, c in enumerate(counts):
        polys[n, :c], tags[n, :c] = random_quads(rng, c, H, W)
    return polys, tags, R.db_targets_ref(polys, counts, tags, H, W, shrink_ratio=ratio)


@pytest.mark.parametrize("ratio", [0.4, 0.7])
@pytest.mark.parametrize("H,W", [(96, 80), (33, 130), (128, 160)])
def test_random_quads(H, W, ratio):
    counts = (0, 1, 37)
    polys, tags, ref = random_case(H, W, counts, 11, ratio)
    assert 0 < ref['ignore_out'].sum() < 38 and ref['gt'].sum() > 0 and ref['mask'].min() == 0
    compare(device_targets(polys, counts, tags, H, W, shrink_ratio=ratio), ref, counts)


@pytest.mark.parametrize("ratio", [0.4, 0.7])
def test_random_quads_wrap_the_chunk(ratio):
    """300 polygons in one image: the map kernel stages 256 records per pass, so the second pass holds 44."""
    H, W, counts = 128, 160, (300, 5)
    polys, tags, ref = random_case(H, W, counts, 12, ratio)
    assert ref['ignore_out'][0, 256:].sum() > 0 and (ref['ignore_out'][0, 256:] == 0).sum() > 0
    compare(device_targets(polys, counts, tags, H, W, shrink_ratio=ratio), ref, counts)


# ---- targeted quads ---------------------------------------------------------------------------------------------------------

TARGETED = [
    # (quads, tags, expected final flags)
    ([[[10.2, 10.4], [60.2, 40.4], [60.2, 10.4], [10.2, 40.4]]], [0], [1]),                 # bow-tie: |a| < 1
    ([[[10.3, 10.6], [40.2, 30.4], [70.7, 12.1], [40.9, 70.3]]], [0], [0]),                 # dart (non-convex)
    ([[[40.4, 5.3], [90.2, -8.0], [100.6, -3.0], [45.7, 40.2]]], [0], [1]),                 # two vertices coincide after the clip
    ([[[20.0, 15.0], [60.3, 18.2], [57.1, 40.6], [17.4, 37.9]]], [0], [0]),                 # a vertex exactly on a pixel
    ([[[10.5, 10.3], [50.5, 10.3], [58.5, 10.9], [18.5, 10.9]]], [0], [1]),                 # thin shear: covers no pixel
    ([[[8.3, 12.6], [52.4, 9.2], [55.1, 38.7], [11.9, 42.3]],
      [[30.6, 25.2], [72.3, 30.8], [69.7, 58.4], [27.2, 52.9]]], [0, 0], [0, 0]),           # two kept quads overlap: max and OR
    ([[[8.3, 12.6], [52.4, 9.2], [55.1, 38.7], [11.9, 42.3]],
      [[30.6, 25.2], [72.3, 30.8], [69.7, 58.4], [27.2, 52.9]]], [0, 1], [0, 1]),           # kept over ignored
]


@functools.lru_cache(maxsize=None)
def targeted_case():
    H, W = 96, 80
    polys = np.zeros((len(TARGETED), 2, 4, 2))
    tags = np.zeros((len(TARGETED), 2), dtype=np.int32)
    counts = tuple(len(q) for q, _, _ in TARGETED)
    for n, (q, t, _) in enumerate(TARGETED):
        polys[n, :len(q)], tags[n, :len(q)] = q, t
    return H, W, polys, tags, counts, R.db_targets_ref(polys, counts, tags, H, W)


def test_targeted_quads():
    H, W, polys, tags, counts, ref = targeted_case()
    for n, (q, _, flags) in enumerate(TARGETED):
        assert ref['ignore_out'][n, :len(q)].tolist() == flags, n
    assert ref['gt'][1].sum() > 0 and ref['gt'][4].sum() == 0
    assert ref['dist'][4, 0] == 0 and ref['mask'][4, 10, 10:59].sum() == 0 and ref['mask'][4].sum() == H * W - 49    # zeroed along it
    both = (ref['gt'][5, 0] == 1).sum()
    assert 0 < (ref['gt'][6, 0] == 1).sum() < both and ref['mask'][6].min() == 0 and ref['mask'][5].min() == 1
    compare(device_targets(polys, counts, tags, H, W), ref, counts)


# ---- edges of the interface ---------------------------------------------------------------------------------------------------

def test_no_polygons():
    """G = 0 and an image with count 0: gt 0, mask 1, thresh_map = thresh_min, thresh_mask 0, all written by the kernel."""
    got = device_targets(np.zeros((2, 0, 4, 2)), [0, 0], np.zeros((2, 0), dtype=np.int32), 33, 70)
    assert (got['gt'] == 0).all() and (got['mask'] == 1).all() and (got['thresh_mask'] == 0).all()
    assert (got['thresh_map'] == np.float32(0.3)).all()


def test_too_many_slots():
    lib = load()
    one = torch.zeros((16,), dtype=torch.float64, device="cuda")
    rc = lib.mr_db_targets(0, 0, 0, 1, 1025, 8, 8, 8.0, 0.4, 0.3, 0.7, 0, 0, 0, ptr(one), ptr(one), ptr(one), ptr(one),
                           stream_ptr())
    assert rc == MR_ERR_UNSUPPORTED and b"1025" in lib.mr_last_error()
    torch.cuda.synchronize()
