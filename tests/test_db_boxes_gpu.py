"""`mr_db_boxes` (csrc/db_post.hip): the DB post-processing after the labelling, on the device.  The kernels are held equal to
their restatement in tests/_db_boxes_ref.py BIT FOR BIT -- candidate rectangles, (sum, count), statuses, boxes, scores, counts --
and `SegDetectorRepresenter(device_geometry=True)` to the host path and to oracle/db_post.py as identical lists.  The
restatement itself is held to the oracle without a GPU in tests/test_db_boxes_cpu.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _db_boxes_ref as R  # noqa: E402
from megreader_amd._lib import call, load, ptr, stream_ptr  # noqa: E402
from megreader_amd.structure import SegDetectorRepresenter  # noqa: E402
from oracle import db_post as O  # noqa: E402

DEV = "cuda"


def ws_bytes(N, H, W, K):
    n = ctypes.c_longlong(-1)
    rc = load().mr_db_boxes_ws_bytes(N, H, W, K, ctypes.byref(n))
    return rc, n.value


def db_boxes(prob, seg, thr, dest, K=100, box_thresh=0.7, min_size=3.0):
    """mr_db_boxes with every optional output, as numpy arrays named like `_db_boxes_ref.db_boxes`'s."""
    prob_d = torch.from_numpy(np.array(prob, dtype=np.float32)).to(DEV)
    seg_d = prob_d if seg is prob else torch.from_numpy(np.array(seg, dtype=np.float32)).to(DEV)
    N, H, W = prob.shape
    rc, nbytes = ws_bytes(N, H, W, K)
    assert rc == 0 and nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = {'boxes': torch.full((N, K, 4, 2), -7.0, dtype=torch.float64, device=DEV),
           'scores': torch.full((N, K), -7.0, dtype=torch.float32, device=DEV),
           'count': torch.full((N,), -7, dtype=torch.int32, device=DEV),
           'components': torch.full((N,), -7, dtype=torch.int32, device=DEV),
           'cand': torch.full((N, K, 4, 2), -7.0, dtype=torch.float64, device=DEV),
           'cand_sums': torch.full((N, K, 2), -7.0, dtype=torch.float32, device=DEV),
           'status': torch.full((N, K), -7, dtype=torch.int32, device=DEV)}
    dest_d = torch.tensor(dest, dtype=torch.int32, device=DEV)
    call("mr_db_boxes", ptr(prob_d), ptr(seg_d), float(thr), ptr(dest_d), N, H, W, K, float(box_thresh), float(min_size), ptr(ws),
         ptr(out['boxes']), ptr(out['scores']), ptr(out['count']), ptr(out['components']), ptr(out['cand']),
         ptr(out['cand_sums']), ptr(out['status']))
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(got, want, what=""):
    for name in ('components', 'status', 'cand', 'cand_sums', 'count', 'boxes', 'scores'):
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]).astype(got[name].dtype)
        assert g.shape == w.shape, (what, name)
        bad = np.argwhere(g.view(np.uint8).reshape(g.shape + (-1,)) != w.view(np.uint8).reshape(w.shape + (-1,)))
        assert len(bad) == 0, (what, name, bad[:4].tolist(), g[tuple(bad[0][:-1])], w[tuple(bad[0][:-1])])


@functools.lru_cache(maxsize=None)
def _maps(seed):
    maps = O.synthetic_maps(seed, N=3, H=96, W=128, regions=7)
    maps.setflags(write=False)
    return maps


SHAPES3 = [(192, 384), (100, 130), (97, 201)]          # (height, width) of the three "original images"


@pytest.mark.parametrize("seed", [3, 4, 5, 6])
def test_kernels_equal_the_restatement_bit_for_bit(seed):
    maps = _maps(seed)
    dest = [(w, h) for h, w in SHAPES3]
    got = db_boxes(maps, maps, 0.3, dest)
    want = R.db_boxes(maps, maps > 0.3, dest)
    same_bits(got, want, seed)
    assert int(got['count'].sum()) >= 3 and (got['status'] == R.WEAK).any() and (got['status'] == R.SHORT).any()
    # (sum, count) are the bits of mr_db_box_scores on the same candidates
    scored = np.argwhere(got['status'] >= R.WEAK)
    rows = np.array([[n] + [float(int(v)) for v in got['cand'][n, k].reshape(-1)] for n, k in scored], dtype=np.float32)
    out = torch.empty((len(rows), 2), dtype=torch.float32, device=DEV)
    prob_d, rows_d = torch.from_numpy(np.array(maps)).to(DEV), torch.from_numpy(rows).to(DEV)
    call("mr_db_box_scores", ptr(prob_d), ptr(rows_d), ptr(out), len(rows), 3, 96, 128)
    assert out.cpu().numpy().tobytes() == np.stack([got['cand_sums'][n, k] for n, k in scored]).tobytes()


@pytest.mark.parametrize("seed", [3, 4, 5, 6])
def test_device_geometry_gives_the_lists_of_the_host_path_and_the_oracle(seed):
    maps = _maps(seed)
    pred = {'binary': torch.from_numpy(np.array(maps)).to(DEV).unsqueeze(1)}
    batch = {'image': torch.empty(3, 3, 96, 128), 'shape': SHAPES3}
    dev_boxes, out = SegDetectorRepresenter(resize=True, device_geometry=True).represent(batch, pred)
    host_boxes, _ = SegDetectorRepresenter(resize=True).represent(batch, pred)
    assert out is pred
    want = [O.boxes_from_bitmap(maps[n], maps[n] > 0.3, SHAPES3[n][1], SHAPES3[n][0], resize=True) for n in range(3)]
    assert dev_boxes == host_boxes == want
    assert sum(len(b) for b in want) >= 3
    plain, _ = SegDetectorRepresenter(device_geometry=True).represent(batch, pred)          # resize=False: the map's own size
    assert plain == [O.boxes_from_bitmap(maps[n], maps[n] > 0.3, 128, 96) for n in range(3)]


def test_max_candidates_cuts_in_raster_order_and_components_tells():
    maps = _maps(3)
    n_comp = [len(O.components(maps[n] > 0.3)) for n in range(3)]
    assert min(n_comp) > 5
    got = db_boxes(maps, maps, 0.3, [(128, 96)] * 3, K=5)
    same_bits(got, R.db_boxes(maps, maps > 0.3, [(128, 96)] * 3, K=5))
    assert got['components'].tolist() == n_comp and (got['status'] != R.NONE).all()
    rep = SegDetectorRepresenter(max_candidates=5, device_geometry=True)
    pred = {'binary': torch.from_numpy(np.array(maps)).to(DEV).unsqueeze(1)}
    boxes, _ = rep.represent({'image': None, 'shape': [(96, 128)] * 3}, pred)
    assert boxes == [O.boxes_from_bitmap(maps[n], maps[n] > 0.3, 128, 96, max_candidates=5) for n in range(3)]
    assert rep.boxes_on_device(pred['binary'], None, None)['components'].tolist() == n_comp


def test_dest_map_other_than_binary_and_the_bitmap_path():
    maps, other = _maps(4), _maps(5)
    # regions from `other`, scores from `maps`
    got = db_boxes(maps, other, 0.3, [(128, 96)] * 3)
    same_bits(got, R.db_boxes(maps, other > 0.3, [(128, 96)] * 3))
    assert (got['status'] == R.WEAK).any()
    dev = SegDetectorRepresenter(dest='thresh_binary', device_geometry=True)
    host = SegDetectorRepresenter(dest='thresh_binary')
    pred = {'binary': torch.from_numpy(np.array(maps)).to(DEV).unsqueeze(1),
            'thresh_binary': torch.from_numpy(np.array(other)).to(DEV).unsqueeze(1)}
    batch = {'image': None, 'shape': [(96, 128)] * 3}
    assert dev.represent(batch, pred)[0] == host.represent(batch, pred)[0] == R.box_lists(got)
    # reference signature with an already binarised map
    one = torch.from_numpy(np.array(maps[:1])).to(DEV)
    boxes, bitmap = dev.boxes_from_bitmap(one, dev.binarize(one), 128, 96)
    assert boxes == O.boxes_from_bitmap(maps[0], maps[0] > 0.3, 128, 96) and bitmap.shape == (96, 128)


def _ring(H, W, cx, cy, r0, r1):
    yy, xx = np.mgrid[0:H, 0:W]
    d = (xx - cx) ** 2 + (yy - cy) ** 2
    return (d >= r0 * r0) & (d <= r1 * r1)


def _edge_cases():
    g = np.random.default_rng(7)
    cases = {}
    cases['37 x 53'] = O.synthetic_maps(13, N=2, H=37, W=53, regions=4)
    cases['empty'] = np.zeros((2, 24, 40), np.float32)
    cases['full'] = np.full((1, 64, 64), 0.9, np.float32)
    ring = _ring(80, 96, 47, 39, 18, 28)
    c = ring.copy()
    c[30:50, 60:] = False
    cases['ring and C'] = np.stack([ring, c]).astype(np.float32) * 0.9
    bar = np.zeros((1, 200, 64), np.float32)
    bar[0, :, 20:31] = 0.95                                     # spans all 200 rows
    bar[0, 5, 3] = bar[0, 6, 4] = bar[0, 100, 50] = 0.95       # a two-pixel and a one-pixel component
    bar[0, 150, 40:60] = 0.95                                   # a 1 x 20 line
    cases['bar over all rows'] = bar
    cases['N = 1'] = O.synthetic_maps(10, N=1, H=96, W=128, regions=7)
    wide = np.zeros((1, 8, 700), np.float32)                    # more than 256 hull edges cannot happen here, many rows of runs can
    wide[0, 2:7, 5:690] = 0.8
    cases['wide'] = wide
    noisy = (g.uniform(0, 1, (1, 48, 300)) < 0.45).astype(np.float32) * 0.9   # one ragged component with many runs per row
    cases['ragged'] = noisy
    cases['lens outline'] = R.lens_outline()[None].astype(np.float32) * 0.9    # 264 hull edges: two rounds of the calipers
    tall = np.zeros((1, 2048, 16), np.float32)                  # the largest H: 4 096 points, 60 KB of LDS
    tall[0, :, 5:12] = 0.9
    tall[0, 700:1400, 4] = tall[0, 1000, 13] = 0.9
    tall[0, 10, 1] = tall[0, 2047, 14] = 0.9
    cases['H = 2048'] = tall
    return cases


EDGE = _edge_cases()


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_shapes(name):
    maps = EDGE[name]
    N, H, W = maps.shape
    dest = [(2 * W + 3, H + 5)] * N
    got = db_boxes(maps, maps, 0.3, dest)
    want = R.db_boxes(maps, maps > 0.3, dest)
    same_bits(got, want, name)
    if name == 'empty':
        assert got['count'].tolist() == [0, 0] and got['components'].tolist() == [0, 0] and not got['boxes'].any()
    if name in ('full', 'bar over all rows', 'wide', '37 x 53', 'N = 1', 'H = 2048'):
        assert got['count'].max() >= 1
    if name == 'ring and C':                                    # the hole and the opening count against the score
        assert got['status'][:, 0].tolist() == [R.WEAK, R.WEAK] and got['components'].tolist() == [1, 1]
    if name == 'lens outline':          # (its hull against convex_hull: tests/test_db_boxes_cpu.py; the oracle's pixel loops are slow here)
        assert got['status'][0, 0] == R.WEAK and got['components'][0] == 1
        return
    for n in range(N):
        assert R.box_lists(got)[n] == O.boxes_from_bitmap(maps[n], maps[n] > 0.3, dest[n][0], dest[n][1], resize=True), n


def test_other_thresholds_and_a_box_too_small_after_unclip():
    maps = np.array(_maps(3)[:1])
    maps[0, 2:5, 2:5] = 0.9              # 3 x 3 pixels: side 2, unclipped 3.5 < 2 + 2; slot 1, behind a speck
    got = db_boxes(maps, maps, 0.5, [(128, 96)], K=40, box_thresh=0.5, min_size=2.0)
    same_bits(got, R.db_boxes(maps, maps > 0.5, [(128, 96)], K=40, box_thresh=0.5, min_size=2.0))
    assert got['status'][0, 1] == R.SMALL and got['status'][0, 0] == R.SHORT and got['count'][0] >= 2


def test_two_calls_give_equal_bits():
    maps = _maps(6)
    a = db_boxes(maps, maps, 0.3, [(128, 96)] * 3)
    b = db_boxes(maps, maps, 0.3, [(128, 96)] * 3)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_represent_scored():
    maps = _maps(5)
    pred = {'binary': torch.from_numpy(np.array(maps)).to(DEV).unsqueeze(1)}
    batch = {'image': None, 'shape': SHAPES3}
    raw = db_boxes(maps, maps, 0.3, [(w, h) for h, w in SHAPES3])
    for device_geometry in (False, True):
        rep = SegDetectorRepresenter(resize=True, device_geometry=device_geometry)
        boxes, scores, out = rep.represent_scored(batch, pred)
        assert out is pred and boxes == rep.represent(batch, pred)[0]
        for n in range(3):
            kept = raw['cand_sums'][n][raw['status'][n] == R.KEPT]
            assert scores[n] == [float(np.float32(np.float64(s) / np.float64(c))) for s, c in kept]
            assert len(scores[n]) == len(boxes[n]) and all(0.7 <= s <= 1.0 for s in scores[n])
    assert sum(len(s) for s in scores) >= 3
    dev = rep.boxes_on_device(pred['binary'], None, SHAPES3)
    assert all(dev[k].is_cuda for k in ('boxes', 'scores', 'count', 'components'))
    assert dev['boxes'].shape == (3, 100, 4, 2) and dev['scores'].dtype == torch.float32


@pytest.mark.parametrize("K,H", [(0, 32), (1025, 32), (100, 2049)])
def test_argument_errors(K, H):
    assert ws_bytes(1, H, 16, K)[0] != 0
    t = torch.zeros(64, device=DEV)
    rc = load().mr_db_boxes(ptr(t), ptr(t), 0.3, ptr(t), 1, H, 16, K, 0.7, 3.0, ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 0, 0, 0,
                            stream_ptr())
    assert rc == 1 and b"mr_db_boxes" in load().mr_last_error()          # MR_ERR_ARG, nothing launched


def test_cpu_tensors_are_refused():
    cpu = torch.zeros(1, 1, 32, 32)
    for rep in (SegDetectorRepresenter(device_geometry=True), SegDetectorRepresenter()):
        with pytest.raises(NotImplementedError):
            rep.boxes_on_device(cpu, None, [(32, 32)])
        with pytest.raises(NotImplementedError):
            rep.represent_scored({'image': cpu, 'shape': [(32, 32)]}, {'binary': cpu})
    with pytest.raises(NotImplementedError):
        SegDetectorRepresenter(device_geometry=True).represent({'image': cpu, 'shape': [(32, 32)]}, {'binary': cpu})
