"""`mr_db_ribbons` (csrc/db_post.hip) against its restatement tests/_db_ribbon_ref.py BIT FOR BIT -- ribbons, knots, why -- behind
`mr_db_boxes` on the same workspace, and what the call must leave alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _db_boxes_ref as B  # noqa: E402
import _db_ribbon_ref as R  # noqa: E402
from megreader_amd._lib import call, load, ptr, stream_ptr  # noqa: E402

DEV = "cuda"
N, H, W, K = 2, 96, 128, 8
GUARD = 32
BOX_THRESH = 0.2          # the score is the mean over the RECTANGLE: an arc fills about a third of its own


@functools.lru_cache(maxsize=None)
def _maps():
    """Two 96 x 128 maps: an arc, a tilted long bar, a short bar and a one-pixel component; a vertical bar, a long bar touching the
    border and more than K components."""
    a = R.paint_sector(H, W, (64.0, 70.0), 45, 9, 110.0)
    a |= R.paint_bar(H, W, (60.0, 76.0), 81, 9, 12.0)
    a |= R.paint_bar(H, W, (112.0, 60.0), 21, 9, 0.0)
    a[5, 120] = True
    b = R.paint_bar(H, W, (12.0, 48.0), 75, 9, 90.0)
    b |= R.paint_bar(H, W, (70.0, 3.0), 91, 9, 0.0)                    # rows 0 .. 7: touches the top border
    b |= R.paint_sector(H, W, (75.0, 90.0), 40, 8, 100.0)
    for i in range(10):                                                 # with the three above: more than K components
        b[90:95, 30 + 9 * i:35 + 9 * i] = True
    maps = np.stack([a, b]).astype(np.float32) * np.float32(0.9)
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def _want(S, dest):
    maps = _maps()
    boxes = B.db_boxes(maps, maps > 0.3, list(dest), K=K, box_thresh=BOX_THRESH)
    return boxes, R.db_ribbons(maps > 0.3, list(dest), boxes, S)


def run(S, dest, ratio=1.5):
    """mr_db_boxes, then mr_db_ribbons on its workspace; every output between guards.  Returns (boxes outputs, ribbon outputs,
    boxes outputs read again after the ribbons call, guards) as numpy arrays."""
    maps = torch.from_numpy(np.array(_maps())).to(DEV)
    nbytes, rbytes = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    assert load().mr_db_boxes_ws_bytes(N, H, W, K, ctypes.byref(nbytes)) == 0
    assert load().mr_db_ribbons_ws_bytes(N, K, ctypes.byref(rbytes)) == 0 and rbytes.value == N * K * 16 * 6 * 8
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    rws = torch.empty(rbytes.value, dtype=torch.uint8, device=DEV)
    box = {'boxes': torch.full((N, K, 4, 2), -7.0, dtype=torch.float64, device=DEV),
           'scores': torch.full((N, K), -7.0, dtype=torch.float32, device=DEV),
           'count': torch.full((N,), -7, dtype=torch.int32, device=DEV),
           'components': torch.full((N,), -7, dtype=torch.int32, device=DEV)}
    dest_d = torch.tensor(dest, dtype=torch.int32, device=DEV)
    call("mr_db_boxes", ptr(maps), ptr(maps), 0.3, ptr(dest_d), N, H, W, K, BOX_THRESH, 3.0, ptr(ws), ptr(box['boxes']),
         ptr(box['scores']), ptr(box['count']), ptr(box['components']), 0, 0, 0)
    before = {k: v.cpu().numpy() for k, v in box.items()}
    sizes = {'ribbons': N * K * 18 * 4, 'knots': N * K, 'why': N * K}
    dtypes = {'ribbons': torch.float64, 'knots': torch.int32, 'why': torch.int32}
    bufs = {k: torch.full((sizes[k] + 2 * GUARD,), -7, dtype=dtypes[k], device=DEV) for k in sizes}
    call("mr_db_ribbons", ptr(dest_d), N, H, W, K, S, ratio, ptr(ws), ptr(rws), bufs['ribbons'][GUARD:].data_ptr(),
         bufs['knots'][GUARD:].data_ptr(), bufs['why'][GUARD:].data_ptr())
    torch.cuda.synchronize()
    after = {k: v.cpu().numpy() for k, v in box.items()}
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    got = {'ribbons': host['ribbons'][GUARD:-GUARD].reshape(N, K, 18, 2, 2), 'knots': host['knots'][GUARD:-GUARD].reshape(N, K),
           'why': host['why'][GUARD:-GUARD].reshape(N, K)}
    guards = np.concatenate([np.concatenate([v[:GUARD], v[-GUARD:]]).astype(np.float64) for v in host.values()])
    return before, got, after, guards, rws.cpu().numpy().view(np.int64).reshape(N, K, 16, 6)


@pytest.mark.parametrize("S,dest", [(3, ((128, 96), (128, 96))), (8, ((301, 177), (128, 200))), (16, ((301, 177), (64, 48)))])
def test_kernel_equals_the_restatement_bit_for_bit(S, dest):
    want_boxes, want = _want(S, dest)
    before, got, after, guards, _ = run(S, dest)
    for name in ('boxes', 'scores', 'count', 'components'):
        assert before[name].tobytes() == want_boxes[name].astype(before[name].dtype).tobytes(), name
        assert after[name].tobytes() == before[name].tobytes(), name          # the call leaves mr_db_boxes' outputs alone
    for name in ('knots', 'why', 'ribbons'):
        g, w = got[name], want[name].astype(got[name].dtype)
        bad = np.argwhere(g.view(np.uint8).reshape(g.shape + (-1,)) != w.view(np.uint8).reshape(w.shape + (-1,)))
        assert len(bad) == 0, (S, name, bad[:4].tolist(), g[tuple(bad[0][:-1])], w[tuple(bad[0][:-1])])
    assert (guards == -7.0).all()
    count = before['count']
    for n in range(N):                                                       # zeros behind the last box and behind the used knots
        assert not got['ribbons'][n, count[n]:].any() and not got['knots'][n, count[n]:].any() and not got['why'][n, count[n]:].any()
        for j in range(count[n]):
            assert not got['ribbons'][n, j, got['knots'][n, j]:].any()
    assert ((got['knots'] == 0) | ((got['knots'] >= 5) & (got['knots'] <= S + 2))).all()


def test_the_maps_hold_every_case():
    want_boxes, want = _want(8, ((301, 177), (128, 200)))
    assert want_boxes['components'].tolist() == [4, 13] and want_boxes['count'][1] >= 3        # more than K = 8 components
    assert (want_boxes['status'][0] == B.SHORT).any()                                          # the one-pixel component
    c0, c1 = int(want_boxes['count'][0]), int(want_boxes['count'][1])
    assert c0 == 3 and sorted(want['why'][0, :3].tolist()) == [R.RIBBON, R.RIBBON, R.SHORT]     # arc, long bar; the short bar
    assert (want['knots'][1, :c1] > 0).sum() >= 3 and (want['why'][1, :c1] == R.SHORT).any()    # vertical, border, arc; the specks
    # the arc is the first box of image 0 (raster order); its interior centres lie on its circle (dest scales x by 301 / 128, y by
    # 177 / 96)
    k = int(want['knots'][0, 0])
    assert k >= 5
    rib = want['ribbons'][0, 0, :k] / np.array([301.0 / 128.0, 177.0 / 96.0])
    centres = rib.mean(axis=1)
    assert np.abs(np.sqrt(((centres[1:-1] - (64.0, 70.0)) ** 2).sum(axis=1)) - 45.0).max() <= 2.0


def test_slab_sums_and_two_calls_give_equal_bits():
    a = run(16, ((128, 96), (128, 96)))
    b = run(16, ((128, 96), (128, 96)))
    for x, y in zip(a[1].values(), b[1].values()):
        assert x.tobytes() == y.tobytes()
    maps = _maps()
    boxes, _ = _want(16, ((128, 96), (128, 96)))
    checked = 0
    for n in range(N):
        root, roots = B.label_components(maps[n] > 0.3)
        for k, r in enumerate(roots[:K]):
            if boxes['status'][n, k] != B.KEPT:
                continue
            ys, xs = np.nonzero(root == r)
            ref = R.ribbon_of(xs, ys, boxes['cand'][n, k].tolist(), 16)
            if ref['sums'] is not None:
                assert a[4][n, k, :len(ref['sums'])].tolist() == ref['sums'], (n, k)
                checked += 1
    assert checked >= 5


@pytest.mark.parametrize("S,ratio", [(2, 1.5), (17, 1.5), (0, 1.5), (8, -1.0), (8, float('nan'))])
def test_argument_errors(S, ratio):
    t = torch.zeros(4096, device=DEV)
    rc = load().mr_db_ribbons(ptr(t), 1, 16, 16, 4, S, ratio, ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), stream_ptr())
    assert rc == 1 and b"mr_db_ribbons" in load().mr_last_error()          # MR_ERR_ARG, nothing launched
