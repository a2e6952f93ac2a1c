"""Recorded all-taps weight gradients: several 3x3 problems in one launch (mr_tn_defer / mr_tn_flush, the TapsGroup form of
igemm_tn_taps_kernel in csrc/tn_taps.hip) through the C ABI.

Inside a recording bracket mr_conv2d_wgrad_tab queues the 3x3 / stride 1 layers that go to the all-taps kernel (reference:
the conv2..conv5 layers of backbones/crnn.py:44-55, the bottleneck 3x3 layers of backbones/resnet.py:110-140) and the flush
packs them into launches with fewer splits each.  Operands are small integers, so every product and partial sum is exact in
bf16 / f32: dW and dbias must EQUAL float64 arithmetic bit for bit, whatever the partition, the split counts, the slab
groups and the order of the atomics.

Shapes.  The four small geometries differ in Wp (10 / 33 / 9 / 34), mask period (40 / 264 / 56 / 136), dilation and Cout
tiling.  On a chip with hundreds of free workgroup slots the planner cuts such problems into one chunk per workgroup, so two
properties need more work than the slots hold: BIG (4 tiles x 187 chunks > 512 slots) is cut into 94 splits of TWO chunks
-- 187 is odd, the last split stages a zero chunk, the last slab group is ragged (94 = 23 * 4 + 2) -- and the 2-chunk
problems beside it become ONE split each (atomics only, no slab).  The tests ask mr_tn_taps_plan for that plan before they
rely on it.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr  # noqa: E402
from megreader_amd.nn import functional as F  # noqa: E402
from megreader_amd.nn import grads as G  # noqa: E402

DEV = "cuda"
BF = dtype_code(torch.bfloat16)

# (N, H, W, Cin, Cout, dil)
A = (3, 4, 9, 64, 64, 1)
B = (2, 8, 32, 128, 72, 1)       # Cout not a multiple of 64
C = (2, 6, 7, 64, 128, 2)        # dilation 2
D = (5, 4, 33, 64, 64, 1)
BIG = (88, 4, 33, 128, 128, 1)   # 187 chunks x 4 tiles: more workgroups than slots at one chunk each


@pytest.fixture(autouse=True)
def _taps_on():
    old = F.set_tn_taps(1)
    oldp = _lib.set_tuning(tn_taps_min_p=0)      # the small shapes must reach the all-taps kernel (default: P >= 10000 only)
    F.ensure_tn_taps_workspace(DEV)
    lib = _lib.load()
    assert lib.mr_tn_pending() == 0
    try:
        yield
    finally:
        lib.mr_tn_defer(0)
        lib.mr_tn_discard()
        F.set_tn_taps(old)
        _lib.set_tuning(**oldp)


@functools.lru_cache(maxsize=None)
def _host_problem(shape, seed, ldx, lddy):
    """Operands and float64 gradients of one problem (computed once per process, never modified)."""
    N, H, W, Cin, Cout, dil = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, H, W, ldx), generator=g).float()
    dy = torch.randint(-3, 4, (N, H, W, lddy), generator=g).float()
    wref = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    dyr = dy[..., :Cout].permute(0, 3, 1, 2).double()
    TF.conv2d(x[..., :Cin].permute(0, 3, 1, 2).double(), wref, None, 1, dil, dil).backward(dyr)
    return x, dy, wref.grad.permute(0, 2, 3, 1).contiguous(), dyr.sum((0, 2, 3))


def _problem(shape, seed=0, ldx=None, lddy=None, bias=True, fill=0):
    N, H, W, Cin, Cout, dil = shape
    ldx, lddy = ldx or Cin, lddy or (Cout + 7) // 8 * 8
    x, dy, ref, b_ref = _host_problem(shape, seed, ldx, lddy)
    assert _lib.load().mr_tn_taps_would_run(N, H, W, Cin, ldx, Cout, lddy, 3, 3, 1, 1, dil, dil, dil, dil, H, W) == 1
    return {"x": x.to(DEV).bfloat16(), "dy": dy.to(DEV).bfloat16(), "gw": torch.full((Cout, 3, 3, Cin), float(fill), device=DEV),
            "gb": torch.full((Cout,), float(fill), device=DEV) if bias else None, "fill": fill,
            "tab": torch.empty(N * H * W, 2, dtype=torch.int32, device=DEV),
            "geom": (N, H, W, Cin, ldx, Cout, lddy, 3, 3, 1, 1, dil, dil, dil, dil, H, W), "ref": ref, "b_ref": b_ref}


def _launch(pr, build=1):
    call("mr_conv2d_wgrad_tab", BF, ptr(pr["dy"]), ptr(pr["x"]), ptr(pr["gw"]), ptr(pr["gb"]), *pr["geom"], ptr(pr["tab"]), build)


def _record(probs, build=1):
    """Every problem inside a recording bracket; each call must have been RECORDED (a silent immediate launch fails here)."""
    lib = _lib.load()
    for pr in probs:
        before = lib.mr_tn_pending()
        old = lib.mr_tn_defer(1)
        _launch(pr, build)
        lib.mr_tn_defer(old)
        assert lib.mr_tn_pending() == before + 1


def _check(pr, times=1):
    got = pr["gw"].cpu().double()
    want = pr["fill"] + times * pr["ref"]
    assert torch.equal(got, want), "dW: max |err| %g" % float((got - want).abs().max())
    if pr["gb"] is not None:
        assert torch.equal(pr["gb"].cpu().double(), pr["fill"] + times * pr["b_ref"])


def _untouched(pr):
    assert float((pr["gw"] - pr["fill"]).abs().max()) == 0
    assert pr["gb"] is None or float((pr["gb"] - pr["fill"]).abs().max()) == 0


def _flush(name="mr_tn_flush"):
    call(name)
    assert _lib.load().mr_tn_pending() == 0
    torch.cuda.synchronize()


def _chunks(shape):
    N, H, W, _, _, dil = shape
    ip = (H * (W + dil) + 7) // 8 * 8
    return (N * ip + 63) // 64


def _tiles(shape):
    return (shape[4] + 63) // 64 * (shape[3] // 64)


def _plan(shapes):
    """The plan mr_tn_flush makes for these problems on this device with the registered workspace."""
    lib = _lib.load()
    n = len(shapes)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slabs = (F.ensure_tn_taps_workspace(DEV).numel() - 16384) // 147456
    arr = ctypes.c_int * n
    tiles, chunks = arr(*[_tiles(s) for s in shapes]), arr(*[_chunks(s) for s in shapes])
    launch, splits, cps, cost = arr(), arr(), arr(), ctypes.c_double()
    assert lib.mr_tn_taps_plan(cus, slabs, n, tiles, chunks, launch, splits, cps, ctypes.byref(cost)) >= 1
    return list(launch), list(splits), list(cps), list(chunks)


@pytest.mark.parametrize("count", [2, 3, 4])
def test_different_geometries_in_one_flush_equal_float64(count):
    """Two, three and four geometries side by side (different Wp, mask period, dilation, Cout tiling), padded row strides,
    one problem without dbias, dw pre-filled (the kernels accumulate); then the whole flush once more on the same workspace:
    the tickets must have been returned to zero."""
    probs = [_problem(D, seed=1, fill=3), _problem(B, seed=2, ldx=136, lddy=80), _problem(C, seed=3, bias=False, fill=-2),
             _problem(A, seed=4)][:count]
    launch = _plan([D, B, C, A][:count])[0]
    assert len(set(launch)) == 1                      # tiny problems: one launch, or the test shows nothing
    _record(probs)
    torch.cuda.synchronize()
    for pr in probs:
        _untouched(pr)                                # recorded, nothing launched
    _flush()
    for pr in probs:
        _check(pr)
    _record(probs, build=0)                           # same tables, same workspace
    _flush()
    for pr in probs:
        _check(pr, times=2)


def test_one_split_problems_beside_a_many_split_one_with_a_ragged_tail():
    shapes = [BIG, A, C]
    launch, splits, cps, chunks = _plan(shapes)
    assert len(set(launch)) == 1
    assert splits[0] >= 8 and chunks[0] % cps[0] != 0        # slab groups; the last split stages a zero chunk
    assert splits[1] == 1 and splits[2] == 1                 # atomics only, beside the slab groups
    probs = [_problem(BIG, seed=5), _problem(A, seed=6, fill=1), _problem(C, seed=7)]
    _record(probs)
    _flush()
    for pr in probs:
        _check(pr)
    _record(probs, build=0)
    _flush()
    for pr in probs:
        _check(pr, times=2)


def test_same_geometry_twice_with_different_operands():
    """Distinct slabs and tickets for two problems of one geometry (and one shared stream table)."""
    p0, p1 = _problem(D, seed=8), _problem(D, seed=9)
    p1["tab"] = p0["tab"]
    assert len(set(_plan([D, D])[0])) == 1
    _record([p0])
    _record([p1], build=0)
    _flush()
    _check(p0)
    _check(p1)


def test_more_records_than_one_launch_and_one_flush_group_hold():
    """14 records: the flush plans 12 + 2, and a launch holds at most 8 problems."""
    shapes = [A, D, C, B] * 3 + [A, D]
    probs = [_problem(s, seed=20 + i) for i, s in enumerate(shapes)]
    _record(probs)
    assert _lib.load().mr_tn_pending() == 14
    _flush()
    for pr in probs:
        _check(pr)


def test_mixed_with_dense_and_row_table_records():
    lib = _lib.load()
    g = torch.Generator().manual_seed(31)
    Ad = torch.randint(-3, 4, (200, 64), generator=g).float()
    Bd = torch.randint(-3, 4, (200, 64), generator=g).float()
    Cd = torch.zeros(64, 64, device=DEV)
    Adev, Bdev = Ad.to(DEV).bfloat16(), Bd.to(DEV).bfloat16()
    # a 3x3 layer the all-taps kernel does not serve (W = 64: tap shifts beyond one chunk): row-table GEMM kernel
    N, H, W, Cin, Cout = 2, 16, 64, 64, 128
    assert lib.mr_tn_taps_would_run(N, H, W, Cin, Cin, Cout, Cout, 3, 3, 1, 1, 1, 1, 1, 1, H, W) == 0
    xr = torch.randint(-3, 4, (N, H, W, Cin), generator=g).float()
    dyr = torch.randint(-3, 4, (N, H, W, Cout), generator=g).float()
    wref = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    TF.conv2d(xr.permute(0, 3, 1, 2).double(), wref, None, 1, 1, 1).backward(dyr.permute(0, 3, 1, 2).double())
    row = {"x": xr.to(DEV).bfloat16(), "dy": dyr.to(DEV).bfloat16(), "gw": torch.zeros(Cout, 3, 3, Cin, device=DEV), "gb": None,
           "tab": torch.empty(N * H * W, 2, dtype=torch.int32, device=DEV),
           "geom": (N, H, W, Cin, Cin, Cout, Cout, 3, 3, 1, 1, 1, 1, 1, 1, H, W)}
    taps = [_problem(A, seed=32), _problem(B, seed=33)]
    lib.mr_tn_defer(1)
    _launch(taps[0])
    call("mr_gemm_tn", BF, ptr(Adev), 64, ptr(Bdev), 64, ptr(Cd), 64, 200, 64, 64, 0, 0)
    _launch(row)
    _launch(taps[1])
    lib.mr_tn_defer(0)
    assert lib.mr_tn_pending() == 4
    _flush()
    for pr in taps:
        _check(pr)
    assert torch.equal(Cd.cpu().double(), Ad.double().t() @ Bd.double())
    assert torch.equal(row["gw"].cpu().double(), wref.grad.permute(0, 2, 3, 1))


def test_discard_leaves_the_gradients_untouched():
    lib = _lib.load()
    probs = [_problem(A, seed=40, fill=5), _problem(D, seed=41, fill=5)]
    _record(probs)
    assert lib.mr_tn_discard() == 2
    assert lib.mr_tn_pending() == 0
    call("mr_tn_flush")
    torch.cuda.synchronize()
    for pr in probs:
        _untouched(pr)


def test_flush_beside_on_a_second_stream():
    """mr_tn_flush_beside: the grouped launch leaves the shared workspace alone (plain atomics)."""
    probs = [_problem(D, seed=50), _problem(B, seed=51), _problem(C, seed=52)]
    _record(probs)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(main)                            # after the producers of the operands and the stream tables
    with torch.cuda.stream(side):
        call("mr_tn_flush_beside")
    assert _lib.load().mr_tn_pending() == 0
    main.wait_stream(side)
    torch.cuda.synchronize()
    for pr in probs:
        _check(pr)


def test_two_stacked_convs_through_autograd_equal_immediate_launches(monkeypatch):
    """Conv2dFn.backward records both layers' weight gradients; parameter gradients equal those of immediate launches
    (mr_tuning.tn_defer = 0) exactly.  Integers throughout: x, the weights and the loss weights are small integers, the
    activations and data gradients are bf16-rounded integers identical in both runs, and every weight-gradient partial sum
    is an integer below 2^24 (108 pixels x |dy| <= 1152 x |x| <= 576), so no order of additions changes a bit."""
    from megreader_amd.nn.modules import Conv2d
    from megreader_amd.optim import FusedAdam
    mr.set_compute_dtype(torch.bfloat16)
    assert _lib.load().mr_tn_taps_would_run(3, 4, 9, 64, 64, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1, 4, 9) == 1
    recorded = []
    end = G._TnDefer.end
    monkeypatch.setattr(G._TnDefer, "end", staticmethod(lambda tensors, params: recorded.append(end(tensors, params)) or recorded[-1]))
    g = torch.Generator().manual_seed(60)
    x = torch.randint(-1, 2, (3, 64, 4, 9), generator=g).float().to(DEV)
    weights = [torch.randint(-1, 2, (64, 64, 3, 3), generator=g).float() for _ in range(2)]
    biases = [torch.randint(-1, 2, (64,), generator=g).float() for _ in range(2)]
    wt = torch.randint(-2, 3, (3, 64, 4, 9), generator=g).float().to(DEV)
    grads = {}
    for mode in (0, 1):
        old_t = _lib.set_tuning(tn_defer=mode)
        F._ROWTABS.clear()
        del recorded[:]
        try:
            net = torch.nn.Sequential(Conv2d(64, 64, 3, padding=1), Conv2d(64, 64, 3, padding=1)).to(DEV)
            with torch.no_grad():
                for layer, w, b in zip(net, weights, biases):
                    layer.weight.copy_(w)
                    layer.bias.copy_(b)
            opt = FusedAdam(net.parameters(), lr=0.0)
            opt.zero_grad()
            y = net(x)
            (y.float() * wt).sum().backward()
            torch.cuda.synchronize()
            assert _lib.load().mr_tn_pending() == 0
            assert recorded == ([True, True] if mode else [False, False])
            grads[mode] = {k: p.grad.detach().float().cpu().clone() for k, p in net.named_parameters()}
        finally:
            _lib.set_tuning(**old_t)
            F._ROWTABS.clear()
    for k in grads[0]:
        assert float(grads[0][k].abs().max()) > 0
        assert torch.equal(grads[0][k], grads[1][k]), k
