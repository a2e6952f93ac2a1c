"""Dense and row-table conv weight-gradient problems in ONE grouped launch (mr_tn_defer / mr_tn_flush; the grouped form of
igemm_tn_glds_kernel branches per workgroup on the problem's operand mode; csrc/gemm_conv.hip: tn_group_plan cuts every problem
into splits of its own).

Operands are small integers, so every product and partial sum is exact in bf16 / f32: a grouped launch must EQUAL float64
arithmetic bit for bit, whatever its split / atomic order -- and therefore equal the immediate launches (mr_tuning.tn_defer = 0)
exactly.  The reference of every problem is computed once, in float64 on the CPU, and shared by the comparisons.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr  # noqa: E402
from megreader_amd.nn import functional as F  # noqa: E402

DEV = "cuda"
BF = dtype_code(torch.bfloat16)


def _ints(shape, g, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=g).float()


class Dense(object):
    """C[NA, NB] += A[P, NA]^T B[P, NB]; two=True: mr_gemm_tn2 with both column-sum destinations"""

    def __init__(self, g, P, NA, NB, colsum=False, two=False):
        self.P, self.NA, self.NB, self.two = P, NA, NB, two
        self.lda = (NA + 7) // 8 * 8
        A = _ints((P, self.lda), g)
        A[:, NA:] = 0                          # padding columns of A feed output rows that are never stored
        B = _ints((P, NB), g)
        self.A, self.B = A.to(DEV).bfloat16(), B.to(DEV).bfloat16()
        self.ref = {"C": A[:, :NA].double().t() @ B.double()}
        if colsum or two:
            self.ref["cs"] = A[:, :NA].double().sum(0)
        if two:
            self.ref["cs2"] = self.ref["cs"]
        self.mode, self.tiles, self.steps = 0, -(-NA // 128) * -(-NB // 128), -(-P // 64)
        self.reset()

    def reset(self):
        self.out = {"C": torch.zeros(self.NA, self.NB, device=DEV)}
        for k in self.ref:
            if k != "C":
                self.out[k] = torch.zeros(self.NA, device=DEV)

    def launch(self):
        cs = self.out.get("cs")
        if self.two:
            call("mr_gemm_tn2", BF, ptr(self.A), self.lda, ptr(self.B), self.NB, ptr(self.out["C"]), self.NB, self.P, self.NA,
                 self.NB, 0, ptr(cs), ptr(self.out["cs2"]))
        else:
            call("mr_gemm_tn", BF, ptr(self.A), self.lda, ptr(self.B), self.NB, ptr(self.out["C"]), self.NB, self.P, self.NA,
                 self.NB, 0, ptr(cs))


class Conv(object):
    """weight and bias gradient of a convolution through a row table (mr_conv2d_wgrad_tab)"""

    def __init__(self, g, N, H, W, C, K, R, S, st, pad):
        Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
        lddy = (K + 7) // 8 * 8
        x = _ints((N, H, W, C), g)
        dy = _ints((N, Ho, Wo, lddy), g)
        dy[..., K:] = 0
        wref = torch.zeros(K, C, R, S, dtype=torch.float64, requires_grad=True)
        TF.conv2d(x.permute(0, 3, 1, 2).double(), wref, None, st, pad).backward(dy[..., :K].permute(0, 3, 1, 2).double())
        self.x, self.dy = x.to(DEV).bfloat16(), dy.to(DEV).bfloat16()
        self.tab = torch.empty(N * Ho * Wo, 2, dtype=torch.int32, device=DEV)
        self.built = False
        self.geom = (N, H, W, C, C, K, lddy, R, S, st, st, pad, pad, 1, 1, Ho, Wo)
        self.shape = (K, R, S, C)
        self.ref = {"C": wref.grad.permute(0, 2, 3, 1).contiguous(), "cs": dy[..., :K].double().sum((0, 1, 2))}
        self.mode, self.tiles, self.steps = 2, -(-K // 128) * -(-(C * R * S) // 128), -(-(N * Ho * Wo) // 64)
        self.reset()

    def reset(self):
        self.out = {"C": torch.zeros(self.shape, device=DEV), "cs": torch.zeros(self.shape[0], device=DEV)}

    def launch(self):
        call("mr_conv2d_wgrad_tab", BF, ptr(self.dy), ptr(self.x), ptr(self.out["C"]), ptr(self.out["cs"]), *self.geom,
             ptr(self.tab), 0 if self.built else 1)        # the row-table kernel runs at once, the GEMM is recorded
        self.built = True


def _check(probs, times=1):
    torch.cuda.synchronize()
    for i, pr in enumerate(probs):
        for k, ref in pr.ref.items():
            got = pr.out[k].cpu().double()
            assert torch.equal(got, times * ref), "problem %d %s: max |err| %g" % (i, k, float((got - times * ref).abs().max()))


def _plan(probs):
    """The plan mr_tn_flush makes for these problems on this device"""
    n = len(probs)
    arr = ctypes.c_int * n
    launch, splits, begin = arr(), arr(), arr()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    launches = _lib.load().mr_tn_group_plan(cus, n, arr(*[p.tiles for p in probs]), arr(*[p.steps for p in probs]),
                                           arr(*[p.mode for p in probs]), launch, splits, begin, None)
    assert launches >= 1
    return launches, list(launch), list(splits)


@pytest.fixture
def off_taps():
    """keep every conv shape off the all-taps kernel: this file is about the 128x128 TN kernel"""
    old = _lib.set_tuning(tn_taps_min_p=1 << 30)
    F._ROWTABS.clear()
    try:
        yield
    finally:
        _lib.load().mr_tn_discard()
        _lib.set_tuning(**old)
        F._ROWTABS.clear()


def _record(probs):
    lib = _lib.load()
    assert lib.mr_tn_pending() == 0
    old = lib.mr_tn_defer(1)
    for pr in probs:
        pr.launch()
    lib.mr_tn_defer(old)
    assert lib.mr_tn_pending() == len(probs) == lib.mr_tn_pending_of(0)          # recorded, nothing launched
    assert lib.mr_tn_pending_of(1) == 0


def _immediate_then_flushed(probs, flush="mr_tn_flush"):
    """immediate launches (mr_tuning.tn_defer = 0) and one flush of the same problems: each equals float64, hence each other"""
    lib = _lib.load()
    old_t = _lib.set_tuning(tn_defer=0)
    try:
        lib.mr_tn_defer(1)
        for pr in probs:
            pr.launch()
        lib.mr_tn_defer(0)
        assert lib.mr_tn_pending() == 0
    finally:
        _lib.set_tuning(**old_t)
    _check(probs)
    immediate = [{k: v.clone() for k, v in pr.out.items()} for pr in probs]
    for pr in probs:
        pr.reset()
    _record(probs)
    call(flush)
    assert lib.mr_tn_pending() == 0
    _check(probs)
    for pr, imm in zip(probs, immediate):
        for k in imm:
            assert torch.equal(pr.out[k], imm[k])


def _mixed(g):
    return [Dense(g, 200, 136, 72, colsum=True),        # tail of a 64-row step, partial tiles in both directions
            Dense(g, 40, 64, 16),                       # shorter than one step
            Dense(g, 264, 256, 128, two=True),          # mr_gemm_tn2: the column sums go to two destinations
            Conv(g, 2, 2, 6, 40, 24, 2, 2, 1, 0),       # shaped like conv6 of the CRNN: 2x2, no padding, a 2 x 6 map
            Conv(g, 3, 9, 9, 16, 24, 3, 3, 2, 1)]       # 3x3 stride 2 with padding: taps that fall outside


def test_dense_and_conv_problems_share_one_launch(off_taps):
    probs = _mixed(torch.Generator().manual_seed(31))
    assert _plan(probs)[0] == 1                         # one grouped launch holds both modes
    _immediate_then_flushed(probs)
    # a second flush accumulates (the kernels add into their outputs): exactly twice the gradient
    _record(probs)
    call("mr_tn_flush")
    _check(probs, times=2)


def test_several_splits_beside_a_single_split(off_taps):
    g = torch.Generator().manual_seed(32)
    probs = [Dense(g, 64 * 40 + 8, 128, 128, colsum=True), Dense(g, 64, 72, 8), Conv(g, 4, 24, 24, 16, 24, 3, 3, 1, 1)]
    launches, _, splits = _plan(probs)
    assert launches == 1 and splits[0] > 1 and splits[1] == 1 and splits[2] > 1
    _immediate_then_flushed(probs)


def test_more_problems_than_one_launch_holds(off_taps):
    cap = _lib.load().mr_tn_capacity(0)
    g = torch.Generator().manual_seed(33)
    probs = []
    while len(probs) < cap + 1:
        i = len(probs)
        probs.append(Conv(g, 2, 5 + i % 3, 7, 8 * (1 + i % 4), 24, 2, 2, 1, 0) if i % 3 == 2 else
                     Dense(g, 40 + 37 * i, 8 * (1 + i % 5), 16 * (1 + i % 3), colsum=bool(i & 1)))
    launches, launch, _ = _plan(probs)
    assert launches >= 2 and max(launch.count(l) for l in set(launch)) <= cap
    _immediate_then_flushed(probs)


def test_flush_beside_on_a_second_stream(off_taps):
    """mr_tn_flush_beside: atomics only, nothing touches the shared split-reduction workspace"""
    probs = _mixed(torch.Generator().manual_seed(34))
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    _record(probs)
    side.wait_stream(main)                              # after the producers of the operands and the row tables
    with torch.cuda.stream(side):
        call("mr_tn_flush_beside")
    assert _lib.load().mr_tn_pending() == 0
    main.wait_stream(side)
    _check(probs)
