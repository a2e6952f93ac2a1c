"""The small HBM-bound kernels of csrc/elementwise.hip through the C ABI -- mr_cast, mr_add, mr_relu_bwd, mr_permute_021,
mr_nchw_to_nhwc, mr_nhwc_to_nchw, mr_colsum, mr_zero_multi -- each against the obvious torch expression on the CPU.

Every one of them is a copy, a select or one rounding of an exact float32 result, so equality is exact.  The sizes hit what model
tensors (always padded) never do: the one-thread scalar tail behind the 16-byte vectors, and a grid at its cap with a second trip
of the grid-stride loop.  Destinations are followed by a guard band of sentinels."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd._lib import call, dtype_code, ptr, vec_of  # noqa: E402
from megreader_amd.nn.functional import zero_segments  # noqa: E402

from _abi_util import SENTINEL, guard_intact, guarded, mixed_values  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
GRID_CAP = 8192 * 256      # threads of a capped grid (grid_for: at most 8192 blocks of 256)


def _check(whole, n, expect, what=""):
    assert torch.equal(whole[:n].cpu(), expect.reshape(-1)), what
    assert guard_intact(whole, n), what


# ------------------------------------------------------------------ mr_cast
@pytest.mark.parametrize("n", [1, 255, 257, GRID_CAP + 3])
@pytest.mark.parametrize("dst_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("src_dtype", DTYPES, ids=IDS)
def test_cast(src_dtype, dst_dtype, n):
    src = mixed_values((n,), n).to(src_dtype)          # f32 sources carry exact bf16 round-to-even ties
    whole, dst = guarded(n, dst_dtype)
    src_d = src.to(DEV)
    call("mr_cast", dtype_code(src_dtype), ptr(src_d), dtype_code(dst_dtype), ptr(dst), n)
    _check(whole, n, src.to(dst_dtype))


@pytest.mark.parametrize("codes", [(0, 2), (2, 0), (-1, 1), (1, 7)])
def test_cast_refuses_unknown_dtype_codes(codes):
    src = torch.ones(8, device=DEV)
    whole, dst = guarded(8, torch.float32)
    with pytest.raises(RuntimeError, match=r"mr_cast failed \(code 2\).*bad dtypes"):
        call("mr_cast", codes[0], ptr(src), codes[1], ptr(dst), 8)
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


# ------------------------------------------------------------------ mr_add / mr_relu_bwd
def _sizes(dtype):
    v = vec_of(dtype)
    return [1, 3, 7, 8, 9, 4099, GRID_CAP * v + v + 1]


def _tiny(dtype):
    """Smallest positive subnormal and smallest positive normal of the storage type."""
    if dtype == torch.float32:
        return [torch.tensor(1, dtype=torch.int32).view(torch.float32).item(), torch.finfo(torch.float32).tiny]
    return [torch.tensor(1, dtype=torch.int16).view(torch.bfloat16).float().item(), torch.finfo(torch.bfloat16).tiny]


def _with_signs_and_zeros(n, dtype, seed):
    """Values of `dtype` (as float32 on the CPU): negatives, positives and, cycling through the positions so that the vector
    body and the scalar tail both see them, +0.0, -0.0, the smallest positive values and their negatives."""
    x = mixed_values((n,), seed).to(dtype).float()
    t = _tiny(dtype)
    special = torch.tensor([0.0, -0.0, t[0], t[1], -t[0], -t[1]])
    idx = torch.arange(n)
    pick = (idx % 5 == 0) | (idx >= n - 4)
    x[pick] = special[(torch.arange(int(pick.sum())) + n) % 6]
    return x


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("si", range(7))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add(dtype, si, relu):
    n = _sizes(dtype)[si]
    a = _with_signs_and_zeros(n, dtype, 2 * n)
    b = _with_signs_and_zeros(n, dtype, 2 * n + 1).roll(1)
    whole, out = guarded(n, dtype)
    a_d, b_d = a.to(DEV, dtype), b.to(DEV, dtype)
    call("mr_add", dtype_code(dtype), ptr(a_d), ptr(b_d), ptr(out), n, relu)
    s = a + b                                   # float32 add of values of `dtype`, then ONE rounding to `dtype`
    if relu:
        s = torch.relu(s)
    _check(whole, n, s.to(dtype))


@pytest.mark.parametrize("si", range(7))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_relu_bwd(dtype, si):
    n = _sizes(dtype)[si]
    y = _with_signs_and_zeros(n, dtype, 3 * n)
    dy = mixed_values((n,), 3 * n + 1).to(dtype)
    whole, dx = guarded(n, dtype)
    dy_d, y_d = dy.to(DEV), y.to(DEV, dtype)
    call("mr_relu_bwd", dtype_code(dtype), ptr(dy_d), ptr(y_d), ptr(dx), n)
    expect = torch.where(y > 0, dy.float(), torch.zeros(())).to(dtype)
    assert int((y == 0).sum()) > 0 or n < 5
    _check(whole, n, expect)


@pytest.mark.parametrize("name", ["mr_add", "mr_relu_bwd"])
def test_add_and_relu_bwd_refuse_misaligned_pointers(name):
    a, b = torch.ones(16, device=DEV), torch.ones(16, device=DEV)
    whole, out = guarded(16, torch.float32)
    tail = (8, 0) if name == "mr_add" else (8,)
    with pytest.raises(RuntimeError, match=r"%s failed \(code 1\).*16-byte aligned" % name):
        call(name, 0, ptr(a) + 4, ptr(b), ptr(out), *tail)
    with pytest.raises(RuntimeError, match=r"%s failed \(code 1\).*16-byte aligned" % name):
        call(name, 0, ptr(a), ptr(b), ptr(out) + 8, *tail)
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


# ------------------------------------------------------------------ mr_permute_021
@pytest.mark.parametrize("A,B,C", [(3, 5, 8), (1, 7, 16), (26, 33, 512)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_permute_021(dtype, A, B, C):
    src = mixed_values((A, B, C), A + B).to(dtype)
    whole, dst = guarded(A * B * C, dtype)
    src_d = src.to(DEV)
    call("mr_permute_021", dtype_code(dtype), ptr(src_d), ptr(dst), A, B, C)
    _check(whole, A * B * C, src.permute(1, 0, 2).contiguous())


@pytest.mark.parametrize("dtype,C", [(torch.float32, 6), (torch.float32, 1), (torch.bfloat16, 12), (torch.bfloat16, 4)])
def test_permute_021_refuses_partial_vectors(dtype, C):
    src = torch.ones(2 * 3 * C, dtype=dtype, device=DEV)
    whole, dst = guarded(2 * 3 * C, dtype)
    with pytest.raises(RuntimeError, match=r"mr_permute_021 failed \(code 1\).*must be a multiple of %d" % vec_of(dtype)):
        call("mr_permute_021", dtype_code(dtype), ptr(src), ptr(dst), 2, 3, C)
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


# ------------------------------------------------------------------ mr_nchw_to_nhwc / mr_nhwc_to_nchw
def _pads(C, dtype):
    v = vec_of(dtype)
    return sorted({(C + v - 1) // v * v, 32})          # the channel count rounded up to whole vectors, and 32


@pytest.mark.parametrize("C", [1, 3, 27])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layout_conversions(dtype, C):
    N, H, W = 2, 3, 5
    x = mixed_values((N, C, H, W), C)
    x_d = x.to(DEV)
    for Cpad in _pads(C, dtype):
        n = N * H * W * Cpad
        whole, nhwc = guarded(n, dtype)
        call("mr_nchw_to_nhwc", dtype_code(dtype), ptr(x_d), ptr(nhwc), N, C, H, W, Cpad)
        expect = torch.zeros(N, H, W, Cpad)
        expect[..., :C] = x.permute(0, 2, 3, 1)
        _check(whole, n, expect.to(dtype), "to NHWC, Cpad %d" % Cpad)         # padded channels come out zero
        # back: the first C of ld channels; the padding is filled with junk first, none of it may come through
        whole[:n].view(N, H, W, Cpad)[..., C:] = 9.0
        back_whole, back = guarded(N * C * H * W, torch.float32)
        call("mr_nhwc_to_nchw", dtype_code(dtype), ptr(nhwc), ptr(back), N, C, H, W, Cpad)
        _check(back_whole, N * C * H * W, x.to(dtype).float(), "to NCHW, ld %d" % Cpad)   # float32: the round trip is exact


def test_nchw_to_nhwc_refuses_a_pad_below_the_channel_count():
    x = torch.ones(2 * 5 * 3 * 5, device=DEV)
    whole, dst = guarded(2 * 3 * 5 * 4, torch.float32)
    with pytest.raises(RuntimeError, match=r"mr_nchw_to_nhwc failed \(code 1\).*Cpad < C"):
        call("mr_nchw_to_nhwc", 0, ptr(x), ptr(dst), 2, 5, 3, 5, 4)
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


def test_layout_conversion_grid_stride():
    """More elements than a capped grid has threads: the second trip of both loops."""
    N, C, H, W, Cpad = 3, 24, 160, 200, 24
    n = N * H * W * Cpad
    assert n > GRID_CAP
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-120, 121, (N, C, H, W), generator=g).float()      # exact in bf16 too
    x_d = x.to(DEV)
    for dtype in DTYPES:
        whole, nhwc = guarded(n, dtype)
        call("mr_nchw_to_nhwc", dtype_code(dtype), ptr(x_d), ptr(nhwc), N, C, H, W, Cpad)
        _check(whole, n, x.permute(0, 2, 3, 1).contiguous().to(dtype))
        back_whole, back = guarded(n, torch.float32)
        call("mr_nhwc_to_nchw", dtype_code(dtype), ptr(nhwc), ptr(back), N, C, H, W, Cpad)
        _check(back_whole, n, x)


# ------------------------------------------------------------------ mr_colsum
@pytest.mark.parametrize("P,C,ld,perm_h", [(1, 1, 1, 0), (63, 70, 72, 0), (1000, 1024, 1024, 256), (5, 2048, 2048, 256),
                                           (70000, 8, 8, 0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_colsum(dtype, P, C, ld, perm_h):
    """Integer inputs in -8..8: every partial sum stays below 2^24, so any summation order gives the same float32.  The
    kernel reads gate-interleaved columns c = 4*j + q and adds into the gate-major slot q*H + j of each block of 4*H."""
    g = torch.Generator().manual_seed(P + C)
    x = torch.randint(-8, 9, (P, ld), generator=g).float()
    start = torch.randint(-50, 51, (C,), generator=g).float()
    whole, out = guarded(C, torch.float32)
    out.copy_(start)
    x_d = x.to(DEV, dtype)
    call("mr_colsum", dtype_code(dtype), ptr(x_d), ptr(out), P, C, ld, perm_h)
    s = x[:, :C].double().sum(0).float()
    if perm_h:
        r = torch.arange(C)
        h4 = 4 * perm_h
        blk, rin = r // h4, r % h4
        s = s[blk * h4 + 4 * (rin % perm_h) + rin // perm_h]          # slot r = q*H + j receives column 4*j + q
    _check(whole, C, start + s)                                       # accumulated into, not overwritten


def test_colsum_refuses_bad_shapes():
    x = torch.ones(64, device=DEV)
    whole, out = guarded(8, torch.float32)
    for P, C, perm_h in ((0, 8, 0), (8, 0, 0), (8, 8, 4), (4, 12, 2)):
        with pytest.raises(RuntimeError, match=r"mr_colsum failed \(code 1\)"):
            call("mr_colsum", 0, ptr(x), ptr(out), P, C, 8, perm_h)
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


# ------------------------------------------------------------------ mr_zero_multi
SEGMENT_BYTES = [16, 0, 8 * 1024 * 1024 + 16, 48, 4096, 1024 * 1024 + 32, 160, 272, 64]
FILL = 0xAB


def _segments(count):
    bufs = [torch.full((b + 256,), FILL, dtype=torch.uint8, device=DEV) for b in SEGMENT_BYTES[:count]]
    return bufs, [(t.data_ptr(), b) for t, b in zip(bufs, SEGMENT_BYTES)]


def _check_segments(bufs):
    for t, b in zip(bufs, SEGMENT_BYTES):
        assert bool((t[:b] == 0).all()) and bool((t[b:] == FILL).all()), b


def _zero_multi(segments):
    n = len(segments)
    call("mr_zero_multi", n, (ctypes.c_void_p * n)(*[p for p, _ in segments]), (ctypes.c_longlong * n)(*[b for _, b in segments]))


@pytest.mark.parametrize("count", range(1, 9))
def test_zero_multi(count):
    bufs, segments = _segments(count)
    _zero_multi(segments)
    _check_segments(bufs)


def test_zero_segments_splits_nine_segments_into_two_launches():
    bufs, segments = _segments(9)
    zero_segments(segments)
    _check_segments(bufs)
    with pytest.raises(RuntimeError, match=r"mr_zero_multi failed \(code 1\).*at most 8 segments"):
        _zero_multi(segments)


def test_zero_multi_refuses_misaligned_segments():
    bufs, segments = _segments(3)
    for bad in ((segments[0][0] + 4, 16), (segments[0][0], 24), (0, 16), (segments[0][0], -16)):
        with pytest.raises(RuntimeError, match=r"mr_zero_multi failed \(code 1\).*segment 1"):
            _zero_multi([segments[2], bad])
    torch.cuda.synchronize()
    for t in bufs:
        assert bool((t == FILL).all())                  # refused before anything is launched: the good segment is untouched too
