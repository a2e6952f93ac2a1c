"""The store epilogues of the direct-to-LDS NT kernels (csrc/igemm_core.h: nt_epilogue_interior / nt_store_interior, the pooled epilogue of
igemm_nt_big_kernel) on EXACT operands: A in [-3, 3], B in [-2, 2], bias and addend multiples of 0.25, K <= 192, so every partial
sum is exact in f32 whatever the order and the stored value must EQUAL round_to_dtype(relu(A B^T + bias [+ addend])) computed in
float64.  Every problem is one tile + 8 rows high, so each launch runs the straight-line interior path (the waves of the full
tile) and the general edge path (the 8-row tile, the ragged column tile) side by side; C has a padded leading dimension and spare
rows filled with a sentinel that must survive."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr  # noqa: E402

DEV = "cuda"
SENTINEL = 2048.0    # exact in bf16 and beyond every possible result (|A B^T + bias + addend| <= 6 * 192 + 16)

# kernel -> (tuning that forces it, tile rows, tile columns)
KERNELS = {"big256": (dict(nt_big=1), 256, 256), "big272": (dict(nt_big=3), 272, 256),
           "tile128": (dict(nt_force_bm=128, nt_force_bn=128), 128, 128), "tile64": (dict(nt_force_bm=64, nt_force_bn=64), 64, 64),
           # the phased 256x256 kernel (igemm_p8.h) and the 8-wave kernels that serve 128x128 / 128x64 / 96x128 tiles by default
           # (mr_tuning.nt_wide8), which a forced 4-wave tile bypasses
           "p8": (dict(nt_big=1, nt_p8=1), 256, 256), "w8_128x128": (dict(nt_big=8), 128, 128),
           "w8_128x64": (dict(nt_big=10), 128, 64), "w8_96x128": (dict(nt_big=13), 96, 128)}
GEMM_CASES = [(k, torch.bfloat16) for k in KERNELS] + [("tile128", torch.float32), ("tile64", torch.float32)]
# columns: a full tile; tile + 24 (a second, partly filled column tile, whole 16-byte vectors); N % 8 != 0 with an odd leading
# dimension (element-wise stores)
N_KINDS = ("full", "plus24", "ragged")


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _quarters(shape, g):
    return torch.randint(-32, 33, shape, generator=g).float() * 0.25     # multiples of 0.25 in [-8, 8]


@pytest.mark.parametrize("nkind", N_KINDS)
@pytest.mark.parametrize("kernel,dtype", GEMM_CASES, ids=["%s_%s" % (k, "bf16" if d == torch.bfloat16 else "f32") for k, d in GEMM_CASES])
def test_gemm_nt_epilogue_is_exact(kernel, dtype, nkind):
    tuning, BM, BN = KERNELS[kernel]
    M = BM + 8
    N, ldc = {"full": (BN, BN + 8), "plus24": (BN + 24, BN + 32), "ragged": (BN + 13, BN + 16 + 3)}[nkind]
    g = torch.Generator().manual_seed(BM + N)
    bias_buf = _quarters((N + 1,), g).to(DEV)            # bias_buf[1:] starts one float past a 16-byte boundary
    assert bias_buf.data_ptr() % 16 == 0
    old = _lib.set_tuning(nt_big_min_k=32, **tuning)
    try:
        for K in (64, 96, 192):
            A = _ints((M, K), -3, 3, g).to(DEV, dtype)
            B = _ints((N, K), -2, 2, g).to(DEV, dtype)
            prod = A.double() @ B.double().t()
            for bias in (None, bias_buf[:N], bias_buf[1:]):
                for relu in (0, 1):
                    C = torch.full((M + 3, ldc), SENTINEL, device=DEV, dtype=dtype)
                    call("mr_gemm_nt", dtype_code(dtype), ptr(A), K, ptr(B), K, ptr(C), ldc, ptr(bias), relu, M, N, K)
                    ref = prod if bias is None else prod + bias.double()
                    if relu:
                        ref = torch.relu(ref)
                    ref = ref.float().to(dtype)          # exact in f32, then the one rounding of the store
                    what = (kernel, nkind, K, "bias %s" % ("none" if bias is None else bias.data_ptr() % 16), relu)
                    bad = C[:M, :N] != ref
                    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())
                    assert bool((C[:M, N:] == SENTINEL).all()), (what, "pad columns written")
                    assert bool((C[M:] == SENTINEL).all()), (what, "rows past M written")
    finally:
        _lib.set_tuning(**old)


@pytest.mark.parametrize("kernel", ["big256", "big272", "tile128"])
def test_conv_fwd_stats_epilogue_sums_the_stored_values(kernel):
    """mr_conv2d_fwd_stats with the offset bias: y exact, and the f64 sums those of the stored (bf16-rounded) values."""
    tuning, BM, BN = KERNELS[kernel]
    dtype, dt = torch.bfloat16, dtype_code(torch.bfloat16)
    Nb, H, W, C, Kc = 1, (BM + 8) // 8, 8, 64, BN          # 1x1 convolution: M = BM + 8 rows, K = 64
    g = torch.Generator().manual_seed(BM)
    x = _ints((Nb, H, W, C), -3, 3, g).to(DEV, dtype)
    w = _ints((Kc, 1, 1, C), -2, 2, g).to(DEV, dtype)
    bias = (_quarters((Kc + 1,), g) + 0.125).to(DEV)[1:]    # eighths: sums of up to 3 digits + .125 round in bf16
    old = _lib.set_tuning(nt_big_min_k=32, **tuning)
    try:
        y = torch.full((Nb, H, W, Kc), SENTINEL, device=DEV, dtype=dtype)
        sums = torch.zeros(_lib.load().mr_bn_scratch_doubles(Kc), dtype=torch.float64, device=DEV)
        call("mr_conv2d_fwd_stats", dt, ptr(x), ptr(w), ptr(bias), ptr(y), ptr(sums), Nb, H, W, C, C, Kc, 1, 1, 1, 1, 0, 0, 1, 1, H, W)
    finally:
        _lib.set_tuning(**old)
    ref = (x.double().view(-1, C) @ w.double().view(Kc, C).t() + bias.double()).float().to(dtype)
    assert torch.equal(y.view(-1, Kc), ref)
    got = sums[:16 * Kc].view(8, 2, Kc).sum(dim=0)
    yd = y.double().view(-1, Kc)
    want = torch.stack([yd.sum(dim=0), (yd * yd).sum(dim=0)])
    # f32 partial sums over <= 17 row blocks of 16 lanes, f64 from there on: <= 272 terms * 2^-24 relative to the sum of magnitudes
    scale = torch.stack([yd.abs().sum(dim=0), (yd * yd).sum(dim=0)]) + 1e-30
    err = float(((got - want).abs() / scale).max())
    print("%s: stats relative error %.3g" % (kernel, err))
    assert err < 272 * 2.0 ** -24


@pytest.mark.parametrize("kernel", ["big256", "big272", "p8", "w8_128x128", "w8_96x128", "tile128", "tile64"])
def test_conv_dgrad_add_epilogue_is_exact(kernel):
    tuning, BM, BN = KERNELS[kernel]
    dtype, dt = torch.bfloat16, dtype_code(torch.bfloat16)
    N, H, W, Cin, Cout = 1, (BM + 8) // 8, 8, BN, 64       # 1x1 dgrad: M = BM + 8 rows of Cin = BN columns, K = Cout = 64
    g = torch.Generator().manual_seed(BM + 1)
    dy = _ints((N, H, W, Cout), -3, 3, g).to(DEV, dtype)
    w_crsk = _ints((Cin, 1, 1, Cout), -2, 2, g).to(DEV, dtype)
    add = _quarters((N, H, W, Cin), g).to(DEV, dtype)
    args = (N, H, W, Cin, Cin, Cout, Cout, 1, 1, 1, 1, 0, 0, 1, 1, H, W)
    ref = (dy.double().view(-1, Cout) @ w_crsk.double().view(Cin, Cout).t() + add.double().view(-1, Cin)).float().to(dtype)
    old = _lib.set_tuning(nt_big_min_k=32, **tuning)
    try:
        dx = torch.full((N, H, W, Cin), SENTINEL, device=DEV, dtype=dtype)
        call("mr_conv2d_dgrad_add", dt, ptr(dy), ptr(w_crsk), ptr(dx), ptr(add), *args)
        alias = add.clone()                                 # the addend may alias dx
        call("mr_conv2d_dgrad_add", dt, ptr(dy), ptr(w_crsk), ptr(alias), ptr(alias), *args)
    finally:
        _lib.set_tuning(**old)
    assert torch.equal(dx.view(-1, Cin), ref)
    assert torch.equal(alias, dx)


@pytest.mark.parametrize("with_y,with_add", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("kernel", ["tile128", "tile64"])
def test_conv_dgrad_bnb_epilogue_is_exact(kernel, with_y, with_add):
    """mr_conv2d_dgrad_bnb on exact operands: dx = round(dgrad [+ addend]); sums = sum g', sum g' xhat over g' = the STORED dx
    where y > 0, xhat = (x - mean) rstd with mean = 0.5, rstd = 2.  Every product and partial sum is a small multiple of 1/8, exact
    in f32 and f64, so the sums must EQUAL the float64 ones."""
    tuning, BM, BN = KERNELS[kernel]
    dtype, dt = torch.bfloat16, dtype_code(torch.bfloat16)
    N, H, W, Cin, Cout = 1, (BM + 8) // 8, 8, BN, 64
    g = torch.Generator().manual_seed(BM + 2 * with_y + with_add)
    dy = _ints((N, H, W, Cout), -3, 3, g).to(DEV, dtype)
    w_crsk = _ints((Cin, 1, 1, Cout), -2, 2, g).to(DEV, dtype)
    add = _quarters((N, H, W, Cin), g).to(DEV, dtype) if with_add else None
    x = _ints((N, H, W, Cin), -3, 3, g).to(DEV, dtype)
    y = _ints((N, H, W, Cin), -1, 2, g).to(DEV, dtype) if with_y else None       # <= 0 on half the elements
    mean = torch.full((Cin,), 0.5, device=DEV)
    rstd = torch.full((Cin,), 2.0, device=DEV)
    args = (N, H, W, Cin, Cin, Cout, Cout, 1, 1, 1, 1, 0, 0, 1, 1, H, W)
    old = _lib.set_tuning(nt_big=-1, **tuning)
    try:
        dx = torch.full((N, H, W, Cin), SENTINEL, device=DEV, dtype=dtype)
        sums = torch.zeros(_lib.load().mr_bn_scratch_doubles(Cin), dtype=torch.float64, device=DEV)
        produced = ctypes.c_int(0)
        call("mr_conv2d_dgrad_bnb", dt, ptr(dy), ptr(w_crsk), ptr(dx), ptr(add), ptr(x), ptr(y), ptr(mean), ptr(rstd), ptr(sums),
             ctypes.byref(produced), *args)
    finally:
        _lib.set_tuning(**old)
    ref = dy.double().view(-1, Cout) @ w_crsk.double().view(Cin, Cout).t()
    if with_add:
        ref = ref + add.double().view(-1, Cin)
    ref = ref.float().to(dtype)
    assert torch.equal(dx.view(-1, Cin), ref)
    assert produced.value == 1
    gp = ref.double()
    if with_y:
        gp = gp * (y.double().view(-1, Cin) > 0)
    want = torch.stack([gp.sum(dim=0), (gp * (x.double().view(-1, Cin) - 0.5) * 2.0).sum(dim=0)])
    got = sums[:16 * Cin].view(8, 2, Cin).sum(dim=0)
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("H,W,Cin,Cout,big", [(8, 32, 256, 256, 1), (4, 33, 512, 512, 3)], ids=["8x32_big256", "4x33_big272"])
def test_pooled_forward_with_offset_bias_equals_the_unfused_path(H, W, Cin, Cout, big):
    """conv + bias + ReLU + max-pool in one launch at 2 images, bias one float past a 16-byte boundary: pooled values and arg-max
    codes bit for bit those of mr_conv2d_fwd + mr_maxpool_fwd (as tests/test_conv_pool_gpu.py), on integer-valued operands."""
    N, dt = 2, dtype_code(torch.bfloat16)
    g = torch.Generator().manual_seed(H * W)
    x = _ints((N, H, W, Cin), -3, 3, g).to(DEV, torch.bfloat16)
    w = _ints((Cout, 3, 3, Cin), -2, 2, g).to(DEV, torch.bfloat16)
    bias = _quarters((Cout + 1,), g).to(DEV)[1:]
    pk, ps, pp = (2, 2), (2, 1), (0, 1)
    PH, PW = (H - pk[0]) // ps[0] + 1, (W + 2 * pp[1] - pk[1]) // ps[1] + 1
    conv, tail = (N, H, W, Cin, Cin, Cout), (3, 3, 1, 1, 1, 1, 1, 1, H, W)
    pool = (pk[0], pk[1], ps[0], ps[1], pp[0], pp[1])
    old = _lib.set_tuning(nt_big=big)
    try:
        assert _lib.load().mr_conv2d_fwd_pool_ok(dt, *conv, *tail, *pool)
        yf = torch.full((N, PH, PW, Cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        cf = torch.full((N, PH, PW, Cout), 255, dtype=torch.uint8, device=DEV)
        call("mr_conv2d_fwd_pool", dt, ptr(x), ptr(w), ptr(bias), ptr(yf), ptr(cf), 1, *conv, *tail, *pool, PH, PW)
        z = torch.empty((N, H, W, Cout), dtype=torch.bfloat16, device=DEV)
        call("mr_conv2d_fwd", dt, ptr(x), ptr(w), ptr(bias), ptr(z), 1, *conv, Cout, *tail)
    finally:
        _lib.set_tuning(**old)
    yu, cu = torch.empty_like(yf), torch.empty_like(cf)
    call("mr_maxpool_fwd", dt, ptr(z), ptr(yu), ptr(cu), N, H, W, Cout, *pool, PH, PW)
    torch.cuda.synchronize()
    assert torch.equal(yf.view(torch.int16), yu.view(torch.int16))
    assert torch.equal(cf, cu)
    # ... and the unfused activation itself against float64
    zr = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), bias.double(), 1, 1)
    assert torch.equal(z, torch.relu(zr).permute(0, 2, 3, 1).float().to(torch.bfloat16))
