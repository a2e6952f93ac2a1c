"""conv + bias + ReLU + max-pool as one forward launch (csrc/igemm_core.h: EpiPool, mr_conv2d_fwd_pool; round 6) against the two
launches it replaces (mr_conv2d_fwd + mr_maxpool_fwd) at the three pooled stages of the CRNN backbone (reference
backbones/crnn.py:14-33): pooled values and arg-max codes must be BIT-IDENTICAL (same bf16 rounding of the activation, same
first-maximum rule), hence so is everything the backward derives from them."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd.nn import functional as F  # noqa: E402

DEV = "cuda"
# (name, N, Cin, H, W, Cout, pool kernel, stride, padding): conv1 (128-row tiles = one window row), conv3 (256-row tile = one image),
# conv5 (264 of 272 rows = two images; odd N: the last tile holds one image), and the same at the benchmarked batch
CASES = [("conv1", 8, 64, 16, 64, 128, (2, 2), (2, 2), (0, 0)), ("conv3", 4, 256, 8, 32, 256, (2, 2), (2, 1), (0, 1)),
         ("conv5", 5, 512, 4, 33, 512, (2, 2), (2, 1), (0, 1)), ("conv5_n256", 256, 512, 4, 33, 512, (2, 2), (2, 1), (0, 1)),
         ("conv5_n255", 255, 512, 4, 33, 512, (2, 2), (2, 1), (0, 1)), ("conv3_n256", 256, 256, 8, 32, 256, (2, 2), (2, 1), (0, 1)),
         ("conv1_n256", 256, 64, 16, 64, 128, (2, 2), (2, 2), (0, 0))]


def _c3(n, w):
    return (n, 256, 8, w, 256, (2, 2), (2, 1), (0, 1))


def _c5(n, w):
    return (n, 512, 4, w, 512, (2, 2), (2, 1), (0, 1))


# The tile classes of the plan (csrc/gemm_conv.hip: conv_pool_plan) at widths other than 128, batch 255 / 256:
#   name -> (class, rows of the tile the forward takes, rows of it that hold data, whole images per tile or 0 = a fraction of one)
#   (a) one image per tile, idle rows     (b) two whole images per tile (N = 255: the last tile holds one)
#   (c) half an image per tile            (d) the 272-row kernel, full and nearly full
# The rows that hold data follow from the geometry alone (image = Ho*Wo rows, window row = kh*Wo rows; _tile_rows below restates
# it); that the library takes the named tile for the named batch is asserted, not assumed.  What is NOT asserted is the library's
# own cut (NtArgs.tile_rows): no entry point reports it, and _tile_rows restates conv_pool_plan's rule.  A plan that kept the kernel
# and the eligibility but cut the tiles elsewhere would still have to produce bit-identical results here, yet the class labels
# printed below would then describe the old cut: re-derive this table whenever conv_pool_plan's `fit` changes.
TILE_CLASSES = {
    "a_conv3_8x30": ("a", 256, 240, 1), "a_conv3_8x31": ("a", 256, 248, 1),
    "a_conv5_4x61": ("a", 256, 244, 1), "a_conv5_4x63": ("a", 256, 252, 1),
    "b_conv5_4x31_n256": ("b", 256, 248, 2), "b_conv5_4x31_n255": ("b", 256, 248, 2), "b_conv5_4x32_n255": ("b", 256, 256, 2),
    "c_conv3_8x60": ("c", 256, 240, 0), "c_conv3_8x64_n255": ("c", 256, 256, 0),
    "d_conv5_4x34": ("d", 272, 272, 2), "d_conv5_4x65_n255": ("d", 272, 260, 1), "d_conv3_8x33": ("d", 272, 264, 1),
}
CLASS_CASES = [("a_conv3_8x30",) + _c3(256, 30), ("a_conv3_8x31",) + _c3(256, 31),
               ("a_conv5_4x61",) + _c5(256, 61), ("a_conv5_4x63",) + _c5(256, 63),
               ("b_conv5_4x31_n256",) + _c5(256, 31), ("b_conv5_4x31_n255",) + _c5(255, 31), ("b_conv5_4x32_n255",) + _c5(255, 32),
               ("c_conv3_8x60",) + _c3(256, 60), ("c_conv3_8x64_n255",) + _c3(255, 64),
               ("d_conv5_4x34",) + _c5(256, 34), ("d_conv5_4x65_n255",) + _c5(255, 65), ("d_conv3_8x33",) + _c3(256, 33)]
CASES = CASES + CLASS_CASES
# cases that must take the fused launch under the default tuning: a change of the plan that drops one of them fails here
MUST_FUSE = set(TILE_CLASSES) | {"conv5_n256", "conv5_n255", "conv3_n256", "conv1_n256"}


def _tile_rows(bm, Ho, Wo, kh):
    """Rows of a bm-row tile that hold data when tiles are cut on window-row (kh*Wo) and image (Ho*Wo) boundaries: the largest
    multiple of a window row <= bm that is a whole number of images or divides one image."""
    img, wrow = Ho * Wo, kh * Wo
    t = (bm // wrow) * wrow
    if t >= img:
        return (t // img) * img
    while t > 0 and img % t:
        t -= wrow
    return t


def _run_case(case, must_fuse):
    """One geometry through the fused launch and through the two launches it replaces; returns nothing, asserts everything."""
    name, N, Cin, H, W, Cout, pk, ps, pp = case
    mr.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(N + Cin + W)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    PH, PW = (H + 2 * pp[0] - pk[0]) // ps[0] + 1, (W + 2 * pp[1] - pk[1]) // ps[1] + 1
    gy = torch.randn(N, Cout, PH, PW, generator=g)

    def run(fused):
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last).to(torch.bfloat16).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        if fused:
            ok = F.conv_relu_pool_eligible(xd, wd, (1, 1), (1, 1), (1, 1), pk, ps, pp)
            if must_fuse:
                assert ok, "%s no longer takes the fused conv + ReLU + max-pool launch" % name
            if not ok:
                # the fused launch rides on the 8-wave tile the plain forward would take: small problems take other tiles
                assert N < 256, name
                pytest.skip("%s at N = %d does not take an 8-wave tile" % (name, N))
            y = F.conv_relu_pool(xd, wd, bd, (1, 1), pk, ps, pp)
        else:
            z = F.conv2d(xd, wd, bd, (1, 1), (1, 1), (1, 1), relu=True, relu_grad_downstream=True)
            y = F.max_pool2d(z, pk, ps, pp, relu_input=True)
        y.backward(gy.to(DEV).contiguous(memory_format=torch.channels_last).to(y.dtype))
        torch.cuda.synchronize()
        return y.detach().clone(), xd.grad.clone(), wd.grad.clone(), bd.grad.clone()

    yf, dxf, dwf, dbf = run(True)
    yu, dxu, dwu, dbu = run(False)
    assert yf.shape == yu.shape == (N, Cout, PH, PW)
    assert torch.equal(yf, yu), float((yf.float() - yu.float()).abs().max())
    assert torch.equal(dxf, dxu)                      # same codes, same ReLU mask, the same dgrad kernel
    for a, r in ((dwf, dwu), (dbf, dbu)):             # split reductions with f32 atomics: equal up to their arrival order
        assert float((a - r).abs().max()) <= 2e-3 * float(r.abs().max()) + 1e-6
    # and against float64 on the bf16-rounded operands
    xr = x.bfloat16().double()
    wr = w.bfloat16().double()
    zr = torch.relu(torch.nn.functional.conv2d(xr, wr, b.double(), 1, 1))
    yr = torch.nn.functional.max_pool2d(zr, pk, ps, pp)
    assert float((yf.double().cpu() - yr).abs().max()) <= 1.6e-2 * float(yr.abs().max())


def _nt_kernel_code(N, Cin, H, W, Cout):
    from megreader_amd import _lib
    return _lib.load().mr_nt_kernel_code(_lib.dtype_code(torch.bfloat16), N * H * W, Cout, 9 * Cin, Cin)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_conv_relu_pool_equals_the_two_launches(case):
    name, N, Cin, H, W, Cout, pk, ps, pp = case
    if name in TILE_CLASSES:
        cls, bm, rows, images = TILE_CLASSES[name]
        img = H * W
        assert _tile_rows(bm, H, W, pk[0]) == rows and rows * 16 >= bm * 15, (name, _tile_rows(bm, H, W, pk[0]))
        assert (rows // img if rows >= img else 0) == images and (images or img % rows == 0)
        assert {"a": images == 1 and rows < bm and bm == 256, "b": images >= 2 and bm == 256, "c": images == 0,
                "d": bm == 272}[cls], name
        if cls == "b" and N == 255:    # the last tile holds one image only
            assert (N * img) % rows == img
        # ... and the forward of this problem takes the tile the class names (256256 / 272256: the 8-wave kernels)
        assert _nt_kernel_code(N, Cin, H, W, Cout) == bm * 1000 + 256, (name, _nt_kernel_code(N, Cin, H, W, Cout))
        print("%s: class (%s), %d of %d tile rows hold data, %s per tile" %
              (name, cls, rows, bm, "%d image(s)" % images if images else "1/%d image" % (img // rows)))
    _run_case(case, name in MUST_FUSE)


# Small grids (fewer tiles than XCDs) of the same 8-wave kernels: the automatic choice never takes them below N = 128, so
# mr_tuning.nt_big forces the 256-row (1) / 272-row (3) kernel.  conv5 at 4x33 fills only 132 of 256 rows (not served), hence no (1).
SMALL = [("conv3_8x32", 1) + _c3(0, 32)[1:], ("conv3_8x32", 3) + _c3(0, 32)[1:], ("conv5_4x32", 1) + _c5(0, 32)[1:],
         ("conv5_4x32", 3) + _c5(0, 32)[1:], ("conv5_4x33", 3) + _c5(0, 33)[1:]]


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("geom", SMALL, ids=["%s_big%d" % (g[0], g[1]) for g in SMALL])
def test_fused_conv_relu_pool_small_grids_with_the_big_tile_forced(geom, n):
    from megreader_amd import _lib
    name, big = geom[0], geom[1]
    old = _lib.set_tuning(nt_big=big)
    try:
        _run_case(("%s_big%d_n%d" % (name, big, n), n) + tuple(geom[2:]), True)
    finally:
        _lib.set_tuning(**old)


CODE_CASES = [c for c in CASES if c[0] in ("conv1_n256", "a_conv3_8x30", "b_conv5_4x31_n255", "c_conv3_8x60", "d_conv5_4x65_n255")]


@pytest.mark.parametrize("case", CODE_CASES, ids=[c[0] for c in CODE_CASES])
def test_fused_launch_writes_the_argmax_codes_of_the_pool_kernel(case):
    """mr_conv2d_fwd_pool against mr_conv2d_fwd + mr_maxpool_fwd through the C ABI: pooled values AND the arg-max code bytes the
    whole backward pass is routed by.  ReLU leaves many all-zero windows, where only the first-maximum rule decides the code."""
    from megreader_amd import _lib
    name, N, Cin, H, W, Cout, pk, ps, pp = case
    g = torch.Generator().manual_seed(N + Cin + W + 1)
    x = torch.randn(N, H, W, Cin, generator=g).to(DEV).to(torch.bfloat16)                       # NHWC
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (Cin * 9) ** 0.5).to(DEV).to(torch.bfloat16)   # KRSC
    b = (torch.randn(Cout, generator=g) * 0.1 - 0.3).to(DEV)     # a negative mean bias: more windows that ReLU clears entirely
    PH, PW = (H + 2 * pp[0] - pk[0]) // ps[0] + 1, (W + 2 * pp[1] - pk[1]) // ps[1] + 1
    dt = _lib.dtype_code(torch.bfloat16)
    conv = (N, H, W, Cin, Cin, Cout)
    tail = (3, 3, 1, 1, 1, 1, 1, 1, H, W)
    assert _lib.load().mr_conv2d_fwd_pool_ok(dt, *conv, *tail, pk[0], pk[1], ps[0], ps[1], pp[0], pp[1]), name
    yf = torch.full((N, PH, PW, Cout), float("nan"), dtype=torch.bfloat16, device=DEV)
    cf = torch.full((N, PH, PW, Cout), 255, dtype=torch.uint8, device=DEV)
    _lib.call("mr_conv2d_fwd_pool", dt, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(yf), _lib.ptr(cf), 1, *conv, *tail,
              pk[0], pk[1], ps[0], ps[1], pp[0], pp[1], PH, PW)
    z = torch.empty((N, H, W, Cout), dtype=torch.bfloat16, device=DEV)
    _lib.call("mr_conv2d_fwd", dt, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(z), 1, *conv, Cout, *tail)
    yu = torch.empty_like(yf)
    cu = torch.empty_like(cf)
    _lib.call("mr_maxpool_fwd", dt, _lib.ptr(z), _lib.ptr(yu), _lib.ptr(cu), N, H, W, Cout, pk[0], pk[1], ps[0], ps[1], pp[0], pp[1],
              PH, PW)
    torch.cuda.synchronize()
    assert torch.equal(yf.view(torch.int16), yu.view(torch.int16))          # every element written, bit for bit
    assert torch.equal(cf, cu), "%d arg-max codes differ" % int((cf != cu).sum())
    assert int(cu.max()) < pk[0] * pk[1]
    # the tie rule is exercised: windows that ReLU cleared entirely exist, and their code is the first tap INSIDE the image
    # (tap 0, or tap 1 in the left padding column of the (0, 1)-padded pools)
    zero = yu == 0
    assert int(zero.sum()) > yu.numel() // 100, "too few all-zero windows for the tie rule to matter"
    first = torch.zeros_like(cu)
    if pp[1]:
        first[:, :, 0, :] = pp[1]
    assert torch.equal(cu[zero], first[zero])


def _backbone_both_ways(net, x, warmup=False):
    def run(env):
        old = os.environ.get("MEGREADER_CONV_POOL")
        os.environ["MEGREADER_CONV_POOL"] = env
        try:
            for p in net.parameters():
                p.grad = None
            y = net(x)
            y.float().square().mean().backward()
            torch.cuda.synchronize()
            return y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()}
        finally:
            if old is None:
                del os.environ["MEGREADER_CONV_POOL"]
            else:
                os.environ["MEGREADER_CONV_POOL"] = old

    if warmup:
        # the first forward of a model pairs every convolution with the BatchNorm behind it; from the second on, those BatchNorms
        # take their batch statistics from the GEMM epilogue instead of a pass of their own (nn/modules.py) -- another summation
        # order, a few bf16 ulps at N = 256 whatever the pooled stages do.  Compare two passes of the same, steady, kind.
        run("0")
    yf, gf = run("1")
    yu, gu = run("0")
    assert torch.equal(yf, yu)
    for k in gf:
        # (the stem's weight gradient is a sum with heavy cancellation reduced with f32 atomics: 0.5 % of its largest element run to run)
        assert float((gf[k] - gu[k]).abs().max()) <= 2e-2 * float(gu[k].abs().max()) + 1e-7, k


def test_crnn_backbone_takes_the_fused_path_and_matches_the_unfused_one():
    from megreader_amd.backbones import crnn_backbone
    mr.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(3)
    net = crnn_backbone().to(DEV).train()
    x = torch.randn(6, 3, 32, 128, device=DEV)
    _backbone_both_ways(net, x)


# fused stages of the backbone at N = 256: conv1's 128-row tile is one window row only where 2 * (W / 2) == 128, i.e. at width 128
# (and 64 / 32); conv3 and conv5 ride on the 256- / 272-row tiles at all three widths
@pytest.mark.parametrize("width,stages", [(128, 3), (120, 2), (240, 2)])
def test_crnn_backbone_at_the_full_batch_counts_its_fused_stages(width, stages, monkeypatch):
    from megreader_amd import _lib
    from megreader_amd.backbones import crnn_backbone
    mr.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(3)
    net = crnn_backbone().to(DEV).train()
    x = torch.randn(256, 3, 32, width, device=DEV)
    # what the plan says for the three pooled stages (conv1 16 x W/2, conv3 8 x W/4, conv5 4 x W/4+1), asked of the library itself
    dt = _lib.dtype_code(torch.bfloat16)
    ok = [_lib.load().mr_conv2d_fwd_pool_ok(dt, 256, h, w, c, c, k, 3, 3, 1, 1, 1, 1, 1, 1, h, w, 2, 2, *sp)
          for (h, w, c, k, sp) in ((16, width // 2, 64, 128, (2, 2, 0, 0)), (8, width // 4, 256, 256, (2, 1, 0, 1)),
                                   (4, width // 4 + 1, 512, 512, (2, 1, 0, 1)))]
    print("width %d: mr_conv2d_fwd_pool_ok of conv1 / conv3 / conv5 = %s" % (width, ok))
    assert ok == [1 if stages == 3 else 0, 1, 1]
    calls = []
    real = F.conv_relu_pool

    def counted(x, weight, *a, **k):
        calls.append(tuple(weight.shape))
        return real(x, weight, *a, **k)
    monkeypatch.setattr(F, "conv_relu_pool", counted)
    _backbone_both_ways(net, x, warmup=True)
    assert len(calls) == stages, calls      # one forward with the fused launches on, one with them off
