"""The small kernels of the DB / PPM / FPN heads one by one, against float64 torch on the dtype-rounded inputs: nearest
upsampling (with `add`, with a channel slice at the C ABI), the FPN's upsample-and-add, Dropout2d's channel scaling, the 2-D
CTC head with an acting clamp, and every wrapper at logical channel counts that are no multiple of the 16-byte vector.
Bounds: 1e-5 (float32) / 1.2e-2 (bfloat16) of the tensor's max, as test_small_ops_vs_torch uses for this family; exact equality
where the arithmetic is a copy or a single rounding."""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr, vec_of  # noqa: E402
from megreader_amd.nn import functional as F  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(autouse=True)
def _reset_dtype():
    yield
    mr.set_compute_dtype(torch.bfloat16)


def _tol(dtype):
    return 1e-5 if dtype == torch.float32 else 1.2e-2


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _dev(x):
    """A dtype-rounded CPU tensor as a channels-last leaf on the device."""
    return x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)


def _ints(shape, g, dtype):
    return torch.randint(-2, 3, shape, generator=g).to(dtype)


# ------------------------------------------------------------------------------------------------ upsample_nearest
NEAREST_SHAPES = [(2, 8, 3, 5), (1, 24, 1, 1), (3, 64, 4, 7)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_upsample_nearest(dtype, s):
    """Forward is a copy (bit-equal), with `add` one rounding of the float32 sum; with integer upstream gradients in -2..2 the
    s x s sums (|sum| <= 128) are exact in bfloat16 too, so dx is bit-equal to the float64 result."""
    mr.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(10 + s)
    for shape in NEAREST_SHAPES:
        N, C, H, W = shape
        x = torch.randn(shape, generator=g).to(dtype)
        add = torch.randn(N, C, H * s, W * s, generator=g).to(dtype)
        gy = _ints((N, C, H * s, W * s), g, dtype)
        up = TF.interpolate(x.float(), scale_factor=s, mode='nearest')
        xr = x.double().requires_grad_(True)
        TF.interpolate(xr, scale_factor=s, mode='nearest').backward(gy.double())

        xd = _dev(x)
        y = F.upsample_nearest(xd, s)
        assert y.dtype == dtype and torch.equal(y.detach().float().cpu(), up), shape
        y.backward(gy.to(DEV))
        assert xd.grad.shape == x.shape and torch.equal(xd.grad.double().cpu(), xr.grad), shape

        xd, ad = _dev(x), _dev(add)
        y = F.upsample_nearest(xd, s, ad)
        assert y.dtype == dtype and torch.equal(y.detach().cpu(), (up + add.float()).to(dtype)), shape
        y.backward(gy.to(DEV))
        assert torch.equal(xd.grad.double().cpu(), xr.grad), shape
        assert ad.grad.shape == add.shape and torch.equal(ad.grad.float().cpu(), gy.float()), shape


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_add", [False, True])
def test_nearest_up_channel_slice_at_the_c_abi(dtype, with_add):
    """mr_nearest_up_fwd into channels [8, 8 + C) of rows C + 16 wide, mr_nearest_up_bwd out of the same slice: the other
    channels keep their fill, the slice equals the unsliced call bit for bit.  Buffers sized as the header states:
    x [N,H,W,C], add [N,H*s,W*s,C], y / dy [N,H*s,W*s,ld], dx [N,H,W,C]."""
    dt = dtype_code(dtype)
    g = torch.Generator().manual_seed(3)
    for (N, C, H, W), s in zip(NEAREST_SHAPES, (2, 8, 4)):
        assert C % vec_of(dtype) == 0
        ld, coff = C + 16, 8
        OH, OW = H * s, W * s
        x = torch.randn(N, H, W, C, generator=g).to(dtype).to(DEV)
        add = torch.randn(N, OH, OW, C, generator=g).to(dtype).to(DEV) if with_add else None
        plain = torch.empty((N, OH, OW, C), dtype=dtype, device=DEV)
        call("mr_nearest_up_fwd", dt, ptr(x), ptr(add), ptr(plain), N, H, W, C, s, C, 0)
        wide = torch.full((N, OH, OW, ld), 7.0, dtype=dtype, device=DEV)
        call("mr_nearest_up_fwd", dt, ptr(x), ptr(add), ptr(wide), N, H, W, C, s, ld, coff)
        want = x.float().repeat_interleave(s, 1).repeat_interleave(s, 2)
        if with_add:
            want = want + add.float()
        assert torch.equal(plain, want.to(dtype))
        assert torch.equal(wide[..., coff:coff + C], plain)
        assert bool((wide[..., :coff] == 7.0).all()) and bool((wide[..., coff + C:] == 7.0).all())

        dy = torch.full((N, OH, OW, ld), 7.0, dtype=dtype, device=DEV)
        dy[..., coff:coff + C] = _ints((N, OH, OW, C), g, dtype).to(DEV)
        dense = dy[..., coff:coff + C].contiguous()
        dx_plain = torch.empty((N, H, W, C), dtype=dtype, device=DEV)
        dx_slice = torch.full((N, H, W, C), 7.0, dtype=dtype, device=DEV)
        call("mr_nearest_up_bwd", dt, ptr(dense), ptr(dx_plain), N, H, W, C, s, C, 0)
        call("mr_nearest_up_bwd", dt, ptr(dy), ptr(dx_slice), N, H, W, C, s, ld, coff)
        want_dx = dense.double().view(N, H, s, W, s, C).sum((2, 4))
        assert torch.equal(dx_plain.double(), want_dx) and torch.equal(dx_slice, dx_plain)


# ------------------------------------------------------------------------------------------------ upsample_add
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 32])
def test_upsample_add(dtype, C):
    """F.interpolate(x, size, 'bilinear', align_corners=False) + y: up-scaling, a non-integer factor, the identity, a 1 x 1 source
    and a down-scaling; values and both gradients."""
    mr.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(C)
    for (h, w), (oh, ow) in (((4, 8), (8, 16)), ((5, 7), (8, 13)), ((6, 6), (6, 6)), ((1, 1), (3, 2)), ((9, 7), (4, 3))):
        x = torch.randn(2, C, h, w, generator=g).to(dtype)
        y = torch.randn(2, C, oh, ow, generator=g).to(dtype)
        gy = torch.randn(2, C, oh, ow, generator=g).to(dtype)
        xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
        outr = TF.interpolate(xr, (oh, ow), mode='bilinear', align_corners=False) + yr
        outr.backward(gy.double())
        xd, yd = _dev(x), _dev(y)
        out = F.upsample_add(xd, yd)
        out.backward(gy.to(DEV).contiguous(memory_format=torch.channels_last))
        case = ((h, w), (oh, ow))
        assert out.dtype == dtype and _rel(out, outr) < _tol(dtype), case
        assert _rel(xd.grad, xr.grad) < _tol(dtype), case
        assert torch.equal(yd.grad.float().cpu(), gy.float()), case


# ------------------------------------------------------------------------------------------------ dropout2d
@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_channels(dtype):
    """y = x * scale[n, c] with zeros, 1 / (1 - p) and a negative scale: one rounding of the float32 product, both ways."""
    mr.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(6)
    for shape in ((3, 16, 5, 7), (2, 8, 1, 1)):
        N, C = shape[:2]
        x = torch.randn(shape, generator=g).to(dtype)
        gy = torch.randn(shape, generator=g).to(dtype)
        scale = torch.where(torch.rand(N, C, generator=g) < 0.4, 0.0, 1.0 / 0.7)
        scale[0, 1], scale[N - 1, C - 1], scale[0, 0] = -1.75, 0.0, 1.0 / 0.7
        sd = scale.to(DEV)
        xd = _dev(x)
        y = F.ScaleChannelsFn.apply(xd, sd)
        y.backward(gy.to(DEV).contiguous(memory_format=torch.channels_last))
        assert y.dtype == dtype and torch.equal(y.detach().cpu(), (x.float() * scale[:, :, None, None]).to(dtype))
        assert torch.equal(xd.grad.cpu(), (gy.float() * scale[:, :, None, None]).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout2d(dtype):
    mr.set_compute_dtype(dtype)
    N, C = 4, 32
    x = (torch.randn(N, C, 3, 5, generator=torch.Generator().manual_seed(8)).abs() + 0.5).to(dtype)     # no zeros of its own
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    for seed in (0, 1):
        torch.manual_seed(seed)
        y = F.dropout2d(xd, 0.3, True)
        torch.manual_seed(seed)
        keep = torch.empty((N, C), dtype=torch.float32, device=DEV).bernoulli_(0.7)
        want = (xd.float() * (keep / (1.0 - 0.3))[:, :, None, None]).to(dtype)
        assert y.shape == x.shape and torch.equal(y, want)
        dropped = (y == 0).flatten(2).all(2)                               # whole (n, c) planes are zero ...
        assert torch.equal(dropped, keep == 0)
        # ... or x / 0.7: the kernel multiplies by the float32 1 / 0.7, which is within an ulp of the division
        assert _rel(y[~dropped], (xd.float() / 0.7)[~dropped]) < (2e-7 if dtype == torch.float32 else 2.0 ** -8)
        assert 0 < int(dropped.sum()) < N * C
    assert F.dropout2d(xd, 0.3, False) is xd and F.dropout2d(xd, 0.0, True) is xd


# ------------------------------------------------------------------------------------------------ ctc2d_head
def _ctc2d_logits(shape, dtype, clamp):
    """(mask logits a, class logits z), dtype-rounded.  clamp: inputs for tiny = 1e-3.  Class logits scaled by 3 put 70 - 75 % of
    the cells under the clamp at H = 4 and H = 1.  At H = 65 that leaves 96 % clamped whatever the class scale (a flat mask is
    1/65 per row, and sum m p = 1 per column allows few cells above 1e-3): there every 6th row's mask logit is raised by 5 and
    both kinds of logits are flat (x 0.1) otherwise, which clamps about 85 %."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(2 + C)
    a = torch.randn(N, 1, H, W, generator=g)
    z = torch.randn(N, C, H, W, generator=g) * 3
    if clamp and H > 8:
        a = a * 0.1 + 5.0 * (torch.arange(H) % 6 == 0).float().view(1, 1, H, 1)
        z = z / 30
    return a.to(dtype), z.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tiny", [float(torch.finfo(torch.float32).tiny), 1e-3])
@pytest.mark.parametrize("shape", [(3, 38, 4, 5), (2, 130, 1, 6), (1, 70, 65, 3)])
def test_ctc2d_head(dtype, tiny, shape):
    """N * W not a multiple of the 4 columns of a workgroup, C beyond one wave and no multiple of 64, H beyond one wave; float32
    and bfloat16 logits in row-padded buffers.  lp, m, p are float32 outputs: 1e-5 for either logit dtype; the gradients 1e-4
    (float32, as test_ctc2d_head_vs_torch) / 1.2e-2 (bfloat16).  With tiny = 1e-3 the clamp acts on most cells and its gradient
    mask m p > tiny with it; cells whose float64 m p is within 1e-5 of tiny may fall on either side in float32 and are left out."""
    N, C, H, W = shape
    clamp = tiny > 1e-6
    a, z = _ctc2d_logits(shape, dtype, clamp)
    ar, zr = a.double().requires_grad_(True), z.double().requires_grad_(True)
    mp = torch.softmax(ar, 2) * torch.softmax(zr, 1)
    pr = torch.log(torch.max(mp, torch.tensor(tiny, dtype=torch.float64))).permute(3, 2, 0, 1)
    gp = torch.randn(pr.shape, generator=torch.Generator().manual_seed(1))
    pr.backward(gp.double())
    mp = mp.detach()
    frac = float((mp <= tiny).double().mean())
    near = (mp - tiny).abs() <= 1e-5 * tiny                                  # [N, C, H, W]
    print("ctc2d_head %s %s tiny %.1e: clamped %.3f, near the clamp %d of %d" % (shape, dtype, tiny, frac, int(near.sum()),
                                                                                  near.numel()))
    if clamp:
        assert 0.1 <= frac <= 0.9, frac
    else:
        assert frac == 0.0
    assert int(near.sum()) <= near.numel() // 1000

    v = vec_of(dtype)
    Cp = (C + v - 1) // v * v
    ab = torch.zeros(N, H, W, v, dtype=dtype, device=DEV)
    ab[..., :1] = a.permute(0, 2, 3, 1)
    zb = torch.zeros(N, H, W, Cp, dtype=dtype, device=DEV)
    zb[..., :C] = z.permute(0, 2, 3, 1)
    ad = ab[..., :1].permute(0, 3, 1, 2).requires_grad_(True)
    zd = zb[..., :C].permute(0, 3, 1, 2).requires_grad_(True)
    lp, m, p = F.ctc2d_head(ad, zd, tiny)
    assert lp.dtype == m.dtype == p.dtype == torch.float32
    keep_lp = (~near).permute(3, 2, 0, 1)
    e_lp = float(((lp.detach().double().cpu() - pr.detach()).abs() * keep_lp).max() / pr.detach().abs().max())
    assert e_lp < 1e-5, e_lp
    assert _rel(m, torch.softmax(a.double(), 2)) < 1e-5 and _rel(p, torch.softmax(z.double(), 1)) < 1e-5
    lp.backward(gp.to(DEV))
    g_tol = 1e-4 if dtype == torch.float32 else 1.2e-2
    assert ad.grad.shape == a.shape and zd.grad.shape == z.shape
    # a cell near the clamp moves dz of its own cell and, through G_h, the rest of its (n, h, w) pixel and da of its column
    bad_pix = near.any(1, keepdim=True)                                      # [N, 1, H, W]
    bad_col = bad_pix.any(2, keepdim=True)                                   # [N, 1, 1, W]
    dz, da = zd.grad.double().cpu(), ad.grad.double().cpu()
    e_z = float(((dz - zr.grad).abs() * ~bad_pix).max() / zr.grad.abs().max())
    scale_a = float(ar.grad.abs().max())
    if H == 1:          # softmax over one row is the constant 1: no gradient reaches the mask logit; on the upstream's scale
        assert scale_a == 0.0
        scale_a = float(gp.abs().max())
    e_a = float(((da - ar.grad).abs() * ~bad_col).max() / scale_a)
    print("ctc2d_head: lp %.2e dz %.2e da %.2e" % (e_lp, e_z, e_a))
    assert e_z < g_tol and e_a < g_tol, (e_z, e_a)


# ------------------------------------------------------------------------------------------------ logical channel counts
def _check(out, ref, ins, refs, gy, dtype, what):
    assert out.shape == ref.shape and out.dtype == dtype, (what, out.shape, ref.shape, out.dtype)
    assert _rel(out, ref) < _tol(dtype), what
    out.backward(gy.to(DEV))
    ref.backward(gy.double())
    for i, (a, r) in enumerate(zip(ins, refs)):
        assert a.grad is not None and a.grad.shape == r.shape, (what, i, None if a.grad is None else a.grad.shape, r.shape)
        assert _rel(a.grad, r.grad) < _tol(dtype), (what, i)


def _pair(shape, g, dtype):
    x = torch.randn(shape, generator=g).to(dtype)
    return x.to(DEV).requires_grad_(True), x.double().requires_grad_(True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 3, 12])
def test_logical_channel_counts(dtype, C):
    """Channel counts that are no multiple of the 16-byte vector (12 is one in float32, not in bfloat16): the wrappers pad the
    operand for the kernel; the result and the input gradients must come back with the logical channel count."""
    mr.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(20 + C)
    N = 2

    xd, xr = _pair((N, C, 5, 7), g, dtype)
    gy = torch.randn(N, C, 3, 2, generator=g).to(dtype)
    _check(F.adaptive_avg_pool2d(xd, (3, 2)), TF.adaptive_avg_pool2d(xr, (3, 2)), [xd], [xr], gy, dtype, "adaptive_avg_pool2d")

    xd, xr = _pair((N, C, 3, 4), g, dtype)
    gy = torch.randn(N, C, 5, 9, generator=g).to(dtype)
    _check(F.interpolate_bilinear(xd, (5, 9)), TF.interpolate(xr, (5, 9), mode='bilinear', align_corners=False), [xd], [xr],
           gy, dtype, "interpolate_bilinear")

    xd, xr = _pair((N, C, 3, 4), g, dtype)
    yd, yr = _pair((N, C, 6, 8), g, dtype)
    gy = torch.randn(N, C, 6, 8, generator=g).to(dtype)
    _check(F.upsample_add(xd, yd), TF.interpolate(xr, (6, 8), mode='bilinear', align_corners=False) + yr, [xd, yd], [xr, yr],
           gy, dtype, "upsample_add")

    xd, xr = _pair((N, C, 3, 4), g, dtype)
    yd, yr = _pair((N, C, 6, 8), g, dtype)
    gy = torch.randn(N, C, 6, 8, generator=g).to(dtype)
    _check(F.upsample_nearest(xd, 2, yd), TF.interpolate(xr, scale_factor=2, mode='nearest') + yr, [xd, yd], [xr, yr],
           gy, dtype, "upsample_nearest")

    xd, xr = _pair((N, C, 3, 4), g, dtype)
    scale = torch.where(torch.rand(N, C, generator=g) < 0.3, 0.0, 1.0 / 0.7)
    scale[0, 0] = -1.5
    gy = torch.randn(N, C, 3, 4, generator=g).to(dtype)
    _check(F.ScaleChannelsFn.apply(xd, scale.to(DEV)), xr * scale.double()[:, :, None, None], [xd], [xr], gy, dtype,
           "ScaleChannelsFn")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chans", [(3, 8, 12), (8, 1), (12, 12), (1, 3)])
def test_cat_ops_logical_channel_counts(dtype, chans):
    """cat_channels and cat_bilinear with parts of mixed channel counts: the logical concatenation, no zero channels between the
    parts, every part's gradient in its own shape."""
    mr.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(sum(chans))
    N = 2
    pairs = [_pair((N, c, 4, 6), g, dtype) for c in chans]
    gy = torch.randn(N, sum(chans), 4, 6, generator=g).to(dtype)
    out = F.cat_channels([a for a, _ in pairs])
    ref = torch.cat([r for _, r in pairs], 1)
    assert out.shape == ref.shape and torch.equal(out.detach().double().cpu(), ref.detach())
    out.backward(gy.to(DEV))
    off = 0
    for (a, _), c in zip(pairs, chans):
        assert a.grad.shape == (N, c, 4, 6) and torch.equal(a.grad.float().cpu(), gy[:, off:off + c].float())
        off += c

    base = _pair((N, chans[0], 4, 6), g, dtype)
    brs = [_pair((N, c, s_, s_), g, dtype) for c, s_ in zip(chans[1:], (1, 3, 2))]
    out = F.cat_bilinear(base[0], [a for a, _ in brs])
    ref = torch.cat([base[1]] + [TF.interpolate(r, (4, 6), mode='bilinear', align_corners=False) for _, r in brs], 1)
    _check(out, ref, [base[0]] + [a for a, _ in brs], [base[1]] + [r for _, r in brs], gy, dtype, "cat_bilinear")
