"""Exact convolution cases for the gather of the implicit-GEMM kernels (tests/test_conv_geometry_gpu.py), importable without a GPU:
the geometry table, the kernel x geometry x channel case lists, the integer operand builder and the float64 reference.

The gather -- (row m, k) -> (image, hi, wi, channel) -- exists in several independently written copies (csrc/igemm_core.h:
igemm_nt_body AMODE 1 / 2, igemm_nt_glds_kernel AMODE 2 / 3 with 2 or 4 stage buffers, igemm_nt_big_kernel; igemm_p8.h;
igemm_nt32.h; the split reduction that starts a split in the middle of the k range; dgrad's flipped tap offset).  With x, dy in
[-2, 2], weights in {-1, 0, 1} and an integer bias every partial sum is an integer far below 2^24: exact in f32 in any order,
so every stored element must EQUAL the float64 result -- one wrong tap at one corner pixel fails.  bf16 outputs additionally
need |value| <= 256 (every such integer is a bf16), which the builder's callers assert on the reference (a condition on the
inputs: if a seed breaks it, the seed changes, not the bound)."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as TF

BF16, F32 = "bf16", "f32"
TORCH_DTYPE = {BF16: torch.bfloat16, F32: torch.float32}
VEC = {BF16: 8, F32: 4}
BF16_EXACT = 256          # integers up to here are bf16 values; a difference of 1 cannot hide in the store's rounding

Geometry = collections.namedtuple("Geometry", "id H W R S sh sw ph pw dh dw N")


def _geom(gid, H, W, R, S, s, p, d=(1, 1), N=8):
    return Geometry(gid, H, W, R, S, s[0], s[1], p[0], p[1], d[0], d[1], N)


# 8 images: k3_p1 has 280 forward rows = one 256- / 272-row tile + an edge tile (interior and edge paths in one launch); the
# 1x1 image gets 280 of them for the same reason
GEOMETRIES = collections.OrderedDict((g.id, g) for g in [
    _geom("k3_p1", 5, 7, 3, 3, (1, 1), (1, 1)),                      # every border class of the common layer
    _geom("k3_s2", 9, 13, 3, 3, (2, 2), (1, 1)),                     # stride, odd sizes
    _geom("k3_d2", 6, 7, 3, 3, (1, 1), (2, 2), (2, 2)),              # dilation
    _geom("k3_s2_d2", 9, 10, 3, 3, (2, 2), (2, 2), (2, 2)),          # stride and dilation together
    _geom("k23_s21", 6, 9, 2, 3, (2, 1), (0, 1)),                    # attention encoder: everything asymmetric
    _geom("k2_p0_ho1", 2, 9, 2, 2, (1, 1), (0, 0)),                  # Ho == 1
    _geom("k5_p2", 5, 6, 5, 5, (1, 1), (2, 2)),                      # 25 taps on the mask path
    _geom("k48_32taps", 6, 9, 4, 8, (1, 1), (2, 4)),                 # exactly 32 taps: bit 31 of the mask
    _geom("k3x11_33taps", 5, 12, 3, 11, (1, 1), (1, 5)),             # 33 taps: first shape on the general gather
    _geom("k7_s2_p3", 11, 13, 7, 7, (2, 2), (3, 3)),                 # ResNet stem geometry (general gather)
    _geom("k3_1x1img", 1, 1, 3, 3, (1, 1), (1, 1), N=280),           # image smaller than the kernel: one valid tap
    _geom("k1_s2", 7, 9, 1, 1, (2, 2), (0, 0)),                      # downsample branch
    _geom("k3_p2_overpad", 4, 5, 3, 3, (1, 1), (2, 2)),              # padding > dilation * (k - 1) / 2: corner windows keep ONE tap
    _geom("k3_p3_overpad", 4, 5, 3, 3, (1, 1), (3, 3)),              # corner windows wholly in padding: output is bias only
    _geom("k3_d13", 5, 9, 3, 3, (1, 1), (1, 3), (1, 3)),             # unequal dilation
    _geom("k3_s2_p0_untouched", 10, 8, 3, 3, (2, 2), (0, 0)),        # dgrad: input row 9 is touched by no window
])
GEOM_INDEX = {gid: i for i, gid in enumerate(GEOMETRIES)}
PADDED_LD = ("k3_p1", "k23_s21")       # gathered operand is a channel slice of a wider tensor (ld = channels + 8) here


def taps(g):
    return g.R * g.S


def out_size(g):
    return ((g.H + 2 * g.ph - g.dh * (g.R - 1) - 1) // g.sh + 1, (g.W + 2 * g.pw - g.dw * (g.S - 1) - 1) // g.sw + 1)


def conv_args(g):
    """The geometry tail of the C entry points: R, S, sh, sw, ph, pw, dh, dw, Ho, Wo."""
    return (g.R, g.S, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw) + out_size(g)


# Gathered channel counts (the input for forward / wgrad, the gradient for dgrad).  64: one k-step per tap; 128: two, the tap
# state carries across steps; 8, 24 (bf16) and 4 (f32): per-vector tap arithmetic, a k-step spans several taps, 24 is no power
# of two.  |y|, |dx| stay <= 256 up to K = R*S*C = 2112 and reach 260..368 from K = 3136: 128 channels go with <= 9 taps only,
# and the 49-tap geometry keeps the small counts in bf16.
GATHERED = {BF16: (64, 128, 8, 24), F32: (32, 64, 4)}
# 72: ragged column tile of whole vectors; 64: a full tile; 44: N % 8 != 0 (element-wise stores) -- all with a padded ld
OUT_CHANNELS = (72, 64, 44)


def gathered_channels(gid, dtype):
    g = GEOMETRIES[gid]
    if dtype == F32:
        return GATHERED[F32]
    return tuple(c for c in GATHERED[BF16] if taps(g) * c <= 2112 and (c < 128 or taps(g) <= 9))


def out_channels(gid, cg):
    return OUT_CHANNELS[(GEOM_INDEX[gid] + cg // 8) % 3]


def relu_of(gid, cg):
    """ReLU on half of the forward cases."""
    return (GEOM_INDEX[gid] + cg // 4) % 2


def padded_ld(n, vec=8):
    """Leading dimension of an output with n channels: n rounded up to 8, plus 8."""
    return (n + vec - 1) // vec * vec + 8


# ---- kernel variants: name -> (dtype, tuning that forces it, mr_nt_tile_code / mr_nt_kernel_code it must report or None) --------
# every launch runs with nt_big_min_k = 32 on top of these
NT_KERNELS = collections.OrderedDict([
    ("default", (BF16, dict(), None)),
    ("tile128_2buf", (BF16, dict(nt_force_bm=128, nt_force_bn=128, nt_deep=0), 128128)),
    ("tile64_4buf", (BF16, dict(nt_force_bm=64, nt_force_bn=64, nt_deep=2), 64064)),
    ("tile96x64", (BF16, dict(nt_force_bm=96, nt_force_bn=64), 96064)),
    ("staged", (BF16, dict(nt_variant=1), None)),
    ("big256", (BF16, dict(nt_big=1), 256256)), ("big272", (BF16, dict(nt_big=3), 272256)),
    ("big288x128", (BF16, dict(nt_big=7), 288128)), ("w8_128x128", (BF16, dict(nt_big=8), None)),
    ("w8_128x64", (BF16, dict(nt_big=10), None)), ("w8_96x128", (BF16, dict(nt_big=13), None)),
    ("p8", (BF16, dict(nt_big=1, nt_p8=1), 256256)),
    ("m32_256x256", (BF16, dict(nt_m32=2), None)), ("m32_288x256", (BF16, dict(nt_m32=3), None)),
    ("m32_256x128", (BF16, dict(nt_m32=4), None)), ("m32_128x256", (BF16, dict(nt_m32=5), None)),
    ("ksplit4", (BF16, dict(nt_force_bm=128, nt_force_bn=128, nt_ksplit=4), 128128)),
    ("default_f32", (F32, dict(), None)),
    ("tile128_f32", (F32, dict(nt_force_bm=128, nt_force_bn=128), 128128)),
    ("tile64_f32", (F32, dict(nt_force_bm=64, nt_force_bn=64), 64064)),
    ("staged_f32", (F32, dict(nt_variant=1), None)),
])
# the 8-wave, phased and ping-pong kernels: bf16, gathered channels a multiple of 64, <= 32 taps, dgrad at unit stride only
WIDE_KERNELS = tuple(k for k in NT_KERNELS if k.startswith(("big", "w8_", "p8", "m32_")))


def _fast_gather(g, dgrad):
    return taps(g) <= 32 and not (dgrad and (g.sh, g.sw) != (1, 1))


def nt_cases(dgrad):
    """[(kernel, geometry id, gathered channels)] of the forward (dgrad=False) or dgrad test: every kernel on every geometry
    it serves.  default / f32 kernels: every gathered channel count; the forced 4-wave and the register-staged kernels: 64, one
    of 8 / 24 and (<= 9 taps) 128; the wide kernels: 64 and (<= 9 taps) 128 on the fast-gather geometries; the split reduction:
    the 128-channel 3x3 cases (K = 1152 = 18 k-steps) on the fast gather."""
    cases = []
    for kernel, (dtype, _, _) in NT_KERNELS.items():
        for gid, g in GEOMETRIES.items():
            chans = gathered_channels(gid, dtype)
            if kernel in WIDE_KERNELS:
                chans = [c for c in chans if c % 64 == 0] if _fast_gather(g, dgrad) else []
            elif kernel == "ksplit4":
                chans = [c for c in chans if c == 128] if (g.R, g.S) == (3, 3) and _fast_gather(g, dgrad) else []
            elif dtype == BF16 and kernel != "default":
                small = (8, 24)[GEOM_INDEX[gid] % 2]
                chans = [c for c in chans if c in (64, 128, small)] if 64 in chans else list(chans)
            cases += [(kernel, gid, c) for c in chans]
    return cases


def dgrad_add_cases():
    """One mr_conv2d_dgrad_add case per geometry, default dispatch, the largest 64-or-smaller gathered count it allows."""
    return [(gid, 64 if 64 in gathered_channels(gid, BF16) else 24) for gid in GEOMETRIES]


# all-taps weight-gradient kernel (csrc/tn_taps.hip: 3x3, stride 1, padding == dilation, Cin % 64 == 0, Cout % 8 == 0, at
# least 32 table entries per image): mr_tn_taps_would_run must say 1 for these under tn_taps_min_p = 0
TAPS_GEOMETRIES = ("k3_p1", "k3_d2")


def wgrad_cases():
    """[(variant, geometry id, Cin, Cout)]: mr_conv2d_wgrad in both dtypes on every geometry and channel count; the row-table
    entry (bf16, <= 32 taps) with build = 1 then build = 0; the all-taps kernel where it runs (Cout 72 where the geometry's own
    output width is no multiple of 8)."""
    cases = []
    for gid, g in GEOMETRIES.items():
        cases += [("wgrad_bf16", gid, c, out_channels(gid, c)) for c in gathered_channels(gid, BF16)]
        cases += [("wgrad_f32", gid, c, out_channels(gid, c)) for c in gathered_channels(gid, F32)]
        if taps(g) <= 32:
            cases += [("tab", gid, c, out_channels(gid, c)) for c in gathered_channels(gid, BF16)]
    for gid in TAPS_GEOMETRIES:
        for c in gathered_channels(gid, BF16):
            if c % 64 == 0:
                cases.append(("taps", gid, c, out_channels(gid, c) if out_channels(gid, c) % 8 == 0 else 72))
    return cases


def wgrad_dtype(variant):
    return F32 if variant == "wgrad_f32" else BF16


# ---- operands and reference ---------------------------------------------------------------------------------------------------
def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def conv_f64(x_nhwc, w_krsc, bias, g):
    """float64 convolution of NHWC / KRSC operands by the library call; NHWC result."""
    y = TF.conv2d(x_nhwc.permute(0, 3, 1, 2), w_krsc.permute(0, 3, 1, 2), bias, (g.sh, g.sw), (g.ph, g.pw), (g.dh, g.dw))
    return y.permute(0, 2, 3, 1)


def conv_replicate_f64(x_nhwc, w_krsc, bias, g):
    """Deliberately wrong: the border pixels repeated into the padding instead of zeros."""
    xp = TF.pad(x_nhwc.permute(0, 3, 1, 2), (g.pw, g.pw, g.ph, g.ph), mode="replicate")
    return TF.conv2d(xp, w_krsc.permute(0, 3, 1, 2), bias, (g.sh, g.sw), 0, (g.dh, g.dw)).permute(0, 2, 3, 1)


def conv_rot180_f64(x_nhwc, w_krsc, bias, g):
    """Deliberately wrong: the kernel rotated by 180 degrees (a gather that walks the taps backwards)."""
    return conv_f64(x_nhwc, w_krsc.flip(1, 2), bias, g)


def _with_grads(fn, x, w, b, dy, g):
    x, w, b = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)      # problems this small spend their time in the thread pool otherwise (8 threads: 50x slower)
    try:
        y = fn(x, w, b, g)
        y.backward(dy)
    finally:
        torch.set_num_threads(threads)
    return y.detach(), x.grad, w.grad, b.grad


Case = collections.namedtuple("Case", "geom cin cout x w_krsc bias dy y dx dw db")


@functools.lru_cache(maxsize=None)
def conv_case(gid, cin, cout, batch=None):
    """Integer operands of geometry gid with cin input and cout output channels (float64, NHWC / KRSC; treat as read-only) and
    the float64 results: y = conv + bias (before any ReLU), and for the upstream gradient dy the autograd dx, dw (KRSC), db."""
    g = GEOMETRIES[gid]
    if batch is not None:
        g = g._replace(N=batch)
    gen = torch.Generator().manual_seed(zlib.crc32(("%s/%d/%d" % (gid, cin, cout)).encode()))
    Ho, Wo = out_size(g)
    x = _ints((g.N, g.H, g.W, cin), -2, 2, gen)
    w = _ints((cout, g.R, g.S, cin), -1, 1, gen)
    b = _ints((cout,), -4, 4, gen)
    dy = _ints((g.N, Ho, Wo, cout), -2, 2, gen)
    y, dx, dw, db = _with_grads(conv_f64, x, w, b, dy, g)
    return Case(g, cin, cout, x, w, b, dy, y, dx, dw, db)


def addend_for(c):
    """Integer addend of mr_conv2d_dgrad_add for case c: dx's shape, values in [-4, 4]."""
    gen = torch.Generator().manual_seed(zlib.crc32(("add/%s/%d/%d" % (c.geom.id, c.cin, c.cout)).encode()))
    return _ints(tuple(c.dx.shape), -4, 4, gen)


def wrong_references(c):
    """{name: (y, dx)} of the two wrong gathers on the operands of case c."""
    out = {}
    for name, fn in (("replicate", conv_replicate_f64), ("rot180", conv_rot180_f64)):
        y, dx, _, _ = _with_grads(fn, c.x, c.w_krsc, c.bias, c.dy, c.geom)
        out[name] = (y, dx)
    return out


def padded_sides(g):
    """{side: (output rows or columns whose window reaches into that side's padding, axis)} for the sides that have padding and
    at least one such window."""
    Ho, Wo = out_size(g)
    sides = {}
    top = [h for h in range(Ho) if h * g.sh - g.ph < 0]
    bottom = [h for h in range(Ho) if h * g.sh - g.ph + (g.R - 1) * g.dh > g.H - 1]
    left = [w for w in range(Wo) if w * g.sw - g.pw < 0]
    right = [w for w in range(Wo) if w * g.sw - g.pw + (g.S - 1) * g.dw > g.W - 1]
    for name, idx, axis in (("top", top, 1), ("bottom", bottom, 1), ("left", left, 2), ("right", right, 2)):
        if idx and (g.ph if axis == 1 else g.pw):
            sides[name] = (idx, axis)
    return sides


def seven_loops(c):
    """Forward (without bias) and input gradient of case c restated as seven plain loops over Python integers: (y, dx) as
    float64 tensors.  For the smallest cases only."""
    g = c.geom
    Ho, Wo = out_size(g)
    x, w, dy = c.x.long().tolist(), c.w_krsc.long().tolist(), c.dy.long().tolist()
    y = [[[[0] * c.cout for _ in range(Wo)] for _ in range(Ho)] for _ in range(g.N)]
    dx = [[[[0] * c.cin for _ in range(g.W)] for _ in range(g.H)] for _ in range(g.N)]
    for n in range(g.N):
        for ho in range(Ho):
            for wo in range(Wo):
                for k in range(c.cout):
                    for r in range(g.R):
                        for s in range(g.S):
                            hi, wi = ho * g.sh - g.ph + r * g.dh, wo * g.sw - g.pw + s * g.dw
                            if not (0 <= hi < g.H and 0 <= wi < g.W):
                                continue
                            for ci in range(c.cin):
                                y[n][ho][wo][k] += x[n][hi][wi][ci] * w[k][r][s][ci]
                                dx[n][hi][wi][ci] += dy[n][ho][wo][k] * w[k][r][s][ci]
    return torch.tensor(y, dtype=torch.float64), torch.tensor(dx, dtype=torch.float64)


def to_dtype(ref, dtype):
    """The one rounding of the store: exact in f32, then to the output dtype."""
    return ref.float().to(TORCH_DTYPE[dtype])
