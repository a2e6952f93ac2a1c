"""The gather of every implicit-GEMM convolution kernel -- (row m, k) -> (image, hi, wi, channel) -- on EXACT operands
(tests/_conv_geometry_ref.py: x, dy in [-2, 2], weights in {-1, 0, 1}, integer bias): every partial sum is exact in f32 whatever
the order, so each stored element of y, dx, dw and dbias must EQUAL the float64 convolution, element by element, on every kernel
variant x geometry the variant serves: borders on all four sides, stride, dilation, both together, asymmetric everything, Ho = 1,
25 / 32 / 33 / 49 taps, an image smaller than the kernel, windows wholly in padding, a strided dgrad that leaves input rows
untouched, gathered operands with a padded leading dimension.  Outputs have a padded leading dimension and three spare rows
filled with a sentinel that must survive.  Kernel variants are forced through mr_tuning as in tests/test_nt_epilogue_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _conv_geometry_ref as R  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr  # noqa: E402

DEV = "cuda"
SENTINEL = 2048.0     # exact in bf16, beyond every bf16 result (|value| <= 256); only ever compared where nothing may be written
POISON = 100.0        # what the channels beside a sliced operand hold: a gather that strays into them leaves the integer range


def _gathered(t, dtype, gid):
    """NHWC operand t (float64, CPU) on the device in `dtype`; on the PADDED_LD geometries as a 16-byte aligned channel slice of
    a tensor 8 channels wider whose other channels hold POISON.  Returns (tensor, leading dimension)."""
    C = t.shape[-1]
    if gid not in R.PADDED_LD:
        return t.to(DEV, R.TORCH_DTYPE[dtype]).contiguous(), C
    wide = torch.full(t.shape[:-1] + (C + 8,), POISON, dtype=R.TORCH_DTYPE[dtype], device=DEV)
    wide[..., 8:] = t.to(DEV, R.TORCH_DTYPE[dtype])
    view = wide[..., 8:]
    assert view.data_ptr() % 16 == 0 and view.stride(-2) == C + 8
    return view, C + 8


def _sentinel_out(rows, n, dtype):
    ld = R.padded_ld(n)
    return torch.full((rows + 3, ld), SENTINEL, dtype=R.TORCH_DTYPE[dtype], device=DEV), ld


def _check_out(out, rows, n, ref, shape, what):
    """out[:rows, :n] must EQUAL ref (NHWC `shape`); pad columns and spare rows must still hold the sentinel."""
    ref = ref.to(DEV).reshape(rows, n)
    bad = out[:rows, :n] != ref
    if bool(bad.any()):
        where = bad.view(shape).nonzero()[:4].tolist()
        got = [float(out[:rows, :n].reshape(shape)[tuple(i)]) for i in where]
        want = [float(ref.reshape(shape)[tuple(i)]) for i in where]
        raise AssertionError("%s: %d of %d elements differ; first (n, h, w, c) %s got %s want %s"
                             % (what, int(bad.sum()), bad.numel(), where, got, want))
    assert bool((out[:rows, n:] == SENTINEL).all()), (what, "pad columns written")
    assert bool((out[rows:] == SENTINEL).all()), (what, "rows past M written")


def _assert_choice(kernel, M, N, K, cg):
    """Under the tuning that forces `kernel`: the host queries name it, where they can report it."""
    dtype, tuning, code = R.NT_KERNELS[kernel]
    lib = _lib.load()
    if code is not None and "nt_force_bm" in tuning:
        assert lib.mr_nt_tile_code(M, N) == code, (kernel, lib.mr_nt_tile_code(M, N))
    elif code is not None:
        got = lib.mr_nt_kernel_code(dtype_code(R.TORCH_DTYPE[dtype]), M, N, K, cg)
        assert got == code, (kernel, got)


def _case_id(case):
    return "%s-%s-c%d" % case


FWD_CASES, DGRAD_CASES, WGRAD_CASES = R.nt_cases(False), R.nt_cases(True), R.wgrad_cases()


@pytest.mark.parametrize("kernel,gid,cin", FWD_CASES, ids=[_case_id(c) for c in FWD_CASES])
def test_conv_forward_is_exact(kernel, gid, cin):
    dtype = R.NT_KERNELS[kernel][0]
    cout, relu = R.out_channels(gid, cin), R.relu_of(gid, cin)
    c = R.conv_case(gid, cin, cout)
    g = c.geom
    Ho, Wo = R.out_size(g)
    M = g.N * Ho * Wo
    if dtype == R.BF16:
        assert float(c.y.abs().max()) <= R.BF16_EXACT           # a condition on the inputs, not a measurement
    ref = R.to_dtype(torch.relu(c.y) if relu else c.y, dtype)
    x, ldx = _gathered(c.x, dtype, gid)
    w = c.w_krsc.to(DEV, R.TORCH_DTYPE[dtype]).contiguous()
    bias = c.bias.float().to(DEV)
    y, ldy = _sentinel_out(M, cout, dtype)
    if kernel == "ksplit4":
        _lib.ensure_tn_workspace(DEV)
    old = _lib.set_tuning(nt_big_min_k=32, **R.NT_KERNELS[kernel][1])
    try:
        _assert_choice(kernel, M, cout, R.taps(g) * cin, cin)
        call("mr_conv2d_fwd", dtype_code(R.TORCH_DTYPE[dtype]), ptr(x), ptr(w), ptr(bias), ptr(y), relu, g.N, g.H, g.W, cin, ldx,
             cout, ldy, *R.conv_args(g))
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning(**old)
    _check_out(y, M, cout, ref, (g.N, Ho, Wo, cout), "y %s %s Cin %d Cout %d ldx %d relu %d" % (kernel, gid, cin, cout, ldx, relu))


def _dgrad_operands(gid, cg, dtype):
    """dgrad of geometry gid with cg gathered (dy) channels: case, device dy (padded ld on PADDED_LD), w_crsk, Cin."""
    cin = R.out_channels(gid, cg)
    c = R.conv_case(gid, cin, cg)
    dy, lddy = _gathered(c.dy, dtype, gid)
    w_crsk = c.w_krsc.permute(3, 1, 2, 0).to(DEV, R.TORCH_DTYPE[dtype]).contiguous()      # [Cin][R][S][Cout]
    return c, dy, lddy, w_crsk, cin


@pytest.mark.parametrize("kernel,gid,cg", DGRAD_CASES, ids=[_case_id(c) for c in DGRAD_CASES])
def test_conv_dgrad_is_exact(kernel, gid, cg):
    dtype = R.NT_KERNELS[kernel][0]
    c, dy, lddy, w_crsk, cin = _dgrad_operands(gid, cg, dtype)
    g = c.geom
    M = g.N * g.H * g.W
    if dtype == R.BF16:
        assert float(c.dx.abs().max()) <= R.BF16_EXACT
    dx, lddx = _sentinel_out(M, cin, dtype)
    if kernel == "ksplit4":
        _lib.ensure_tn_workspace(DEV)
    old = _lib.set_tuning(nt_big_min_k=32, **R.NT_KERNELS[kernel][1])
    try:
        _assert_choice(kernel, M, cin, R.taps(g) * cg, cg)
        call("mr_conv2d_dgrad", dtype_code(R.TORCH_DTYPE[dtype]), ptr(dy), ptr(w_crsk), ptr(dx), g.N, g.H, g.W, cin, lddx, cg, lddy,
             *R.conv_args(g))
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning(**old)
    _check_out(dx, M, cin, R.to_dtype(c.dx, dtype), (g.N, g.H, g.W, cin),
               "dx %s %s Cout %d Cin %d lddy %d" % (kernel, gid, cg, cin, lddy))
    if gid == "k3_s2_p0_untouched":       # rows no window touches come back as 0, not as the sentinel
        assert not bool(dx[:M, :cin].reshape(g.N, g.H, g.W, cin)[:, 9].any())


@pytest.mark.parametrize("gid,cg", R.dgrad_add_cases(), ids=[g for g, _ in R.dgrad_add_cases()])
def test_conv_dgrad_add_is_exact(gid, cg):
    """mr_conv2d_dgrad_add with an integer addend in dx's (padded) layout, through whatever the dispatcher gives the geometry."""
    dtype = R.BF16
    c, dy, lddy, w_crsk, cin = _dgrad_operands(gid, cg, dtype)
    g = c.geom
    M = g.N * g.H * g.W
    add = R.addend_for(c)
    want = c.dx + add
    assert float(want.abs().max()) <= R.BF16_EXACT
    dx, lddx = _sentinel_out(M, cin, dtype)
    addend = torch.full_like(dx, POISON)
    addend[:M, :cin] = add.reshape(M, cin).to(DEV, torch.bfloat16)
    old = _lib.set_tuning(nt_big_min_k=32)
    try:
        call("mr_conv2d_dgrad_add", dtype_code(torch.bfloat16), ptr(dy), ptr(w_crsk), ptr(dx), ptr(addend), g.N, g.H, g.W, cin, lddx,
             cg, lddy, *R.conv_args(g))
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning(**old)
    _check_out(dx, M, cin, R.to_dtype(want, dtype), (g.N, g.H, g.W, cin), "dx + addend %s Cout %d Cin %d" % (gid, cg, cin))


@pytest.mark.parametrize("variant,gid,cin,cout", WGRAD_CASES, ids=[_case_id(c[:3]) for c in WGRAD_CASES])
def test_conv_wgrad_is_exact(variant, gid, cin, cout):
    """dw and dbias are accumulated: pre-filled with 5.0 they must come back as exactly 5 + reference (exact addends make the
    order of the atomics irrelevant); one guard row behind each must keep its 5.0."""
    dtype = R.wgrad_dtype(variant)
    tdt, dt = R.TORCH_DTYPE[dtype], dtype_code(R.TORCH_DTYPE[dtype])
    c = R.conv_case(gid, cin, cout)
    g = c.geom
    Ho, Wo = R.out_size(g)
    x, ldx = _gathered(c.x, dtype, gid)
    lddy = R.padded_ld(cout)
    dy = torch.zeros((g.N, Ho, Wo, lddy), dtype=tdt, device=DEV)           # channels Cout .. lddy - 1 are zero padding
    dy[..., :cout] = c.dy.to(DEV, tdt)
    geom = (g.N, g.H, g.W, cin, ldx, cout, lddy) + R.conv_args(g)
    want_w = (5.0 + c.dw).float().to(DEV)
    want_b = (5.0 + c.db).float().to(DEV)

    def run(name, *extra):
        dw = torch.full((cout + 1, g.R, g.S, cin), 5.0, device=DEV)
        db = torch.full((cout + 1,), 5.0, device=DEV)
        call(name, dt, ptr(dy), ptr(x), ptr(dw), ptr(db), *geom, *extra)
        torch.cuda.synchronize()
        what = (variant, gid, cin, cout, name) + extra[1:]
        bad = dw[:cout] != want_w
        assert not bool(bad.any()), (what, int(bad.sum()), "first (k, r, s, c)", bad.nonzero()[:4].tolist())
        assert torch.equal(db[:cout], want_b), (what, "dbias", (db[:cout] != want_b).nonzero()[:4].tolist())
        assert bool((dw[cout] == 5.0).all()) and float(db[cout]) == 5.0, (what, "guard row written")

    if variant in ("wgrad_bf16", "wgrad_f32"):
        run("mr_conv2d_wgrad")
        return
    lib = _lib.load()
    _lib.ensure_tn_workspace(DEV)
    tab = torch.zeros(g.N * Ho * Wo, 2, dtype=torch.int32, device=DEV)
    old = _lib.set_tuning(tn_taps_min_p=0) if variant == "taps" else {}
    try:
        assert lib.mr_tn_taps_would_run(*geom) == (1 if variant == "taps" else 0), (variant, gid, cin, cout)
        run("mr_conv2d_wgrad_tab", ptr(tab), 1)
        run("mr_conv2d_wgrad_tab", ptr(tab), 0)         # the table of the first call, trusted
    finally:
        _lib.set_tuning(**old)
