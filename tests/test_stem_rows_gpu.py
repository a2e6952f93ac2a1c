"""The bf16 MFMA stem kernels (megreader_amd/csrc/stem.hip) at the C ABI, at the shapes where their tiling can go wrong:
a workgroup owns a run of pooled rows of one image, keeps the run's input rows in LDS and requests the next strip's rows
while it computes the current one; the backward sums whole runs per workgroup and reduces few partial sets.

Data are small dyadic numbers (as in test_stem_gpu.py): every product and sum is exact in bf16 operands / f32 accumulation,
so every comparison is torch.equal -- the forward against the generic FMA kernel of the same entry point (wpack = NULL),
the backward against a float64 torch reference."""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from megreader_amd._lib import MR_BF16, call, load, ptr  # noqa: E402

DEV = "cuda"

# (N, H, W): one strip with both halo rows outside the image and three idle waves; first + last strip and an odd strip
# count; a strip count that is no multiple of a run; the recognition crop's rows; a wave tail (W/2 = 80); the widest row
# the LDS rule admits; more strips than the backward launches workgroups
SHAPES = [(1, 2, 32), (1, 4, 32), (1, 6, 32), (5, 10, 32), (2, 32, 128), (2, 4, 160), (1, 4, 992), (70, 32, 32)]
# ... and more RUNS of strips than it launches workgroups (each workgroup then sums several runs)
BWD_SHAPES = SHAPES + [(520, 2, 32)]
CINS = [1, 3]

_CACHE = {}


def _reference(x, w, b, gy):
    """CPU torch, float64: conv -> relu -> maxpool on bf16-rounded operands; y and the gradients wrt w and b."""
    x = x.bfloat16().double()
    w = w.bfloat16().double().requires_grad_(True)
    b = b.double().requires_grad_(True)
    y = TF.max_pool2d(TF.relu(TF.conv2d(x, w, b, padding=1)), 2, 2)
    y.backward(gy.double())
    return y.detach(), w.grad, b.grad


def _case(N, C, H, W):
    """Inputs on the device, the float64 reference and the MFMA forward's codes: made once per shape, never modified."""
    key = (N, C, H, W)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(N * 1000 + C * 100 + H + W)
        x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
        w = torch.randint(-4, 5, (64, C, 3, 3), generator=g).float() / 8
        b = torch.randint(-8, 9, (64,), generator=g).float() / 8
        gy = torch.randint(-4, 5, (N, 64, H // 2, W // 2), generator=g).float()
        y_ref, dw_ref, db_ref = _reference(x, w, b, gy)
        d = dict(x=x.to(DEV), w=w.to(DEV), b=b.to(DEV), dw_ref=dw_ref, db_ref=db_ref, y_ref=y_ref,
                 dy=gy.to(DEV).permute(0, 2, 3, 1).contiguous().bfloat16())
        d['y'], d['code'] = _forward(d['x'], d['w'], d['b'], mfma=True)
        _CACHE[key] = d
    return _CACHE[key]


def _pack(w):
    wpack = torch.empty((64, 32), dtype=torch.bfloat16, device=DEV)
    call("mr_stem_pack", ptr(w), *w.stride(), ptr(wpack), w.shape[1])
    return wpack


def _forward(x, w, b, mfma, y=None, want_code=True):
    N, C, H, W = x.shape
    if y is None:
        y = torch.empty((N, H // 2, W // 2, 64), dtype=torch.bfloat16, device=DEV)
    code = torch.empty((N, H // 2, W // 2, 64), dtype=torch.uint8, device=DEV) if want_code else None
    call("mr_stem_fwd", MR_BF16, ptr(x), ptr(w), *w.stride(), ptr(_pack(w)) if mfma else 0, ptr(b), ptr(y), ptr(code),
         N, C, H, W)
    return y, code


def _workspace(C, fill=None):
    ws = torch.empty((load().mr_stem_bwd_workspace(C),), dtype=torch.float32, device=DEV)
    if fill is not None:
        ws.view(torch.uint8).fill_(fill)
    return ws


def _backward(d, ws, dw, db):
    N, C, H, W = d['x'].shape
    strides = dw.stride() if dw is not None else (0, 0, 0, 0)
    call("mr_stem_bwd", MR_BF16, ptr(d['dy']), ptr(d['code']), ptr(d['x']), ptr(ws), ptr(dw), *strides, ptr(db), N, C, H, W)


def _zeros(C):
    return torch.zeros((64, C, 3, 3), device=DEV), torch.zeros((64,), device=DEV)


@pytest.mark.parametrize("C", CINS)
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_forward_equals_generic_kernel_bit_for_bit(N, H, W, C):
    d = _case(N, C, H, W)
    y_g, code_g = _forward(d['x'], d['w'], d['b'], mfma=False)
    assert torch.equal(d['y'].view(torch.int16), y_g.view(torch.int16))
    assert torch.equal(d['code'], code_g)
    # ... and both are the reference's values (exact, then rounded to bf16)
    assert torch.equal(d['y'].float().cpu().permute(0, 3, 1, 2), d['y_ref'].float().bfloat16().float())


@pytest.mark.parametrize("C", CINS)
@pytest.mark.parametrize("N,H,W", [(1, 6, 32), (2, 32, 128)])
def test_forward_ties_and_negative_bias(N, H, W, C):
    d = _case(N, C, H, W)
    # constant image: every window away from the border is an exact four-way tie -> first maximum, position 0
    x1 = torch.ones_like(d['x'])
    y_m, code_m = _forward(x1, d['w'], d['b'], mfma=True)
    y_g, code_g = _forward(x1, d['w'], d['b'], mfma=False)
    assert torch.equal(y_m.view(torch.int16), y_g.view(torch.int16)) and torch.equal(code_m, code_g)
    if H >= 6:
        assert int((code_m[:, 1:-1, 1:-1] & 3).max()) == 0
    # bias below every sum (|conv| <= 27 * 3 * 0.5): ReLU passes nothing, bit 2 is clear everywhere, y is zero
    bn = torch.full_like(d['b'], -64.0)
    y_m, code_m = _forward(d['x'], d['w'], bn, mfma=True)
    y_g, code_g = _forward(d['x'], d['w'], bn, mfma=False)
    assert torch.equal(code_m, code_g) and int((code_m & 4).max()) == 0
    assert int(y_m.view(torch.int16).abs().max()) == 0 and int(y_g.view(torch.int16).abs().max()) == 0


@pytest.mark.parametrize("C", CINS)
@pytest.mark.parametrize("N,H,W", [(1, 2, 32), (5, 10, 32), (2, 32, 128)])
@pytest.mark.parametrize("mfma", [True, False])
def test_forward_without_code_buffer(N, H, W, C, mfma):
    """code == NULL: y is the same and nothing is written outside y."""
    d = _case(N, C, H, W)
    n = d['y'].numel()
    guard = 4096
    buf = torch.full((n + 2 * guard,), -2.0, dtype=torch.bfloat16, device=DEV)   # -2.0 is no ReLU output
    y = buf[guard:guard + n].view(d['y'].shape)
    _forward(d['x'], d['w'], d['b'], mfma=mfma, y=y, want_code=False)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), d['y'].view(torch.int16))
    assert bool((buf[:guard] == -2.0).all()) and bool((buf[guard + n:] == -2.0).all())


@pytest.mark.parametrize("C", CINS)
@pytest.mark.parametrize("N,H,W", BWD_SHAPES)
def test_backward_equals_float64_reference(N, H, W, C):
    d = _case(N, C, H, W)
    ws = _workspace(C, fill=0xFF)                     # the workspace need not be initialised: all-ones bytes (NaNs)
    dw, db = _zeros(C)
    _backward(d, ws, dw, db)
    assert torch.equal(dw.double().cpu(), d['dw_ref'])
    assert torch.equal(db.double().cpu(), d['db_ref'])
    # the same call twice more on the same workspace: identical
    for _ in range(2):
        dw2, db2 = _zeros(C)
        _backward(d, ws, dw2, db2)
        assert torch.equal(dw2, dw) and torch.equal(db2, db)
    # accumulation into pre-filled sinks; a channels-last (strided) dw sink
    g = torch.Generator().manual_seed(7)
    pw = torch.randint(-5, 6, (64, C, 3, 3), generator=g).float().to(DEV)
    pb = torch.randint(-5, 6, (64,), generator=g).float().to(DEV)
    dw3 = pw.clone().contiguous(memory_format=torch.channels_last)
    db3 = pb.clone()
    _backward(d, ws, dw3, db3)
    assert torch.equal(dw3.double().cpu(), d['dw_ref'] + pw.double().cpu())
    assert torch.equal(db3.double().cpu(), d['db_ref'] + pb.double().cpu())
    # either sink may be null
    dw4, db4 = _zeros(C)
    _backward(d, ws, dw4, None)
    _backward(d, ws, None, db4)
    assert torch.equal(dw4, dw) and torch.equal(db4, db)


@pytest.mark.parametrize("C", CINS)
@pytest.mark.parametrize("N,H,W", [(5, 10, 32), (2, 32, 128), (520, 2, 32)])
def test_backward_graph_replay(N, H, W, C):
    """One single-stream capture, replayed three times on the same workspace."""
    d = _case(N, C, H, W)
    ws = _workspace(C)
    dw, db = _zeros(C)
    _backward(d, ws, dw, db)                          # (loads the library and the kernels outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _backward(d, ws, dw, db)
    for _ in range(3):
        dw.zero_()
        db.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dw.double().cpu(), d['dw_ref'])
        assert torch.equal(db.double().cpu(), d['db_ref'])
