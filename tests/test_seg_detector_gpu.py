"""DB head (decoders.SegDetector mirror: HIP convs / BN / nearest upsampling, ConvTranspose2d as a GEMM) against the
oracle restatement (oracle/seg_detector.py, bit-identical to the unmodified reference on CPU -- tests/
test_oracle_models.py): forward maps, loss and every parameter / input gradient, fp32; plus one training step of the
whole DB detector (deformable ResNet-50 + head + loss, BASELINE.json configs[4]) in bf16."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd.decoders import L1BalanceCELoss, SegDetector  # noqa: E402
from megreader_amd.synthetic import detection_batch  # noqa: E402
from oracle.seg_detector import SegDetectorOracle, l1_balance_ce_loss  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True)
def _reset_dtype():
    yield
    mr.set_compute_dtype(torch.bfloat16)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _relu_masks(head_modules):
    """Forward hooks on the ReLU slots (indices 2 and 5) of the binarize / thresh heads: the sign pattern decides which
    elements pass gradient, and an element whose pre-activation is within rounding of zero takes a different side in
    float32 and float64 -- one such element moves dbeta of a 16-channel BN by 1/sqrt(elements per channel) ~ 5e-3."""
    masks, hooks = [], []
    for seq in head_modules:
        for i in (2, 5):
            hooks.append(seq[i].register_forward_hook(lambda m, a, out: masks.append((out.detach() > 0).cpu())))
    return masks, hooks


def test_seg_detector_fp32_vs_oracle():
    """Forward maps, loss and every parameter / input gradient against the oracle in FLOAT64.  The inputs are the first
    seed whose four head ReLU sign patterns agree between the float64 oracle and the HIP float32 run (see
    _relu_masks): with equal masks every operator is smooth and the bar is float32 rounding, 2e-5 of the tensor's max (measured 2e-6)
    for a linear functional of the maps; for the loss (hard-negative top-k of the balanced BCE, k = 50 step function)
    the yardstick is the oracle's own float32 run: 4x its error, floor 5e-5 (measured 2e-6)."""
    import copy
    mr.set_compute_dtype(torch.float32)
    chans = [16, 32, 64, 128]
    torch.manual_seed(3)
    ora32 = SegDetectorOracle(in_channels=chans, inner_channels=64, k=50, adaptive=True).train()
    ora64 = copy.deepcopy(ora32).double().train()
    model = SegDetector(in_channels=chans, inner_channels=64, k=50, adaptive=True)
    model.load_state_dict(ora32.state_dict(), strict=True)
    model.to(DEV).train()
    batch = detection_batch(2, 256, seed=1, boxes=3)

    def run_oracle(ora, dt, feats, functional):
        ora.zero_grad()
        f = [x.detach().clone().to(dt).requires_grad_(True) for x in feats]
        p = ora(f)
        l = functional(p, dt, "cpu")
        l.backward()
        return p, l, f, {k: v.grad.clone() for k, v in ora.named_parameters()}

    def loss_fn(p, dt, dev):
        if dev == "cpu":
            return l1_balance_ce_loss(p, {k: v.to(dt) for k, v in batch.items()})
        return L1BalanceCELoss()(p, {k: v.to(dev) for k, v in batch.items()})[0]

    gw = torch.Generator().manual_seed(5)
    ws = {k: torch.randn(2, 1, 256, 256, generator=gw) for k in ("binary", "thresh")}

    def lin_fn(p, dt, dev):
        return sum((p[k] * ws[k].to(device=dev, dtype=dt)).sum() for k in ws)

    chosen = None
    for seed in range(8):
        g = torch.Generator().manual_seed(seed)
        feats = [torch.randn(2, c, 64 // s, 64 // s, generator=g) for c, s in zip(chans, (1, 2, 4, 8))]
        m_o, h_o = _relu_masks([ora64.binarize, ora64.thresh])
        m_d, h_d = _relu_masks([model.binarize, model.thresh])
        with torch.no_grad():
            ora64([f.double() for f in feats])
            model([f.to(DEV) for f in feats])
        for h in h_o + h_d:
            h.remove()
        if all(torch.equal(a, b) for a, b in zip(m_o, m_d)):
            chosen = feats
            break
    assert chosen is not None, "no seed in 0..7 with agreeing ReLU sign patterns"
    feats = chosen
    print("SegDetector fp32: inputs seed %d" % seed)

    failures, worst = [], {}
    for name, fn, floor in (("linear", lin_fn, 2e-5), ("loss", loss_fn, 5e-5)):
        p64, l64, f64, w64 = run_oracle(ora64, torch.float64, feats, fn)
        p32, l32, f32, w32 = run_oracle(ora32, torch.float32, feats, fn)
        model.zero_grad()
        fd = [f.detach().to(DEV).requires_grad_(True) for f in feats]
        pd = model(fd)
        for k in p64:
            assert pd[k].shape == p64[k].shape and _rel(pd[k], p64[k]) < 2e-4, k
        ld = fn(pd, torch.float32, DEV)
        assert abs(float(ld) - float(l64)) < 1e-4 * max(1.0, abs(float(l64))), (name, float(ld), float(l64))
        ld.backward()
        worst[name] = 0.0
        # the deconvolution biases in front of a BatchNorm (x.3.bias) have a mathematically zero gradient: compare
        # them on the scale of the deconvolution's weight gradient instead of their own
        pairs = [("feature c%d" % (i + 2), a.grad, b.grad, c.grad, None) for i, (a, b, c) in
                 enumerate(zip(fd, f64, f32))]
        for k, p in model.named_parameters():
            assert p.grad is not None, k
            scale = w64[k.replace(".bias", ".weight")].abs().max() if k.endswith(".3.bias") else None
            pairs.append((k, p.grad, w64[k], w32[k], scale))
        for k, a, b, c, scale in pairs:
            if scale is not None:
                e_hip = float((a.double().cpu() - b).abs().max() / scale)
                e_cpu = float((c.double() - b).abs().max() / scale)
            else:
                e_hip, e_cpu = _rel(a, b), _rel(c, b)
            worst[name] = max(worst[name], e_hip)
            bar = floor if name == "linear" else max(4 * e_cpu, floor)
            if not e_hip < bar:
                failures.append((name, k, "hip %.2e" % e_hip, "cpu f32 %.2e" % e_cpu))
    print("SegDetector fp32: worst gradient error vs f64 / max|g|: linear %.2e, loss %.2e"
          % (worst["linear"], worst["loss"]))
    assert not failures, failures


def test_db_detector_training_step_bf16():
    from megreader_amd.backbones import deformable_resnet50
    from megreader_amd.optim import FusedSGD
    mr.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    backbone = deformable_resnet50(pretrained=False).to(DEV).train()
    head = SegDetector(in_channels=[256, 512, 1024, 2048], adaptive=True, k=50).to(DEV).train()
    crit = L1BalanceCELoss()
    params = list(backbone.parameters()) + list(head.parameters())
    opt = FusedSGD(params, lr=0.007, momentum=0.9, weight_decay=1e-4)
    batch = {k: v.to(DEV) for k, v in detection_batch(2, 256, seed=0, boxes=4).items()}
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss, metrics = crit(head(backbone(batch['image'])), batch)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(l == l and abs(l) < 1e3 for l in losses), losses
    assert set(metrics) == {'bce_loss', 'thresh_loss', 'l1_loss'}


@pytest.mark.parametrize("n,quantized", [(2, False), (2, True), (3, False), (1, True)])
def test_fused_db_loss_equals_the_torch_restatement(n, quantized):
    """csrc/db_loss.hip (radix-selected sum of the nc largest negative losses, every reduction, one backward launch) against the
    torch restatement of reference decoders/seg_detector_loss.py:157-185 -- including the [N,N,H,W] broadcast of gt * mask.
    quantized: predictions on a 1/64 grid, so thousands of negative losses are EQUAL at the selection threshold: the loss must
    still agree exactly; the gradient gives the tied elements equal shares (the restatement's sort picks some of them), so it
    is compared where no tie is involved and through its sum."""
    from megreader_amd.decoders import seg_detector_loss as sdl
    g = torch.Generator().manual_seed(11 + n)
    H = W = 256
    batch = {k: v.to(DEV) for k, v in detection_batch(n, H, seed=3, boxes=2).items()}
    batch['mask'][:, :24, :] = 0.0          # ignored pixels
    batch['mask'][0, :, 200:] = 0.0

    def maps():
        out = {}
        for k in ("binary", "thresh", "thresh_binary"):
            p = torch.rand(n, 1, H, W, generator=g) * 0.98 + 0.01
            if quantized:
                p = (p * 64).round().clamp(1, 63) / 64
            out[k] = p.to(DEV).requires_grad_(True)
        return out
    pred = maps()
    res = {}
    for fused in (False, True):
        old = sdl.FUSED_DB_LOSS
        sdl.FUSED_DB_LOSS = fused
        try:
            for v in pred.values():
                v.grad = None
            loss, metrics = L1BalanceCELoss()(pred, batch)
            loss.backward()
            res[fused] = (float(loss), {k: float(v) for k, v in metrics.items()}, {k: v.grad.clone() for k, v in pred.items()})
        finally:
            sdl.FUSED_DB_LOSS = old
    l0, m0, g0 = res[False]
    l1, m1, g1 = res[True]
    assert abs(l0 - l1) < 2e-6 * max(1.0, abs(l0)), (l0, l1)
    for k in m0:
        assert abs(m0[k] - m1[k]) < 2e-6 * max(1.0, abs(m0[k])), (k, m0[k], m1[k])
    for k in ("thresh", "thresh_binary"):
        assert _rel(g1[k], g0[k]) < 1e-5, k
    if not quantized:
        assert _rel(g1["binary"], g0["binary"]) < 1e-5
    else:
        d = (g1["binary"] - g0["binary"]).abs()
        scale = float(g0["binary"].abs().max())
        assert float((d > 1e-5 * scale).float().mean()) < 0.2          # only tied elements may differ ...
        assert abs(float(g1["binary"].sum()) - float(g0["binary"].sum())) < 2e-3 * float(g0["binary"].abs().sum())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_db_head_tail_equals_the_torch_expression(dtype):
    """sigmoid / sigmoid / step function of the DB heads (decoders/seg_detector.py:77-79,142-147) as one launch each way."""
    from megreader_amd.nn import functional as F
    g = torch.Generator().manual_seed(2)
    xb = (torch.randn(2, 1, 40, 56, generator=g) * 3).to(dtype).to(DEV).requires_grad_(True)
    xt = (torch.randn(2, 1, 40, 56, generator=g) * 3).to(dtype).to(DEV).requires_grad_(True)
    w = [torch.randn(2, 1, 40, 56, generator=g).to(DEV) for _ in range(3)]
    k = 50.0
    b, t, tb = F.db_head_tail(xb, xt, k)
    (b * w[0] + t * w[1] + tb * w[2]).sum().backward()
    got = (b.detach(), t.detach(), tb.detach(), xb.grad.clone(), xt.grad.clone())
    xb2 = xb.detach().clone().requires_grad_(True)
    xt2 = xt.detach().clone().requires_grad_(True)
    b2, t2 = torch.sigmoid(xb2.double()), torch.sigmoid(xt2.double())
    tb2 = torch.reciprocal(1 + torch.exp(-k * (b2 - t2)))
    (b2 * w[0] + t2 * w[1] + tb2 * w[2]).sum().backward()
    want = (b2.detach(), t2.detach(), tb2.detach(), xb2.grad, xt2.grad)
    tol = 2e-6 if dtype == torch.float32 else 1e-2
    for i, (a, r) in enumerate(zip(got, want)):
        assert _rel(a, r) < (5e-6 if i < 3 else tol), i


def _head_tail_both_ways(xb, xt, w, k=50.0):
    """(HIP results, float64 torch results) of F.db_head_tail and the gradients of sum_i (out_i * w_i).sum(); w_i = None leaves
    that output without an upstream gradient (the nullable gb / gt / gtb of mr_db_head_tail_bwd)."""
    from megreader_amd.nn import functional as F

    def total(outs):
        return sum((o * wi).sum() for o, wi in zip(outs, w) if wi is not None)
    xb, xt = xb.to(DEV).requires_grad_(True), xt.to(DEV).requires_grad_(True)
    outs = F.db_head_tail(xb, xt, k)
    total(outs).backward()
    got = tuple(o.detach() for o in outs) + (xb.grad.clone(), xt.grad.clone())
    xb2 = xb.detach().clone().requires_grad_(True)
    xt2 = xt.detach().clone().requires_grad_(True)
    b2, t2 = torch.sigmoid(xb2.double()), torch.sigmoid(xt2.double())
    tb2 = torch.reciprocal(1 + torch.exp(-k * (b2 - t2)))
    total((b2, t2, tb2)).backward()
    grads = [x.grad if x.grad is not None else torch.zeros_like(x, dtype=torch.float64) for x in (xb2, xt2)]   # not reached: 0
    return got, (b2.detach(), t2.detach(), tb2.detach(), grads[0], grads[1])


def _head_tail_bounds(dtype):          # as test_db_head_tail_equals_the_torch_expression: outputs (f32), input gradients (dtype)
    return 5e-6, (2e-6 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 3])
def test_db_head_tail_sizes(dtype, n):
    """One element, one element past a workgroup, and three elements past the 4096-workgroup cap of the grid, where the kernels
    stride; the last elements are compared on their own as well.  With one element the max norm is that element's own relative
    error, and the float32 bar follows from the arithmetic instead: binary and thresh are rounded to float32 (2^-25 each below 1),
    the step function multiplies the error of their difference by k = 50, and the product chain adds a few roundings --
    (k + 8) 2^-24 = 3.5e-6 of the gradient."""
    g = torch.Generator().manual_seed(n)
    xb = (torch.randn(1, 1, 1, n, generator=g) * 3).to(dtype)
    xt = (torch.randn(1, 1, 1, n, generator=g) * 3).to(dtype)
    w = [torch.randn(1, 1, 1, n, generator=g).to(DEV) for _ in range(3)]
    got, want = _head_tail_both_ways(xb, xt, w)
    t_out, t_grad = _head_tail_bounds(dtype)
    if n == 1:
        t_grad = max(t_grad, (50.0 + 8) * 2.0 ** -24)
    for i, (a, r) in enumerate(zip(got, want)):
        assert a.shape == r.shape and bool(torch.isfinite(a).all()), i
        assert _rel(a, r) < (t_out if i < 3 else t_grad), i
        tail = slice(max(0, n - 3), n)
        assert float((a[..., tail].double() - r[..., tail]).abs().max()) <= (t_out if i < 3 else t_grad) * float(r.abs().max()), i


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_db_head_tail_saturated_logits(dtype):
    """Logits of +-120: exp(120) overflows float32 and exp(-120) underflows it, so the sigmoids are exactly 0 and 1 -- the float64
    values rounded to float32 -- every output stays finite, and no gradient passes a saturated sigmoid."""
    g = torch.Generator().manual_seed(9)
    shape = (2, 1, 9, 31)
    xs = []
    for _ in range(2):
        x = torch.randn(shape, generator=g) * 3
        kind = torch.randint(0, 4, shape, generator=g)          # half of the elements saturate, either way
        x[kind == 0] = 120.0
        x[kind == 1] = -120.0
        xs.append(x.to(dtype))
    w = [torch.randn(shape, generator=g).to(DEV) for _ in range(3)]
    got, want = _head_tail_both_ways(xs[0], xs[1], w)
    t_out, t_grad = _head_tail_bounds(dtype)
    for a in got:
        assert bool(torch.isfinite(a).all())
    sat = [(x.float().abs() == 120.0).to(DEV) for x in xs]
    for i in (0, 1):
        assert torch.equal(got[i][sat[i]], want[i].float()[sat[i]])     # the float64 sigmoid rounded once
        assert set(got[i][sat[i]].unique().tolist()) == {0.0, 1.0}
        assert not got[3 + i][sat[i]].any()                     # b (1 - b) = 0
        assert _rel(got[i], want[i]) < t_out and _rel(got[3 + i], want[3 + i]) < t_grad
    # thresh_binary: where both sigmoids saturate, binary - thresh is exactly -1, 0 or 1 and the map spans 1 / (1 + exp(+-50)):
    # those element by element on their own scale (one expf and one divide), the whole map in the max norm
    both = sat[0] & sat[1]
    assert int(both.sum()) > 50
    assert float(((got[2].double() - want[2]).abs() / want[2])[both].max()) < t_out
    assert _rel(got[2], want[2]) < t_out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_db_head_tail_single_upstream_gradient(dtype, which):
    """Only one of binary / thresh / thresh_binary feeds the loss: the other two upstream gradients arrive as None."""
    g = torch.Generator().manual_seed(4 + which)
    shape = (2, 1, 7, 37)
    xb = (torch.randn(shape, generator=g) * 3).to(dtype)
    xt = (torch.randn(shape, generator=g) * 3).to(dtype)
    w = [torch.randn(shape, generator=g).to(DEV) if i == which else None for i in range(3)]
    got, want = _head_tail_both_ways(xb, xt, w)
    _, t_grad = _head_tail_bounds(dtype)
    if which == 0:
        assert not got[4].any() and not want[4].any()           # thresh does not reach binary
    if which == 1:
        assert not got[3].any() and not want[3].any()
    for i in (3, 4):
        assert _rel(got[i], want[i]) < t_grad, i
