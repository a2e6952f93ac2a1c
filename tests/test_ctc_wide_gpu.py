"""1-D CTC on wide alphabets (csrc/ctc.hip: mr_ctc_wide -- row-parallel log-softmax + class-streaming gradient kernel) against
float64 on the CPU: F.ctc_loss(F.log_softmax(x.double(), 2), ..., zero_infinity=True) and its gradient with respect to x.

Bars (inputs randn * 2, so every |lp| < 32):
  loss             relative 1e-6
  log-probability  3.8e-6 absolute = 2 float32 ulps at |lp| < 32 (one for the rounded difference, one for lz)
  gradient         |g - g_ref| <= rel * |g_ref| + 2e-6 * k_b,  k_b = 1 / (N * max(L_b, 1));  rel = 5e-6 in f32 (the log-probability
                   bar carried through exp), 2^-7 in bf16 (two bf16 unit round-offs: f64 -> f32 -> bf16).  No flat absolute bar: the
                   median |g| at these shapes is 2e-7 .. 2e-6
  row sum (f32)    |sum_c g[t, b, :]| <= 1e-6 * k_b on every active row.  Measured on the MI355X: 4.4e-7 .. 9.97e-7 over the cases
                   (9.0e-7 at 3 932 classes on the kernels for narrow alphabets).  Nearly all of it is sum_c exp(lp) - 1 of the
                   float32 log-probabilities themselves (printed next to it: 4.7e-7 .. 9.7e-7), i.e. the rounding of
                   lz = max + logf(sum) near 10; the gradient kernel adds a few 1e-8 to it
  exact            through the C ABI into a NaN-filled padded buffer: no NaN left; rows at or beyond the input length, padding
                   columns and dead samples exact zeros; nothing behind the buffer touched
Every case plants class C-1, class 2 and the classes 64k-1 / 64k in its targets and asserts the path (mr_ctc_wide) it took."""
import functools

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr, vec_of  # noqa: E402
from megreader_amd.nn import functional as F  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
LP_BAR = 3.8e-6
GUARD = 256


def _plant(targets, lengths, C):
    """class C-1, class 2, 64k-1 and 64k (last / first lane of a sweep) into the two longest targets"""
    order = sorted(range(len(lengths)), key=lambda i: -int(lengths[i]))
    a, b = order[0], order[1]
    assert int(lengths[a]) >= 3 and int(lengths[b]) >= 2
    k = max(1, (C // 64) // 2)
    targets[a, 0], targets[a, 2] = C - 1, 64 * k - 1
    targets[b, 0], targets[b, 1] = 64 * k, 2
    return targets


def _six(C, seed, S=32, T=12):
    """the six samples of tests/test_kernels_gpu.py::test_ctc_matches_torch_and_oracle: a repeated label, an empty target and an
    infeasible sample (ten repeats in twelve frames)"""
    g = torch.Generator().manual_seed(seed)
    N = 6
    logits = torch.randn(T, N, C, generator=g) * 2
    lengths = torch.tensor([3, 1, 6, 0, 10, 5])
    targets = torch.zeros(N, S, dtype=torch.int32)
    for i, L in enumerate(lengths.tolist()):
        targets[i, :L] = torch.randint(2, C, (L,), generator=g, dtype=torch.int32)
    targets[4, :10] = 5                       # 10 repeats need T >= 19 > 12: infeasible -> zero_infinity path
    targets = _plant(targets, torch.tensor([3, 1, 6, 0, 0, 5]), C)      # (not into the infeasible one)
    targets[2, 1] = targets[2, 0]            # repeated label (class C-1 twice)
    return logits, targets, torch.full((N,), T, dtype=torch.int64), lengths


def _ragged(C, seed):
    """T = 26, N = 16 with the ragged input lengths of test_ctc_ragged_input_lengths_at_the_32x100_shape"""
    g = torch.Generator().manual_seed(seed)
    T, N, S = 26, 16, 32
    logits = torch.randn(T, N, C, generator=g) * 2
    lengths = torch.randint(3, 11, (N,), generator=g)
    lengths[3] = 0
    targets = torch.zeros(N, S, dtype=torch.int32)
    for i, L in enumerate(lengths.tolist()):
        targets[i, :L] = torch.randint(2, C, (L,), generator=g, dtype=torch.int32)
    targets = _plant(targets, lengths.clone().index_fill_(0, torch.tensor([15]), 0), C)
    targets[2, 1] = targets[2, 0]
    in_len = torch.tensor([26, 25, 26, 7, 21, 26, 13, 26, 20, 26, 24, 26, 11, 26, 26, 1])
    in_len = torch.maximum(in_len, 2 * lengths + 1)
    in_len[15], lengths[15] = 1, 3                               # 3 labels in one step -> zero_infinity path
    targets[15, :3] = torch.tensor([4, 9, 4], dtype=torch.int32)
    return logits, targets, in_len, lengths


def _nine(C, seed):
    """T = 33, N = 9, S = 25 of test_ctc_scaled_linear_domain_equals_log_domain (int64 targets)"""
    g = torch.Generator().manual_seed(seed)
    T, N, S = 33, 9, 25
    logits = torch.randn(T, N, C, generator=g) * 2
    lengths = torch.tensor([3, 1, 6, 0, 10, 5, 25, 12, 2])
    in_len = torch.tensor([33, 20, 33, 5, 12, 33, 33, 30, 1])
    targets = torch.zeros(N, S, dtype=torch.int64)
    for i, L in enumerate(lengths.tolist()):
        targets[i, :L] = torch.randint(1, C, (L,), generator=g)
    targets[6, :25] = torch.randperm(C - 2, generator=g)[:25] + 2        # 25 distinct labels fit 33 frames
    targets = _plant(targets, torch.tensor([0, 0, 0, 0, 0, 0, 25, 12, 0]), C)
    targets[2, 1] = targets[2, 0]
    targets[4, :10] = 5                        # 10 repeats in 12 frames: infeasible
    return logits, targets, in_len, lengths


def _long(C, seed):
    """T = 130: the emission table [T][2S+1] f64 exceeds 64 KB, so the log-domain recursion feeds the wide gradient kernel"""
    g = torch.Generator().manual_seed(seed)
    T, N, S = 130, 3, 32
    logits = torch.randn(T, N, C, generator=g) * 2
    lengths = torch.tensor([32, 0, 7])
    in_len = torch.tensor([130, 130, 101])
    targets = torch.zeros(N, S, dtype=torch.int32)
    for i, L in enumerate(lengths.tolist()):
        targets[i, :L] = torch.randint(2, C, (L,), generator=g, dtype=torch.int32)
    targets = _plant(targets, lengths, C)
    targets[0, 5] = targets[0, 4]
    return logits, targets, in_len, lengths


def _three_pass(C, seed):
    """C > 8192: the log-softmax rows no longer fit in registers (three passes over the logits)"""
    g = torch.Generator().manual_seed(seed)
    T, N, S = 5, 2, 8
    logits = torch.randn(T, N, C, generator=g) * 2
    lengths = torch.tensor([3, 2])
    targets = torch.zeros(N, S, dtype=torch.int32)
    for i, L in enumerate(lengths.tolist()):
        targets[i, :L] = torch.randint(2, C, (L,), generator=g, dtype=torch.int32)
    targets = _plant(targets, lengths, C)
    return logits, targets, torch.tensor([5, 4]), lengths


#        name: (builder, C, S, wide)
CASES = {
    "first_refused_3933": (lambda: _six(3933, 23), 3933, 32, 1),
    "odd_4099": (lambda: _six(4099, 24), 4099, 32, 1),
    "chinese_26x16": (lambda: _ragged(5360, 29), 5360, 32, 1),
    "chinese_33x9_S25": (lambda: _nine(5360, 31), 5360, 25, 1),
    "long_130x3_4099": (lambda: _long(4099, 37), 4099, 32, 1),
    "three_pass_8200": (lambda: _three_pass(8200, 41), 8200, 8, 1),
    "three_pass_8197": (lambda: _three_pass(8197, 43), 8197, 8, 1),
    "guard_96": (lambda: _six(96, 25), 96, 32, 0),
    "guard_3932": (lambda: _six(3932, 26), 3932, 32, 0),
}


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    """inputs and the float64 CPU reference of one case, computed once and shared (never modified)"""
    logits, targets, in_len, lengths = CASES[name][0]()
    logits = logits.to(dtype)
    x = logits.double().requires_grad_(True)
    lp = TF.log_softmax(x, dim=2)
    loss = TF.ctc_loss(lp, targets, in_len, lengths, zero_infinity=True)
    loss.backward()
    nll = TF.ctc_loss(lp.detach(), targets, in_len, lengths, reduction='none', zero_infinity=False)
    C = logits.shape[2]
    tl = targets[:, :int(lengths.max())]
    assert all(int((tl == c).sum()) for c in (C - 1, 2))
    assert bool(((tl % 64 == 63) & (tl > 2)).any() and ((tl % 64 == 0) & (tl > 2)).any())
    return dict(logits=logits, targets=targets, in_len=in_len, lengths=lengths, lp=lp.detach(), loss=float(loss.detach()),
                grad=x.grad.detach(), dead=torch.isinf(nll))


def _kb(ref):
    N = ref["lengths"].numel()
    return (1.0 / (N * ref["lengths"].clamp(min=1).double())).view(1, N, 1)


def _check_values(ref, dtype, loss, logp, grad, what):
    lp_err = float((logp.double().cpu() - ref["lp"]).abs().max())
    g = grad.double().cpu()
    rel = 5e-6 if dtype == torch.float32 else 2.0 ** -7
    kb = _kb(ref)
    excess = ((g - ref["grad"]).abs() - rel * ref["grad"].abs()) / kb        # in units of k_b: must stay <= 2e-6
    print("%s: loss %.9f (ref %.9f)  log-prob max|d| %.2e  gradient excess over rel*|g_ref| %.2e k_b" %
          (what, float(loss), ref["loss"], lp_err, float(excess.max())))
    assert float(ref["lp"].abs().max()) < 32
    assert abs(float(loss) - ref["loss"]) <= 1e-6 * max(1.0, abs(ref["loss"]))
    assert lp_err <= LP_BAR
    assert float(excess.max()) <= 2e-6
    if dtype == torch.float32:
        T = g.shape[0]
        active = (torch.arange(T).view(T, 1) < ref["in_len"].view(1, -1)) & ~ref["dead"].view(1, -1)
        rows = (g.sum(dim=2).abs() / kb[:, :, 0])[active]
        fwd = (logp.double().cpu().exp().sum(dim=2) - 1).abs()[active]     # what the float32 log-probabilities alone leave
        print("%s: row sum max %.2e k_b (sum_c exp(lp) - 1 of the same log-probabilities: max %.2e)" %
              (what, float(rows.max()), float(fwd.max())))
        assert float(rows.max()) <= 1e-6


def _run_functional(ref, dtype, **kw):
    xd = ref["logits"].to(DEV).requires_grad_(True)
    loss, logp = F.ctc_loss_logits(xd, ref["targets"].to(DEV), ref["in_len"].to(DEV), ref["lengths"].to(DEV), **kw)
    return xd, loss, logp


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", [n for n in CASES if n != "chinese_33x9_S25"])
def test_ctc_against_float64(name, dtype):
    _, C, S, wide = CASES[name]
    assert _lib.load().mr_ctc_wide(C, S) == wide
    ref = _reference(name, dtype)
    xd, loss, logp = _run_functional(ref, dtype)
    assert loss.dtype == torch.float64 and logp.dtype == torch.float32
    loss.backward()
    assert xd.grad.dtype == dtype and xd.grad.shape == xd.shape
    _check_values(ref, dtype, loss, logp, xd.grad, "%s %s" % (name, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("linear", [0, 1])
def test_ctc_wide_in_both_recursion_domains(linear, dtype):
    """mr_tuning.ctc_linear = 0 / 1: the wide gradient kernel serves the log-domain and the scaled linear-domain alpha / beta"""
    name = "chinese_33x9_S25"
    assert _lib.load().mr_ctc_wide(5360, 25) == 1
    ref = _reference(name, dtype)
    old = _lib.set_tuning(ctc_linear=linear)
    try:
        xd, loss, logp = _run_functional(ref, dtype, log_probs_f64=True)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning(**old)
    assert logp.dtype == torch.float64
    assert torch.equal(logp.float().double(), logp)              # the float32 values widened, nothing more
    _check_values(ref, dtype, loss, logp, xd.grad, "%s linear=%d %s" % (name, linear, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ctc_wide_per_sample(dtype):
    """per_sample=True, zero_infinity=False (the reference's own python CTCLoss: nll_b / L_b, no batch mean) on the first case's
    inputs without the infeasible sample; each sample's loss gets its own upstream weight"""
    full = _reference("first_refused_3933", dtype)
    keep = torch.tensor([0, 1, 2, 3, 5])
    logits, targets = full["logits"][:, keep].contiguous(), full["targets"][keep]
    in_len, lengths = full["in_len"][keep], full["lengths"][keep]
    N = keep.numel()
    w = torch.tensor([0.5, -1.25, 2.0, 0.0, 1.0], dtype=torch.float64)      # the empty target (nll / 0) gets weight 0
    x = logits.double().requires_grad_(True)
    lp = TF.log_softmax(x, dim=2)
    nll = TF.ctc_loss(lp, targets, in_len, lengths, reduction='none', zero_infinity=False)
    per_ref = nll / lengths.clamp(min=1)
    (per_ref * w).sum().backward()
    assert _lib.load().mr_ctc_wide(3933, 32) == 1
    xd = logits.to(DEV).requires_grad_(True)
    per, logp = F.ctc_loss_logits(xd, targets.to(DEV), in_len.to(DEV), lengths.to(DEV), per_sample=True, zero_infinity=False)
    assert per.shape == (N,) and per.dtype == torch.float64
    pos = lengths > 0
    assert float(((per.cpu() - per_ref.detach()).abs() / per_ref.detach().abs().clamp(min=1.0))[pos].max()) <= 1e-6
    (per[pos.to(DEV)] * w[pos].to(DEV)).sum().backward()
    assert float((logp.double().cpu() - lp.detach()).abs().max()) <= LP_BAR
    rel = 5e-6 if dtype == torch.float32 else 2.0 ** -7
    kb = (w.abs() / lengths.clamp(min=1).double()).view(1, N, 1)             # |upstream gradient| / L_b: k_b of this mode
    err = (xd.grad.double().cpu() - x.grad).abs() - rel * x.grad.abs()
    assert bool((xd.grad[:, 3] == 0).all()) and bool((x.grad[:, 3] == 0).all())
    excess = (err / kb.clamp(min=1e-30))[:, pos]
    print("per-sample %s: gradient excess %.2e k_b" % (dtype, float(excess.max())))
    assert float(excess.max()) <= 2e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pad", ["vector", "odd"])
@pytest.mark.parametrize("name", ["first_refused_3933", "odd_4099", "chinese_26x16", "long_130x3_4099"])
def test_ctc_wide_gradient_buffer_is_written_exactly_once(name, pad, dtype):
    """mr_ctc_fwd / mr_ctc_bwd through the C ABI into a NaN-filled [T][N][ldg] buffer.  pad = vector: ldg as CTCLossFn pads it (a
    multiple of 8 in bf16, 4 in f32: 16-byte stores); odd: the next ldg that is no such multiple (scalar stores)."""
    _, C, S, wide = CASES[name]
    assert _lib.load().mr_ctc_wide(C, S) == wide == 1
    ref = _reference(name, dtype)
    logits = ref["logits"].to(DEV)
    T, N, _ = logits.shape
    v = vec_of(dtype)
    ldg = -(-C // v) * v if pad == "vector" else (C + 1 if (C + 1) % v else C + 2)
    targets, in_len, lengths = ref["targets"].to(DEV), ref["in_len"].to(DEV).long(), ref["lengths"].to(DEV).long()
    t64 = int(targets.dtype == torch.int64)
    lp = torch.full((T, N, C), float("nan"), dtype=torch.float32, device=DEV)
    alpha = torch.empty((N, T, 2 * S + 1), dtype=torch.float64, device=DEV)
    beta = torch.empty_like(alpha)
    nll = torch.empty((N,), dtype=torch.float64, device=DEV)
    loss = torch.empty((), dtype=torch.float64, device=DEV)
    call("mr_ctc_fwd", dtype_code(dtype), ptr(logits), C, ptr(targets), t64, ptr(in_len), ptr(lengths), 1, T, N, C, S, 0, 1,
         ptr(lp), ptr(alpha), ptr(beta), ptr(nll), ptr(loss), 0)
    n = T * N * ldg
    whole = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    gout = torch.ones((), dtype=torch.float64, device=DEV)
    call("mr_ctc_bwd", dtype_code(dtype), ptr(lp), ptr(alpha), ptr(beta), ptr(nll), ptr(targets), t64, ptr(in_len), ptr(lengths),
         1, ptr(gout), T, N, C, S, 0, 1, ptr(whole), ldg)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(lp).any())
    assert bool(torch.isnan(whole[n:]).all()), "wrote behind the gradient buffer"
    g = whole[:n].view(T, N, ldg).cpu()
    assert not bool(torch.isnan(g).any()), "an element of grad[T][N][ldg] was not written"
    assert bool((g[:, :, C:] == 0).all()), "padding columns"
    assert torch.equal(torch.isinf(nll.cpu()), ref["dead"])
    assert bool((g[:, ref["dead"]] == 0).all()), "dead samples"
    for b in range(N):
        assert bool((g[int(ref["in_len"][b]):, b] == 0).all()), "rows at or beyond the input length"
    live = g[:, :, :C][:int(ref["in_len"].min()), ~ref["dead"]]
    assert bool((live != 0).any(dim=2).all())                    # ... and only those
    rel = 5e-6 if dtype == torch.float32 else 2.0 ** -7
    excess = ((g[:, :, :C].double() - ref["grad"]).abs() - rel * ref["grad"].abs()) / _kb(ref)
    assert float(excess.max()) <= 2e-6


# ---------------------------------------------------------------------------------------------- eval side at 5 360 classes
def test_softmax_eval_at_5360_classes():
    g = torch.Generator().manual_seed(47)
    T, N, C = 26, 4, 5360
    logits = torch.randn(T, N, C, generator=g) * 2
    out = F.softmax_eval_nc1t(logits.to(DEV))
    assert out.shape == (N, C, 1, T) and out.dtype == torch.float32
    ref = TF.log_softmax(logits.double(), dim=2).permute(1, 2, 0).unsqueeze(2)
    assert float(ref.abs().max()) < 32
    err = float((out.double().cpu().log() - ref).abs().max())
    print("softmax_eval_nc1t at C = 5360: max |log p - log p_f64| %.2e" % err)
    assert err <= LP_BAR


def test_greedy_decode_at_5360_classes():
    """bit-exact against oracle.decode.greedy_decode on one synthetic score tensor: winners throughout 0 .. C-1, exact ties (the
    lower index wins), repeats, blanks and `unknown`."""
    from megreader_amd.ops.decode import ctc_greedy_decode
    from oracle.decode import greedy_decode
    g = torch.Generator().manual_seed(53)
    N, C, T = 4, 5360, 26
    p = torch.rand(N, C, 1, T, generator=g) * 0.5
    win = torch.randint(0, C, (N, T), generator=g)
    win[0, :8] = torch.tensor([C - 1, C - 1, 0, C - 1, 1, C - 1, 2, 2])          # repeats, blank between repeats, unknown
    win[1, :6] = torch.tensor([63, 64, 64, 1, 64, 5359])
    win[2, :4] = torch.tensor([4095, 4096, 0, 0])
    for n in range(N):
        for t in range(T):
            p[n, win[n, t], 0, t] = 0.75
    # exact ties: the same top score at a higher index as well -> the lower index must win
    for n, t, hi in ((0, 9, C - 1), (1, 7, 4097), (2, 5, 65), (3, 0, 5000), (3, 1, C - 1)):
        lo = int(win[n, t])
        if hi == lo:
            hi = lo + 1 if lo + 1 < C else lo
        if hi < lo:
            lo, hi = hi, lo
            p[n, lo, 0, t] = 0.75
        p[n, hi, 0, t] = 0.75
    want = greedy_decode(p.numpy())
    assert int(p.argmax(dim=1).max()) > 5000 and int((want != 0).sum()) > 60
    ids, lens = ctc_greedy_decode(p.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), torch.from_numpy(want))
    assert torch.equal(lens.cpu(), torch.from_numpy((want != 0).sum(axis=1)).int())
