"""The fused update kernels (mr_adam_step / mr_sgd_step, csrc/elementwise.hip) and the device step counter, element by element
against torch.optim.Adam / torch.optim.SGD run in float64 on the CPU -- through the C ABI and through FusedAdam / FusedSGD.

Measure, after every step: err = max |x_hip - x_f64| / max(|x_f64|, floor), floor = lr for the parameters and the smallest
normal float32 for the state buffers.  Bar: BAR times the same figure of torch's OWN optimizer run in float32 on the same
inputs (the yardstick): the kernel does float32 arithmetic like it, and additionally forms 1 - beta^t in float32 where torch
forms it in double.  The state figures say little where n is large: fresh gradient signs every step make some of 4 M momentum
elements cancel to 1e-7 of their terms, and both float32 runs are then wrong by the element's own size; every state error feeds
the parameters, whose figure is the one that bites.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd._lib import call, ptr  # noqa: E402
from megreader_amd.nn import prep  # noqa: E402
from megreader_amd.optim import FusedAdam, FusedSGD  # noqa: E402

from _abi_util import GUARD, guarded, job_table  # noqa: E402

DEV = "cuda"
K_STEPS = 25
# Kernel error / yardstick error measured on the MI355X, over the six sizes (CHANGELOG.md has the yardsticks beside them):
#   mr_adam_step  parameters 0 .. 1.80, m 0 .. 3.31, v 0 .. 1.96    (before the bias correction went through expm1 / log: parameters
#                 up to 34 at beta2 = 0.999, 1.1 at beta2 = 0.9)
#   mr_sgd_step   parameters 0.82 .. 1.91, momentum buffer 0.63 .. 1.62; without weight decay bit-identical to torch (1.00)
#   FusedAdam / FusedSGD on the two-layer net 0.77 .. 1.28, graph replay 0.99
# The margin is for the one thing the kernel does in float32 and torch in double, 1 - beta^t.
BAR = 8.0
FLT_MIN = float(np.finfo(np.float32).tiny)
SIZES = [1, 3, 4, 5, 1027, 4194304 + 4 * 256 * 3 + 3]      # tail only, vector + tail, ..., grid-stride loop (4096 blocks) + tail
ADAM_HYPER = [(1e-3, .9, .999, 1e-8, 0.), (1e-2, .9, .999, 1e-3, 1e-2), (1e-3, .5, .9, 1e-8, 1e-4)]    # lr, b1, b2, eps, wd
SGD_HYPER = [(0.007, 0.9, 1e-4), (0.1, 0., 0.), (0.01, 0.5, 0.)]                                       # lr, momentum, wd


@pytest.fixture(autouse=True)
def _reset_dtype():
    yield
    mr.set_compute_dtype(torch.bfloat16)


def _f32(x):
    """The value the kernel receives in its float32 hyper slot."""
    return float(np.float32(x))


def _log_uniform(g, n, lo, hi):
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * (np.log10(hi) - np.log10(lo)) + np.log10(lo))
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (mag * sign).float()


class _Inputs(object):
    """Parameters spread log-uniformly over 1e-3..1e1 and K_STEPS fresh gradients over 1e-8..1e3 with every 7th element exactly
    zero (sqrt(v)-dominated, eps-dominated and v == 0 elements).  Step k's gradient is a window of one random pool moved by a
    step-dependent offset: every element sees a new magnitude and sign each step at the cost of one copy."""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.n = n
        self.p0 = _log_uniform(g, n, 1e-3, 1e1)
        self.pool = _log_uniform(g, n + 1009 * K_STEPS, 1e-8, 1e3)

    def grad(self, k):
        out = self.pool[1009 * k:1009 * k + self.n].clone()
        out[::7] = 0.
        return out


_INPUTS = {}


def _inputs(n):
    if n not in _INPUTS:
        _INPUTS[n] = _Inputs(n, 1234 + n % 1000)
    return _INPUTS[n]


def _torch_opt(kind, p, hp):
    if kind == "adam":
        lr, b1, b2, eps, wd = (_f32(x) for x in hp)
        return torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    lr, mu, wd = (_f32(x) for x in hp)
    return torch.optim.SGD([p], lr=lr, momentum=mu, weight_decay=wd, foreach=False)


def _state(kind, opt, p):
    st = opt.state[p]
    if kind == "adam":
        return [st['exp_avg'], st['exp_avg_sq']]
    return [st['momentum_buffer']] if st.get('momentum_buffer') is not None else []


def _err(x, ref, floor):
    """max |x - ref| / max(|ref|, floor), evaluated in float64 on the device (the large cases move 100 MB per step through it)."""
    x, ref = x.detach().to(DEV).double(), ref.detach().to(DEV)
    return float(((x - ref).abs_() / ref.abs().clamp_min_(floor)).max())


class _Tracker(object):
    """Worst err over the steps, per quantity, of the kernel and of the float32 yardstick against one float64 run."""

    def __init__(self, names):
        self.names = names
        self.hip = dict.fromkeys(names, 0.0)
        self.yard = dict.fromkeys(names, 0.0)

    def update(self, name, hip, yard, ref, floor):
        self.hip[name] = max(self.hip[name], _err(hip, ref, floor))
        self.yard[name] = max(self.yard[name], _err(yard, ref, floor))

    def check(self, what):
        for name in self.names:
            ratio = self.hip[name] / self.yard[name] if self.yard[name] > 0 else (0.0 if self.hip[name] == 0 else float("inf"))
            print("%s %s: kernel %.3e yardstick %.3e ratio %.2f" % (what, name, self.hip[name], self.yard[name], ratio))
        for name in self.names:
            assert self.hip[name] <= BAR * self.yard[name], (what, name, self.hip[name], self.yard[name])


def _tick_table():
    """A real one-job mr_prep_batch table (a four-element bias sum) whose launch carries the tick."""
    src = torch.arange(4, dtype=torch.float32, device=DEV)
    dst = torch.zeros(4, dtype=torch.float32, device=DEV)
    table, njobs, nblocks = job_table([prep.bias_job(ptr(src), 0, ptr(dst), 4, 0)])
    return (table, njobs, nblocks, src, dst)


def _advance(hyper, mode, tick_table):
    if mode == "tick":
        call("mr_opt_tick", ptr(hyper))
    else:
        call("mr_prep_batch", 0, ptr(tick_table[0]), tick_table[1], tick_table[2], ptr(hyper))


def _run_abi(kind, hp, n, gs, mode):
    """K_STEPS steps of the kernel, the float64 reference and the float32 yardstick in lockstep; lr changes after step 10."""
    inp = _inputs(n)
    nstate = 2 if kind == "adam" else 1
    names = ["p", "m", "v"][:1 + nstate] if kind == "adam" else ["p", "buf"]
    p64 = inp.p0.double().requires_grad_(True)
    # the yardstick may run anywhere (it is torch's own float32 optimizer either way): on the device where the buffers are large
    p32 = inp.p0.clone().to(DEV if n > (1 << 20) else "cpu").requires_grad_(True)
    o64, o32 = _torch_opt(kind, p64, hp), _torch_opt(kind, p32, hp)
    bufs = [guarded(n, torch.float32, sentinel=0.0) for _ in range(1 + nstate)]
    for whole, _ in bufs:
        whole[n:] = 5.0                       # guard band behind the parameters and the (zero-initialised) state
    p_d = bufs[0][1]
    p_d.copy_(inp.p0)
    g_d = torch.empty(n, dtype=torch.float32, device=DEV)
    hyper = torch.zeros(8, dtype=torch.float32, device=DEV)
    vals = list(hp) if kind == "adam" else [hp[0], hp[1], 0., 0., hp[2]]
    hyper[:5] = torch.tensor(vals, dtype=torch.float32)
    hyper[6] = gs
    scale = gs if gs != 0 else 1.0            # a power of two: g * scale is exact in both precisions
    tick_table = _tick_table() if mode == "prep" else None
    lr = _f32(hp[0])
    track = _Tracker(names)
    for k in range(K_STEPS):
        if k == 10:
            lr = _f32(hp[0] * 0.3)
            hyper[0] = lr
            o64.param_groups[0]['lr'] = o32.param_groups[0]['lr'] = lr
        g = inp.grad(k)
        g_d.copy_(g)
        if kind == "adam":
            call("mr_adam_step", ptr(p_d), ptr(g_d), ptr(bufs[1][1]), ptr(bufs[2][1]), n, ptr(hyper))
        else:
            call("mr_sgd_step", ptr(p_d), ptr(g_d), ptr(bufs[1][1]), n, ptr(hyper))
        assert float(hyper[5]) == k           # the update launch only reads the counter ...
        _advance(hyper, mode, tick_table)
        assert float(hyper[5]) == k + 1       # ... and the launch behind it adds exactly one
        p64.grad = g.double() * scale
        p32.grad = (g_d if p32.is_cuda else g) * scale
        o64.step()
        o32.step()
        track.update("p", p_d, p32, p64, lr)
        s64, s32 = _state(kind, o64, p64), _state(kind, o32, p32)
        if s64:
            for name, (_, view), a, b in zip(names[1:], bufs[1:], s32, s64):
                track.update(name, view, a, b, FLT_MIN)
        else:       # SGD without momentum and weight decay: the buffer is the scaled gradient itself
            assert hp[1] == 0 and hp[2] == 0
            assert torch.equal(bufs[1][1].cpu(), g * scale)
            track.names = ["p"]
    for whole, _ in bufs:
        assert bool((whole[n:] == 5.0).all()) and whole.numel() == n + GUARD
    track.check("%s %s n=%d gs=%g %s" % (kind, hp, n, gs, mode))
    return track


def _variants(hi, si):
    return (0.0, 0.25)[(hi + si) % 2], ("tick", "prep")[((hi + si) // 2 + hi) % 2]


@pytest.mark.parametrize("si", range(len(SIZES)), ids=["n%d" % n for n in SIZES])
@pytest.mark.parametrize("hi", range(len(ADAM_HYPER)), ids=["h%d" % i for i in range(len(ADAM_HYPER))])
def test_adam_step_matches_torch_float64(hi, si):
    gs, mode = _variants(hi, si)
    _run_abi("adam", ADAM_HYPER[hi], SIZES[si], gs, mode)


@pytest.mark.parametrize("si", range(len(SIZES)), ids=["n%d" % n for n in SIZES])
@pytest.mark.parametrize("hi", range(len(SGD_HYPER)), ids=["h%d" % i for i in range(len(SGD_HYPER))])
def test_sgd_step_matches_torch_float64(hi, si):
    gs, mode = _variants(hi, si)
    _run_abi("sgd", SGD_HYPER[hi], SIZES[si], gs, mode)


def test_variants_cover_both_scales_and_both_ticks_at_every_size():
    for si in range(len(SIZES)):
        seen = {_variants(hi, si) for hi in range(3)}
        assert {v[0] for v in seen} == {0.0, 0.25} and {v[1] for v in seen} == {"tick", "prep"}


def test_step_counter():
    hyper = torch.zeros(8, dtype=torch.float32, device=DEV)
    hyper[0] = 1e-3
    call("mr_prep_batch", 0, 0, 0, 0, ptr(hyper))                 # no jobs, a tick: adds one
    assert float(hyper[5]) == 1
    call("mr_prep_batch", 1, 0, 0, 0, 0)                          # no jobs, no tick: nothing
    table, njobs, nblocks, src, dst = _tick_table()
    call("mr_prep_batch", 0, ptr(table), njobs, nblocks, 0)       # jobs, tick = NULL: adds nothing
    assert float(hyper[5]) == 1 and torch.equal(dst, src)
    # a launch of many blocks (a 512 x 512 matrix job: 64 tiles, and a 10000-element bias job: 3 blocks) adds one, not one per block
    w = torch.randn(512, 512, device=DEV)
    b = torch.randn(10000, device=DEV)
    wn = torch.empty(512, 512, device=DEV)
    bn = torch.empty(10000, device=DEV)
    table, njobs, nblocks = job_table([prep.matrix_job(ptr(w), 512, ptr(wn), 512, 0, 0, 512, 512, 0),
                                       prep.bias_job(ptr(b), 0, ptr(bn), 10000, 0)])
    assert nblocks == 67
    for dt in (0, 1):
        before = float(hyper[5])
        call("mr_prep_batch", dt, ptr(table), njobs, nblocks, ptr(hyper))
        assert float(hyper[5]) == before + 1
    assert torch.equal(bn, b)
    # ... and so does a launch of several times more blocks than the device holds at once (1024 jobs of 16 tiles over one small
    # source): while all blocks of a launch are resident together, an increment per block can hide behind every block reading the
    # counter before any of them writes it back
    w = torch.randn(64, 1024, device=DEV)
    wn = torch.empty(64, 1024, device=DEV)
    table, njobs, nblocks = job_table([prep.matrix_job(ptr(w), 1024, ptr(wn), 1024, 0, 0, 64, 1024, 0)] * 1024)
    assert nblocks == 16384
    call("mr_prep_batch", 0, ptr(table), njobs, nblocks, ptr(hyper))
    assert float(hyper[5]) == 4 and torch.equal(wn, w)
    hyper[5] = 3
    call("mr_opt_tick", ptr(hyper))
    assert float(hyper[5]) == 4
    assert hyper[:5].tolist() == [_f32(1e-3), 0, 0, 0, 0] and hyper[6:].tolist() == [0, 0]     # nothing else in the block moves


@pytest.mark.parametrize("which", ["p", "g", "state"])
def test_update_kernels_refuse_misaligned_buffers(which):
    """Both kernels read and write f32x4: a pointer 4 bytes off a 16-byte boundary is refused on the host, nothing is launched."""
    n = 64
    bufs = {k: torch.ones(n + 4, dtype=torch.float32, device=DEV) for k in ("p", "g", "m", "v")}
    hyper = torch.zeros(8, dtype=torch.float32, device=DEV)
    hyper[0] = 0.5
    off = {k: 0 for k in bufs}
    off["m" if which == "state" else which] = 4
    with pytest.raises(RuntimeError, match=r"mr_adam_step failed \(code 1\).*16-byte aligned"):
        call("mr_adam_step", ptr(bufs["p"]) + off["p"], ptr(bufs["g"]) + off["g"], ptr(bufs["m"]) + off["m"], ptr(bufs["v"]), n,
             ptr(hyper))
    with pytest.raises(RuntimeError, match=r"mr_sgd_step failed \(code 1\).*16-byte aligned"):
        call("mr_sgd_step", ptr(bufs["p"]) + off["p"], ptr(bufs["g"]) + off["g"], ptr(bufs["m"]) + off["m"], n, ptr(hyper))
    torch.cuda.synchronize()
    for t in bufs.values():
        assert bool((t == 1).all())


# ------------------------------------------------------------------ through FusedAdam / FusedSGD
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from megreader_amd.nn import Conv2d, Linear
        self.conv = Conv2d(8, 12, 3, 1, 1)
        self.fc = Linear(12, 10)
        self.unused = torch.nn.Parameter(torch.randn(37))       # never receives a gradient

    def forward(self, x):
        y = self.conv(x).float().mean((2, 3))
        return self.fc(y).float()


def _make(kind, seed, wd=None, unused=False):
    """(net, fused optimizer, [(name, float64 copy, float32 copy)], float64 torch optimizer, float32 torch optimizer): two param
    groups, the second with a quarter of the learning rate."""
    mr.set_compute_dtype(torch.float32)
    torch.manual_seed(seed)
    net = _Net().to(DEV)
    first = list(net.conv.parameters()) + ([net.unused] if unused else [])
    second = list(net.fc.parameters())
    if kind == "adam":
        kw = dict(lr=1e-2, weight_decay=1e-2 if wd is None else wd)
        fused, ref_cls, ref_kw = FusedAdam, torch.optim.Adam, {k: _f32(v) for k, v in kw.items()}
    else:
        kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4 if wd is None else wd)
        fused, ref_cls, ref_kw = FusedSGD, torch.optim.SGD, {k: _f32(v) for k, v in kw.items()}
    lr2 = kw['lr'] / 4
    opt = fused([{'params': first}, {'params': second, 'lr': lr2}], **kw)
    copies, refs = [], []
    for dt in (torch.float64, torch.float32):
        c = [[p.detach().cpu().to(dt).contiguous().requires_grad_(True) for p in grp] for grp in (first, second)]
        copies.append(c[0] + c[1])
        refs.append(ref_cls([{'params': c[0]}, {'params': c[1], 'lr': _f32(lr2)}], foreach=False, **ref_kw))
    return net, opt, first + second, copies, refs, [_f32(kw['lr'])] * len(first) + [_f32(lr2)] * len(second)


def _compare_params(track, params, copies, lrs):
    for i, (p, c64, c32, lr) in enumerate(zip(params, copies[0], copies[1], lrs)):
        track.update("p", p, c32, c64, lr)


@pytest.mark.parametrize("scale", [None, 0.5])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fused_classes_match_torch_float64(kind, scale):
    net, opt, params, copies, refs, lrs = _make(kind, 5)
    opt.zero_grad()                                                  # the parameters move into the flat buffer, then ...
    net(torch.randn(2, 8, 4, 6, device=DEV)).sum().backward()        # ... operand images exist: the refresh launch carries the tick
    opt.zero_grad()
    if scale is not None:
        opt.set_grad_scale(scale)
    g = torch.Generator().manual_seed(11)
    track = _Tracker(["p"])
    for k in range(6):
        for p, c64, c32 in zip(params, copies[0], copies[1]):
            gr = torch.randn(p.shape, generator=g) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g))
            p.grad.copy_(gr)
            c64.grad = gr.double() * (scale or 1.0)
            c32.grad = gr * (scale or 1.0)
        opt.step()
        refs[0].step()
        refs[1].step()
        _compare_params(track, params, copies, lrs)
        live = [f for f in opt._flat if f is not None]
        assert len(live) == 2 and all(float(f['hyper'][5]) == k + 1 for f in live)
    assert any('prep_plan' in f for f in opt._flat)
    track.check("Fused %s scale=%s" % (kind, scale))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fused_step_after_set_to_none_and_autograd_backward(kind):
    """zero_grad(set_to_none=True) detaches .grad; autograd then creates gradients outside the flat buffer and step() folds them
    back in.  The parameter that never receives one (weight_decay = 0) stays bit-identical, as in torch."""
    net, opt, params, copies, refs, lrs = _make(kind, 6, wd=0.0, unused=True)
    x = torch.randn(2, 8, 4, 6, device=DEV)
    unused0 = net.unused.detach().clone()
    track = _Tracker(["p"])
    for k in range(3):
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in params)
        (net(x) ** 2).sum().backward()
        assert net.unused.grad is None
        for p, c64, c32 in zip(params, copies[0], copies[1]):
            if p.grad is not None:
                c64.grad = p.grad.detach().cpu().double()
                c32.grad = p.grad.detach().cpu().clone()
            else:
                c64.grad = c32.grad = None
        opt.step()
        refs[0].step()
        refs[1].step()
        _compare_params(track, params, copies, lrs)
    assert torch.equal(net.unused.detach(), unused0)
    i = [j for j, p in enumerate(params) if p is net.unused][0]
    assert torch.equal(copies[0][i].detach().float(), unused0.cpu())
    track.check("Fused %s after set_to_none" % kind)


def test_graph_replay_matches_eight_reference_steps():
    """Three eager steps, one single-stream capture of opt.step(), five replays with new gradients in the static buffer and a new
    learning rate pushed before each: the device counter reads 8 and the parameters are those of eight float64 steps."""
    net, opt, params, copies, refs, lrs = _make("adam", 7)
    opt.zero_grad()
    net(torch.randn(2, 8, 4, 6, device=DEV)).sum().backward()       # the captured step holds an update and a refresh launch
    opt.zero_grad()
    g = torch.Generator().manual_seed(12)
    track = _Tracker(["p"])

    def feed():
        for p, c64, c32 in zip(params, copies[0], copies[1]):
            gr = torch.randn(p.shape, generator=g) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g))
            p.grad.copy_(gr)
            c64.grad, c32.grad = gr.double(), gr.clone()

    def reference_step():
        refs[0].step()
        refs[1].step()
        _compare_params(track, params, copies, lrs)

    for _ in range(3):
        feed()
        opt.step()
        reference_step()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        opt.step()                  # recorded, not run
    assert all(float(f['hyper'][5]) == 3 for f in opt._flat) and all('prep_plan' in f for f in opt._flat)
    for r in range(5):
        feed()
        for grp, r64, r32 in zip(opt.param_groups, refs[0].param_groups, refs[1].param_groups):
            grp['lr'] = grp['lr'] * 0.7
            r64['lr'] = r32['lr'] = _f32(grp['lr'])
        lrs = [_f32(opt.param_groups[0]['lr'])] * len(opt.param_groups[0]['params']) + \
              [_f32(opt.param_groups[1]['lr'])] * len(opt.param_groups[1]['params'])
        opt.push_hyper()
        graph.replay()
        torch.cuda.synchronize()
        reference_step()
    assert all(float(f['hyper'][5]) == 8 for f in opt._flat)
    track.check("graph replay")
