"""Compute-dtype weight images (mr_prep_conv_weight / mr_prep_matrix / mr_prep_bias / mr_stem_pack and mr_prep_batch,
csrc/elementwise.hip) against plain torch indexing of the float32 source on the CPU followed by `.to(dtype)`.

Every image is a copy with at most one rounding, so equality is exact.  Destinations are pre-filled with a sentinel and followed
by a guard band; the expected image keeps the sentinel wherever the contract leaves elements unwritten (columns K..ldk-1 of the
CRSK image, C..ldn-1 and R..ldt-1 of the matrix images)."""
import random
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr, vec_of  # noqa: E402
from megreader_amd.nn import prep  # noqa: E402
from megreader_amd.optim import FusedAdam  # noqa: E402

from _abi_util import SENTINEL, guard_intact, guarded, job_table, mixed_values as _values  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
LAYOUTS = ["contiguous", "channels_last", "sliced"]

# K, C, R, S, Cpad, ldk
CONV_CASES = [(20, 16, 3, 2, 16, 24),       # partial tile, scalar transposed path
              (64, 8, 3, 3, 8, 64),         # exactly one full tile, vector path
              (130, 24, 1, 1, 24, 136),     # three row tiles, the last of two rows
              (72, 40, 3, 3, 40, 72),       # six column tiles, 64 no multiple of Cpad, last one partial
              (66, 8, 1, 1, 8, 66)]         # a full row tile, but ldk no multiple of the 16-byte vector
# R, C, perm_h, lds, ldn, ldt
MATRIX_CASES = [(32, 16, 8, 16, 16, 32),
                (1024, 512, 256, 512, 512, 1024),
                (2048, 256, 256, 256, 256, 2048),     # two gate blocks
                (40, 38, 0, 44, 38, 40),              # source rows wider than C
                (200, 70, 0, 70, 72, 208)]
# R, perm_h, second source
BIAS_CASES = [(1024, 256, True), (2048, 256, True), (5000, 0, False)]
STEM_CASES = [(1, "contiguous"), (3, "contiguous"), (1, "channels_last"), (3, "channels_last")]


@pytest.fixture(autouse=True)
def _reset_dtype():
    yield
    mr.set_compute_dtype(torch.bfloat16)


def _perm(R, perm_h):
    """Destination row of every source row: r = q*H + j -> 4*j + q inside each block of 4*H rows."""
    r = torch.arange(R)
    if perm_h == 0:
        return r
    h4 = 4 * perm_h
    blk, rin = r // h4, r % h4
    return blk * h4 + 4 * (rin % perm_h) + rin // perm_h


class _Image(object):
    """One destination: guarded device buffer + the expected contents."""

    def __init__(self, expect):
        self.expect = expect.contiguous()
        self.n = expect.numel()
        self.whole, self.view = guarded(self.n, expect.dtype)

    def reset(self):
        self.whole.fill_(SENTINEL)

    def check(self, what):
        assert torch.equal(self.view.cpu(), self.expect.reshape(-1)), what
        assert guard_intact(self.whole, self.n), what


class _Case(object):
    def __init__(self, name, jobs, images, keep):
        self.name, self.jobs, self.images, self.keep = name, jobs, images, keep

    def reset(self):
        for im in self.images:
            im.reset()

    def check(self, how):
        for i, im in enumerate(self.images):
            im.check("%s image %d (%s)" % (self.name, i, how))


def _layout(w, layout, seed):
    """Device tensor with the values of w [K,C,R,S] in the given source layout."""
    if layout == "contiguous":
        return w.to(DEV)
    if layout == "channels_last":
        return w.to(DEV).contiguous(memory_format=torch.channels_last)
    K, C, R, S = w.shape
    big = _values((K, C + 3, R, S), seed + 1).to(DEV)
    big[:, 1:1 + C] = w.to(DEV)
    return big[:, 1:1 + C]


def _conv_case(dtype, K, C, R, S, Cpad, ldk, layout, crsk=True, seed=0):
    w = _values((K, C, R, S), seed)
    src = _layout(w, layout, seed)
    assert torch.equal(src.cpu(), w)
    krsc = torch.zeros(K, R, S, Cpad)
    krsc[..., :C] = w.permute(0, 2, 3, 1)
    images = [_Image(krsc.to(dtype))]
    if crsk:
        t = torch.full((C, R, S, ldk), SENTINEL)
        t[..., :K] = w.permute(1, 2, 3, 0)
        images.append(_Image(t.to(dtype)))
    job = prep.conv_job(ptr(src), src.stride(), ptr(images[0].view), ptr(images[1].view) if crsk else 0, K, C, R, S, Cpad, ldk)
    return _Case("conv %s %s" % ((K, C, R, S, Cpad, ldk), layout), [job], images, [src])


def _matrix_case(dtype, R, C, perm_h, lds, ldn, ldt, seed=0):
    wide = _values((R, lds), seed)
    src = wide.to(DEV)
    rp = _perm(R, perm_h)
    n = torch.full((R, ldn), SENTINEL)
    n[rp, :C] = wide[:, :C]
    t = torch.full((C, ldt), SENTINEL)
    t[:, rp] = wide[:, :C].t()
    images = [_Image(n.to(dtype)), _Image(t.to(dtype))]
    job = prep.matrix_job(ptr(src), lds, ptr(images[0].view), ldn, ptr(images[1].view), ldt, R, C, perm_h)
    return _Case("matrix %s" % ((R, C, perm_h, lds, ldn, ldt),), [job], images, [src])


def _bias_case(R, perm_h, two, seed=0):
    a = _values((R,), seed)
    b = _values((R,), seed + 1) if two else None
    out = torch.empty(R)
    out[_perm(R, perm_h)] = a + b if two else a
    ad, bd = a.to(DEV), (b.to(DEV) if two else None)
    images = [_Image(out)]
    return _Case("bias %s" % ((R, perm_h, two),), [prep.bias_job(ptr(ad), ptr(bd), ptr(images[0].view), R, perm_h)], images, [ad, bd])


def _stem_case(dtype, cin, layout, seed=0):
    w = _values((64, cin, 3, 3), seed)
    src = _layout(w, layout, seed)
    pack = torch.zeros(64, 32)
    for dr in range(3):
        for ds in range(3):
            for c in range(cin):
                pack[:, (dr * 3 + ds) * cin + c] = w[:, c, dr, ds]
    images = [_Image(pack.to(dtype))]
    return _Case("stem %d %s" % (cin, layout), [prep.stem_job(ptr(src), src.stride(), ptr(images[0].view), cin)], images, [src])


def _run_individual(dtype, case):
    case.reset()
    for j in case.jobs:
        prep.run_job(dtype_code(dtype), j)
    case.check("individual entry point")


def _run_batch(dtype, cases, jobs=None, tick=None):
    for c in cases:
        c.reset()
    jobs = [j for c in cases for j in c.jobs] if jobs is None else jobs
    table, njobs, nblocks = job_table(jobs)
    call("mr_prep_batch", dtype_code(dtype), ptr(table), njobs, nblocks, ptr(tick))
    for c in cases:
        c.check("mr_prep_batch, %d jobs" % njobs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K,C,R,S,Cpad,ldk", CONV_CASES)
def test_conv_images(K, C, R, S, Cpad, ldk, layout, dtype):
    case = _conv_case(dtype, K, C, R, S, Cpad, ldk, layout, seed=K + C)
    _run_individual(dtype, case)
    _run_batch(dtype, [case])          # a single-job table


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_conv_krsc_only_with_three_channels_padded_to_one_vector(layout, dtype):
    case = _conv_case(dtype, 70, 3, 3, 3, vec_of(dtype), 70, layout, crsk=False, seed=3)
    _run_individual(dtype, case)
    _run_batch(dtype, [case])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,C,perm_h,lds,ldn,ldt", MATRIX_CASES)
def test_matrix_images(R, C, perm_h, lds, ldn, ldt, dtype):
    case = _matrix_case(dtype, R, C, perm_h, lds, ldn, ldt, seed=R + C)
    _run_individual(dtype, case)
    _run_batch(dtype, [case])


@pytest.mark.parametrize("R,perm_h,two", BIAS_CASES)
def test_bias_images(R, perm_h, two):
    case = _bias_case(R, perm_h, two, seed=R)
    _run_individual(torch.float32, case)
    for dtype in DTYPES:               # the bias image is float32 whatever the launch's dtype
        _run_batch(dtype, [case])


@pytest.mark.parametrize("cin,layout", STEM_CASES)
def test_stem_pack(cin, layout):
    case = _stem_case(torch.bfloat16, cin, layout, seed=cin)
    _run_individual(torch.bfloat16, case)       # mr_stem_pack writes bf16 only
    _run_batch(torch.bfloat16, [case])
    _run_batch(torch.float32, [_stem_case(torch.float32, cin, layout, seed=cin)])


def _all_cases(dtype):
    cases = []
    for i, (K, C, R, S, Cpad, ldk) in enumerate(CONV_CASES):
        cases.append(_conv_case(dtype, K, C, R, S, Cpad, ldk, LAYOUTS[i % 3], seed=50 + i))
    cases.append(_conv_case(dtype, 70, 3, 3, 3, vec_of(dtype), 70, "channels_last", crsk=False, seed=60))
    cases += [_matrix_case(dtype, *m, seed=70 + i) for i, m in enumerate(MATRIX_CASES)]
    cases += [_bias_case(*b, seed=80 + i) for i, b in enumerate(BIAS_CASES)]
    cases += [_stem_case(dtype, cin, layout, seed=90 + i) for i, (cin, layout) in enumerate(STEM_CASES)]
    return cases


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_every_case_in_one_launch_in_shuffled_order(dtype):
    cases = _all_cases(dtype)
    random.Random(7).shuffle(cases)
    hyper = torch.zeros(8, dtype=torch.float32, device=DEV)
    _run_batch(dtype, cases, tick=hyper)
    assert hyper.tolist() == [0, 0, 0, 0, 0, 1, 0, 0]          # hundreds of blocks, one tick


def _small_bias_jobs(count, seed):
    a = _values((count, 4), seed).to(DEV)
    b = _values((count, 4), seed + 1).to(DEV)
    image = _Image(a.cpu() + b.cpu())
    jobs = [prep.bias_job(ptr(a) + 16 * i, ptr(b) + 16 * i, ptr(image.view) + 16 * i, 4, 0) for i in range(count)]
    return _Case("%d four-element bias jobs" % count, jobs, [image], [a, b])


def test_job_limit():
    case = _small_bias_jobs(1025, 5)
    im = case.images[0]
    im.expect[1024:] = SENTINEL                                    # the job behind the limit is never part of a launch
    for dtype in DTYPES:
        _run_batch(dtype, [case], jobs=case.jobs[:1024])           # 1024 jobs: the whole table the kernel can hold
    case.reset()
    table, njobs, nblocks = job_table(case.jobs)
    assert njobs == 1025
    with pytest.raises(RuntimeError, match=r"mr_prep_batch failed \(code 1\).*at most 1024 jobs"):
        call("mr_prep_batch", 0, ptr(table), njobs, nblocks, 0)
    torch.cuda.synchronize()
    assert bool((im.whole == SENTINEL).all())                      # refused on the host: nothing was written


def test_plan_over_more_than_max_jobs_launches_twice_and_ticks_once():
    case = _small_bias_jobs(prep.MAX_JOBS + 10, 6)
    entries = [types.SimpleNamespace(dtype=torch.float32, jobs=case.jobs[:700]),
               types.SimpleNamespace(dtype=torch.float32, jobs=case.jobs[700:])]
    plan = prep._Plan(entries, torch.device(DEV))
    assert [(t[2], t[3]) for t in plan.tables] == [(prep.MAX_JOBS, prep.MAX_JOBS), (10, 10)]
    hyper = torch.zeros(8, dtype=torch.float32, device=DEV)
    case.reset()
    plan.launch(tick=hyper)
    case.check("prep._Plan, two launches")
    assert float(hyper[5]) == 1
    plan.launch(tick=None)
    assert float(hyper[5]) == 1


# ------------------------------------------------------------------ refresh after a real update
def _expected_entry(key, params, buffers, dtype):
    """The images of one prep-cache entry, from the CURRENT master parameters by torch indexing (padding = the zeros the buffers
    were allocated with)."""
    cpu = [None if p is None else p.detach().cpu().float() for p in params]
    if key[0] == "conv":
        w, b = cpu
        K, C, R, S = w.shape
        krsc = torch.zeros(buffers[0].shape)
        krsc[:K, :, :, :C] = w.permute(0, 2, 3, 1)
        out = [krsc.to(dtype)]
        if buffers[1] is not None:
            crsk = torch.zeros(buffers[1].shape)
            crsk[..., :K] = w.permute(1, 2, 3, 0)
            out.append(crsk.to(dtype))
        else:
            out.append(None)
        if buffers[2] is not None:
            bp = torch.zeros(buffers[2].shape)
            bp[:K] = b
            out.append(bp)
        else:
            out.append(None)
        return out
    if key[0] == "linear":
        w, = cpu
        t = torch.zeros(buffers[1].shape)
        t[:, :w.shape[0]] = w.t()
        return [w.to(dtype), t.to(dtype)]
    assert key[0] == "bilstm"
    H = cpu[1].shape[1]
    rp = _perm(4 * H, H)
    wcat = torch.empty(buffers[0].shape)
    whh = torch.empty(buffers[2].shape)
    bcat = torch.empty(buffers[4].shape)
    for d in range(2):
        wi, wh, bi, bh = cpu[4 * d:4 * d + 4]
        wcat[d * 4 * H + rp] = wi
        whh[d][rp] = wh
        bcat[d * 4 * H + rp] = bi + bh
    return [wcat.to(dtype), wcat.t().contiguous().to(dtype), whh.to(dtype), whh.transpose(1, 2).contiguous().to(dtype), bcat]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_refreshed_images_follow_a_real_update(dtype):
    """Three FusedAdam(lr=1e-2) steps, then every cached image must be the torch-indexing image of the parameters as they are NOW
    (a refresh that went stale, or read the wrong rows, would reproduce an old or a shuffled image)."""
    mr.set_compute_dtype(dtype)
    torch.manual_seed(2)
    from megreader_amd.nn import Conv2d, Linear, LSTM

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = Conv2d(8, 16, 3, 1, 1)
            self.c2 = Conv2d(16, 132, (3, 2), 1, (1, 0))     # three row tiles; 132 -> 136 padded output channels in bf16
            self.rnn = LSTM(32, 32, bidirectional=True)
            self.fc = Linear(64, 10)

        def forward(self, x):
            y = self.c2(self.c1(x))[:, :32]           # [N,32,H,W-1]
            seq = y.float().mean(2).permute(2, 0, 1)  # [T,N,32]
            out, _ = self.rnn(seq)
            return self.fc(out).float().sum()

    net = Net().to(DEV)
    before = [p.detach().clone() for p in net.parameters()]
    opt = FusedAdam(net.parameters(), lr=1e-2)
    x = torch.randn(2, 8, 4, 9, device=DEV, requires_grad=True)
    for _ in range(3):
        opt.zero_grad()
        net(x).backward()
        opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))
    seen = set()
    for p in net.parameters():
        for (key, dt), e in p.__dict__.get("_mr_prep", {}).items():
            assert dt == dtype
            seen.add(key[0])
            expect = _expected_entry(key, e.params, e.buffers, dtype)
            assert len(expect) == len(e.buffers)
            for i, (want, got) in enumerate(zip(expect, e.buffers)):
                assert (want is None) == (got is None)
                if want is not None:
                    assert torch.equal(got.cpu(), want), (key, i)
    assert seen == {"conv", "linear", "bilstm"}
