"""Helpers of the direct C-ABI tests (test_optim_gpu / test_prep_gpu / test_elementwise_gpu): destinations with a sentinel guard
band behind them, and mr_prep_batch job tables laid out as include/megreader_hip.h documents them."""
import torch

from megreader_amd.nn import prep

GUARD = 256          # elements behind every destination that no kernel may touch
SENTINEL = -77.0     # exactly representable in f32 and bf16; no source value of these tests equals it


def guarded(n, dtype, device="cuda", sentinel=SENTINEL):
    """(whole buffer, its first n elements): n + GUARD elements of `sentinel`; the base keeps torch's allocation alignment."""
    buf = torch.full((n + GUARD,), sentinel, dtype=dtype, device=device)
    return buf, buf[:n]


def guard_intact(buf, n, sentinel=SENTINEL):
    return bool((buf[n:] == sentinel).all()) and buf.numel() == n + GUARD


def mixed_values(shape, seed):
    """float32 normals (no denormals): a third full-precision, a third bf16-representable, a third exact bf16 round-to-even ties
    (bit 15 set, bits 0..14 clear: half of both the even and the odd neighbours)."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    x = torch.randn(n, generator=g) + torch.where(torch.rand(n, generator=g) < 0.5, 0.25, -0.25)
    bits = x.view(torch.int32)
    kind = torch.arange(n) % 3
    bits[kind >= 1] &= ~0xFFFF
    bits[kind == 2] |= 0x8000
    assert bool(torch.isfinite(x).all()) and float(x.abs().min()) > 1e-30
    return x.reshape(shape)


def _cdiv(a, b):
    return (a + b - 1) // b


def blocks_of(j):
    """Grid blocks of one job, restated from the header: conv ceil(K/64)*ceil(R*S*Cpad/64), matrix ceil(R/64)*ceil(C/64),
    bias ceil(R/4096), stem 1."""
    if j['kind'] == prep.KIND_CONV:
        return _cdiv(j['d0'], 64) * _cdiv(j['d2'] * j['d3'] * j['pad'], 64)
    if j['kind'] == prep.KIND_MATRIX:
        return _cdiv(j['d0'], 64) * _cdiv(j['d1'], 64)
    if j['kind'] == prep.KIND_BIAS:
        return _cdiv(j['d0'], 4096)
    return 1


def job_table(jobs, device="cuda"):
    """(device table, njobs, total_blocks) of a list of prep.conv_job / matrix_job / bias_job / stem_job descriptions."""
    arr = (prep.PrepJob * max(len(jobs), 1))()
    nblocks = 0
    for slot, j in zip(arr, jobs):
        for name, _ in prep.PrepJob._fields_:
            if name in j:
                setattr(slot, name, j[name])
        slot.block_start = nblocks
        nblocks += blocks_of(j)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device), len(jobs), nblocks
