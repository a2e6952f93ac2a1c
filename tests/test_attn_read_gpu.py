"""mr_attn_read at the C ABI (ops.decode.attention_read): the attention maps, their moments, the words' log-probabilities and the
string scores against the float64 restatement (tests/_attn_ref.py) on the same rounded inputs.  The bar is the one of
tests/test_ctc_beam_gpu.py and tests/test_lexicon_ctc_gpu.py: the kernel's largest error may be at most 8 x the largest error of
the float32 restatement (the kernel's own order of summation) against float64.  Shapes (N, height x width, S, C, H): the smallest
at which each branch exists -- one position and two steps; an odd grid with several step groups per image; 17 rows with H no
multiple of the 16-byte vector (the element path); the published 32 x 32 steps x 38 classes at H = 512; C = 300 > 256 classes
with T = 70 > 64 positions (more than one position and class per lane); the LDS budget: T = 4096, the most the entry point takes,
at H = 512, where the energies leave room for 2 steps per workgroup and not the 4 that S = 3 asks for (39 KiB of LDS), and H = 6000,
where the hproj rows leave room for 1 (47 KiB).  The bar compares two maxima, so a case needs more than one number of a kind:
the H = 6000 case has 8 rows (with one row its single score was compared with a restatement that happened to land 1/16 ulp from
float64: kernel 1.7e-8, under half an ulp, against 1.9e-9)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_ref as ref  # noqa: E402
from megreader_amd._lib import load  # noqa: E402
from megreader_amd.ops.decode import attention_read  # noqa: E402

DEV = "cuda"
BLANK = 0
#          N  h   w   S   C    H
SHAPES = [(1, 1, 1, 2, 3, 8),
          (5, 3, 11, 9, 11, 72),
          (17, 1, 20, 7, 5, 37),
          (16, 1, 32, 32, 38, 512),
          (3, 2, 35, 5, 300, 64),
          (1, 64, 64, 3, 5, 512),
          (8, 1, 64, 2, 3, 6000)]
CASES = [(s, torch.bfloat16) for s in SHAPES] + [(s, torch.float32) for s in SHAPES[:3]]
GUARD = 12345.0
_CACHE = {}


def _inputs(shape, dtype):
    N, h, w, S, C, H = shape
    g = torch.Generator().manual_seed(1000 + N * 7 + C)
    T = h * w
    r = lambda *s: torch.randn(*s, generator=g)                           # noqa: E731
    d = dict(hproj=(r(S, N, H) * 0.8).to(dtype), eproj=(r(N, T, H) * 0.8).to(dtype), v=r(H) * 6.0 * H ** -0.5,
             logits=(r(S, N, C) * 3.0).to(dtype), words=torch.randint(0, C, (N, S), generator=g).to(torch.int32))
    d["words"][0, S - 1] = BLANK                  # a row whose string ends in the last step
    if N > 1:
        d["words"][1] = 1 + d["words"][1] % (C - 1)   # a row without a blank
    return d


def _case(shape, dtype):
    """(inputs, kernel outputs with att, kernel outputs without, float64 and float32 restatements), computed once."""
    key = (shape, dtype)
    if key not in _CACHE:
        N, h, w, S, C, H = shape
        d = _inputs(shape, dtype)
        on = {k: v.to(DEV) for k, v in d.items()}
        with_att = attention_read(on["hproj"], on["eproj"], on["v"], on["logits"], on["words"], BLANK, h, w, attention=True)
        without = attention_read(on["hproj"], on["eproj"], on["v"], on["logits"], on["words"], BLANK, h, w)
        torch.cuda.synchronize()
        host = {k: v.double().numpy() if v.is_floating_point() else v.numpy() for k, v in d.items()}
        args = (host["hproj"], host["eproj"], host["v"].astype(np.float32).astype(np.float64), host["logits"], host["words"],
                BLANK, h, w)
        vec = 8 if dtype == torch.bfloat16 else 4
        _CACHE[key] = (d, {k: v.cpu().numpy() for k, v in with_att.items()}, {k: v.cpu().numpy() for k, v in without.items()},
                       ref.replay_read(*args, dtype=np.float64), ref.replay_read(*args, dtype=np.float32, vec=vec))
    return _CACHE[key]


def _err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (a == b)                                                      # (equal infinities are no error)
    with np.errstate(invalid='ignore'):
        return float(np.where(same, 0.0, np.abs(a - b)).max())


@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_maps_moments_and_scores_against_float64(shape, dtype):
    _, got, _, f64, f32 = _case(shape, dtype)
    for key in ("att", "sym_lp", "moments", "score"):
        e32, ek = _err(f32[key], f64[key]), _err(got[key], f64[key])
        print("%s %s %-8s kernel %.3e  f32 restatement %.3e  ratio %.2f" % (shape, dtype, key, ek, e32, ek / e32 if e32 else 0.0))
        assert np.isfinite(got[key]).all()
        assert ek <= 8.0 * e32, (key, ek, e32)
    rows = got["att"].astype(np.float64).sum(-1)
    bar = 8.0 * _err(f32["att"].astype(np.float64).sum(-1), 1.0)
    assert _err(rows, 1.0) <= bar, (_err(rows, 1.0), bar)
    assert np.array_equal(got["length"], f64["length"])


@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_without_the_maps_the_rest_is_bit_equal(shape, dtype):
    _, got, bare, _, _ = _case(shape, dtype)
    assert "att" not in bare
    for key in ("sym_lp", "moments", "length", "score"):
        assert got[key].tobytes() == bare[key].tobytes(), key


def _raw(d, shape, out, att=True, blank=BLANK, **over):
    """The entry point itself on caller-owned buffers (`out`: name -> tensor)."""
    N, h, w, S, C, H = shape
    a = dict(N=N, S=S, T=h * w, H=H, C=C, height=h, width=w, ldh=H, ldl=C, ldp=S)
    a.update(over)
    code = a.pop("code", 1 if d["eproj"].dtype == torch.bfloat16 else 0)
    p = lambda t: 0 if t is None else t.data_ptr()                        # noqa: E731
    return load().mr_attn_read(code, p(d["hproj"]), a["ldh"], p(d["eproj"]), p(d["v"]), p(d["logits"]), a["ldl"], p(d["words"]),
                               a["ldp"], blank, a["N"], a["S"], a["T"], a["H"], a["C"], a["height"], a["width"],
                               p(out["att"]) if att else 0, p(out["sym_lp"]), p(out["moments"]), p(out["length"]),
                               p(out["score"]), torch.cuda.current_stream().cuda_stream)


def _guarded(shape, pad=64):
    N, h, w, S, C, H = shape
    sizes = dict(att=N * S * h * w, sym_lp=N * S, moments=N * S * 4, length=N, score=N)
    full = {k: (torch.full((n + pad,), int(GUARD), dtype=torch.int32, device=DEV) if k == "length"
                else torch.full((n + pad,), GUARD, dtype=torch.float32, device=DEV)) for k, n in sizes.items()}
    return full, sizes


@pytest.mark.parametrize("shape,dtype", [CASES[1], CASES[4], CASES[6]], ids=lambda v: str(v).replace("torch.", ""))
def test_guards_behind_every_output_are_intact(shape, dtype):
    d, got, _, _, _ = _case(shape, dtype)
    on = {k: v.to(DEV) for k, v in d.items()}
    full, sizes = _guarded(shape)
    assert _raw(on, shape, full) == 0
    torch.cuda.synchronize()
    for key, n in sizes.items():
        assert bool((full[key][n:] == GUARD).all()), key
        assert full[key][:n].cpu().numpy().tobytes() == got[key].tobytes(), key


def test_a_refused_shape_launches_nothing():
    shape, dtype = CASES[1]
    d, _, _, _, _ = _case(shape, dtype)
    on = {k: v.to(DEV) for k, v in d.items()}
    N, h, w, S, C, H = shape
    bad = [dict(T=4097, height=1, width=4097), dict(height=h + 1), dict(S=0), dict(H=0), dict(C=0), dict(ldh=H - 1),
           dict(ldl=C - 1), dict(ldp=S - 1), dict(T=4096, height=64, width=64, H=8000, ldh=8000)]
    for over in bad + [dict(blank=C), dict(blank=-1)]:
        full, sizes = _guarded(shape)
        blank = over.pop("blank", BLANK)
        assert _raw(on, shape, full, blank=blank, **over) == 1, over                   # MR_ERR_ARG
        assert load().mr_last_error().decode().startswith("mr_attn_read:")
        torch.cuda.synchronize()
        assert all(bool((t == GUARD).all()) for t in full.values()), over
    full, _ = _guarded(shape)
    assert _raw(on, shape, full, code=7) == 2                                          # MR_ERR_DTYPE
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in full.values())
    full["sym_lp"] = None
    assert _raw(on, shape, full) == 1 and "null" in load().mr_last_error().decode()
