"""mr_decode_greedy_fwd / mr_decode_greedy_trim (csrc/decode_persist.hip): the eval loop of the reference
(decoders/attention_decoder.py:84-118: arg-max feedback from a start word, early stop) as ONE persistent launch plus a trim.

  * the words are the arg-max of the kernel's OWN hidden states (first index on ties), for every step including the last;
  * the states equal the per-step launches (mr_gemm_nt + mr_attn_fwd2 + mr_gemm_gru_fwd) fed the kernel's words, or the float64
    recurrence beyond 32 rows;
  * the product configuration (no H_all) gives the same words, run to run and for either way of zeroing the workspace;
  * the shape gate; the trim against a torch restatement.

Inputs: the recipe of tests/test_decode_persist_gpu.py (_inputs / _coin_inputs), restated.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd._lib import call, dtype_code, load, ptr, set_tuning  # noqa: E402

DEV = "cuda"
H = 512
BF = torch.bfloat16

#          N   T   Ep   S   C
SHAPES = [(16, 64, 552, 32, 38),     # published
          (32, 64, 552, 12, 38),     # full grid, groups of 4 rows
          (5, 33, 64, 9, 11),        # ragged
          (17, 20, 8, 7, 5),         # ragged
          (3, 9, 16, 6, 256),        # C at the limit
          (40, 64, 552, 5, 97),      # groups of 8 rows
          (64, 37, 576, 4, 7),       # groups of 8 rows
          (16, 64, 552, 1, 38),      # S = 1: the tail only
          (1, 1, 16, 2, 3)]          # N = T = 1, S = 2


def _inputs(N, T, Ep, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    d = {}
    d["cat_w"] = (torch.randn(4 * H, H, generator=g) * H ** -0.5).to(BF)
    d["cat_b"] = torch.cat([torch.zeros(H), torch.randn(3 * H, generator=g) * 0.1]).float()
    d["ic_w"] = (torch.randn(3 * H, Ep, generator=g) * Ep ** -0.5).to(BF)
    d["G"] = (torch.randn(C, 3 * H, generator=g) * 0.5).to(BF)
    d["idx"] = torch.randint(0, C, (S, N), generator=g, dtype=torch.int64)
    d["eproj"] = (torch.randn(N, T, H, generator=g) * 0.7).to(BF)
    d["enc"] = torch.randn(N, T, Ep, generator=g).to(BF)
    d["v"] = (torch.randn(H, generator=g) * H ** -0.5 * 4).float()
    d["h0"] = (torch.randn(N, H, generator=g) * 0.3).to(BF)
    g = torch.Generator().manual_seed(S)
    d["out_w"] = (torch.randn(C, H, generator=g) * H ** -0.5 * 3).to(BF)
    d["out_b"] = (torch.randn(C, generator=g) * 0.2).float()
    del d["idx"]                                     # the greedy form reads no words
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def _greedy(d, N, T, Ep, S, C, start, with_h=True, prezero=True, ldp=None):
    """(pred [N, S] int32, H_all or None, status word)"""
    ldp = S if ldp is None else ldp
    pred = torch.full((N, ldp), -7, dtype=torch.int32, device=DEV)
    H_all = torch.full((S + 1, N, H), float("nan"), dtype=BF, device=DEV) if with_h else None
    nbytes = load().mr_decode_persist_ws_bytes(N)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV) if prezero else \
        torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    call("mr_decode_greedy_fwd", ptr(d["cat_w"]), ptr(d["cat_b"]), ptr(d["ic_w"]), Ep, ptr(d["G"]), 3 * H, ptr(d["out_w"]),
         ptr(d["out_b"]), C, ptr(d["eproj"]), ptr(d["enc"]), ptr(d["v"]), ptr(d["h0"]), start, ptr(pred), ldp, ptr(H_all), ptr(ws),
         -nbytes if prezero else nbytes, S, N, T, Ep)
    torch.cuda.synchronize()
    status = int(ws[nbytes - 256:nbytes - 252].view(torch.int32).item())
    return pred, H_all, status


@functools.lru_cache(maxsize=None)
def _run(shape):
    """One launch per shape, shared (read-only) by the tests below."""
    N, T, Ep, S, C = shape
    assert load().mr_decode_greedy_ok(dtype_code(BF), N, T, H, Ep, C) == 1
    d = _inputs(N, T, Ep, S, C, seed=N * 5 + S)
    pred, H_all, status = _greedy(d, N, T, Ep, S, C, start=C - 1)
    return d, pred, H_all, status


def _fed_words(pred, start):
    """idx [S][N] of a teacher-forced replay: the start word, then the kernel's own words."""
    S = pred.shape[1]
    first = torch.full((1, pred.shape[0]), start, dtype=torch.int64, device=DEV)
    return torch.cat((first, pred.t()[:S - 1].long()), 0).contiguous()


def _per_step(d, idx, N, T, Ep, S):
    dt = dtype_code(BF)
    H_all = torch.full((S + 1, N, H), float("nan"), dtype=BF, device=DEV)
    H_all[0].copy_(d["h0"])
    HC = 4 * H
    hc = torch.empty((N, HC), dtype=BF, device=DEV)
    w = torch.empty((N, T), dtype=torch.float32, device=DEV)
    ctx = torch.empty((N, Ep), dtype=BF, device=DEV)
    save = torch.empty((N, 3 * H), dtype=torch.float32, device=DEV)
    for s in range(S):
        call("mr_gemm_nt", dt, ptr(H_all[s]), H, ptr(d["cat_w"]), H, ptr(hc), HC, ptr(d["cat_b"]), 0, N, HC, H)
        call("mr_attn_fwd2", dt, ptr(hc), HC, ptr(d["eproj"]), ptr(d["v"]), ptr(d["enc"]), ptr(w), ptr(ctx), N, T, H, Ep)
        call("mr_gemm_gru_fwd", dt, ptr(ctx), Ep, ptr(d["ic_w"]), Ep, ptr(d["G"]), 3 * H, ptr(idx[s]), ptr(hc) + H * 2, HC,
             ptr(H_all[s]), ptr(H_all[s + 1]), ptr(save), N, H, Ep)
    return H_all


def _f64(d, idx, N, T, Ep, S):
    """The recurrence in float64 on the same (bf16-valued) inputs; no intermediate rounding."""
    f = {k: v.double() for k, v in d.items()}
    h = f["h0"]
    out = [h]
    for s in range(S):
        hc = h @ f["cat_w"].t() + f["cat_b"]
        hproj, gh = hc[:, :H], hc[:, H:]
        w = torch.softmax(torch.tanh(hproj.unsqueeze(1) + f["eproj"]) @ f["v"], dim=1)
        ctx = torch.bmm(w.unsqueeze(1), f["enc"]).squeeze(1)
        gi = f["G"][idx[s]] + ctx @ f["ic_w"].t()
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out)


@pytest.mark.parametrize("shape", SHAPES)
def test_words_are_the_argmax_of_the_kernels_own_states(shape):
    N, T, Ep, S, C = shape
    d, pred, H_all, status = _run(shape)
    assert status == 0, "a hand-off of the greedy decode kernel timed out (code %d)" % status
    assert pred.shape == (N, S) and int(pred.min()) >= 0 and int(pred.max()) < C          # every step, the last included
    assert torch.isfinite(H_all.float()).all() and torch.equal(H_all[0], d["h0"])
    logits = H_all[1:].float() @ d["out_w"].float().t() + d["out_b"]                     # [S, N, C]
    am = logits.argmax(-1).t()                                                            # [N, S]
    if C > 1:
        top2 = logits.topk(2, dim=-1).values
        clear = ((top2[..., 0] - top2[..., 1]) > 1e-3).t()
    else:
        clear = torch.ones_like(am, dtype=torch.bool)
    close = 1.0 - float(clear.double().mean())
    print("shape %s: %.3f %% of the positions under the 1e-3 margin" % (shape, 100 * close))
    assert torch.equal(pred.long()[clear], am[clear])
    assert close <= 0.02


@pytest.mark.parametrize("C,period", [(12, 2), (8, 4), (24, 8)])
def test_first_index_wins_ties(C, period):
    """Classes that are copies of one another: within a lane's four classes (rows 2k and 2k + 1 identical), across the two lanes
    of a slice (row c + 4 = row c) and across slices (rows c + 8, c + 16 = row c).  Only the first copy may ever be predicted."""
    N, T, Ep, S = 6, 20, 16, 8
    d = _inputs(N, T, Ep, S, C, seed=77 + C)
    if period == 2:
        first = torch.arange(C, device=DEV) // 2 * 2
    else:
        first = torch.arange(C, device=DEV) % period
    d["out_w"] = d["out_w"][first].contiguous()
    d["out_b"] = d["out_b"][first].contiguous()
    pred, _, status = _greedy(d, N, T, Ep, S, C, start=C - 1)
    assert status == 0
    assert int(pred.min()) >= 0
    if period == 2:
        assert bool((pred % 2 == 0).all()), pred
    else:
        assert int(pred.max()) < period, pred
    assert len(pred.unique()) > 1                   # (not a constant answer)


@pytest.mark.parametrize("shape", SHAPES)
def test_states_match_the_launches_fed_the_same_words(shape):
    N, T, Ep, S, C = shape
    d, pred, H_all, status = _run(shape)
    assert status == 0
    idx = _fed_words(pred, C - 1)
    a = H_all.double()
    if N <= 32:
        b = _per_step(d, idx, N, T, Ep, S).double()
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 3e-2 * scale
        assert float(((a - b).abs() > 4e-3 * scale).double().mean()) < 0.02
    else:
        b = _f64(d, idx, N, T, Ep, S)
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 3e-2 * scale


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[5], SHAPES[7]])
def test_product_configuration_gives_the_same_words(shape):
    N, T, Ep, S, C = shape
    d, pred, _, _ = _run(shape)
    for with_h, prezero in ((False, True), (False, True), (False, False), (True, False)):
        got, _, status = _greedy(d, N, T, Ep, S, C, start=C - 1, with_h=with_h, prezero=prezero)
        assert status == 0
        assert torch.equal(got, pred), (with_h, prezero)
    # a wider pred: only the S used columns of a row are written
    got, _, status = _greedy(d, N, T, Ep, S, C, start=C - 1, with_h=False, ldp=S + 3)
    assert status == 0 and torch.equal(got[:, :S], pred) and bool((got[:, S:] == -7).all())


def test_shape_gate():
    lib = load()
    bf = dtype_code(BF)
    N, T, Ep, S, C = 16, 64, 552, 4, 38
    assert lib.mr_decode_greedy_ok(bf, N, T, H, Ep, C) == 1
    assert lib.mr_decode_greedy_ok(bf, N, T, H, Ep, 256) == 1
    assert lib.mr_decode_greedy_ok(bf, N, T, H, Ep, 257) == 0
    assert lib.mr_decode_greedy_ok(bf, N, T, H, Ep, 0) == 0
    assert lib.mr_decode_greedy_ok(dtype_code(torch.float32), N, T, H, Ep, C) == 0
    assert lib.mr_decode_greedy_ok(bf, N, T, 256, Ep, C) == 0
    assert lib.mr_decode_greedy_ok(bf, N, 65, H, Ep, C) == 0
    assert lib.mr_decode_greedy_ok(bf, N, T, H, 584, C) == 0
    assert lib.mr_decode_greedy_ok(bf, 65, T, H, Ep, C) == 0
    set_tuning(decode_persist=0)
    try:
        assert lib.mr_decode_greedy_ok(bf, N, T, H, Ep, C) == 0
    finally:
        set_tuning(decode_persist=1)
    assert lib.mr_decode_greedy_ok(bf, N, T, H, Ep, C) == 1
    # the launch refuses what the query refuses, before anything runs: pred and the workspace stay as they were
    d = _inputs(N, T, Ep, S, 257, seed=3)
    pred = torch.full((N, S), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.mr_decode_persist_ws_bytes(N)
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="mr_decode_greedy_fwd"):
        call("mr_decode_greedy_fwd", ptr(d["cat_w"]), ptr(d["cat_b"]), ptr(d["ic_w"]), Ep, ptr(d["G"]), 3 * H, ptr(d["out_w"]),
             ptr(d["out_b"]), 257, ptr(d["eproj"]), ptr(d["enc"]), ptr(d["v"]), ptr(d["h0"]), 0, ptr(pred), S, 0, ptr(ws), nbytes,
             S, N, T, Ep)
    torch.cuda.synchronize()
    assert bool((pred == -7).all()) and bool((ws == 0xAB).all())


# ------------------------------------------------------------------------------------------------------------------ the trim
def _trim_ref(pred, S, blank):
    out = pred.clone()
    hit = (pred[:, :S] == blank).all(0).nonzero()
    if hit.numel():
        out[:, int(hit[0]) + 1:S] = blank
    return out


def _trim_cases():
    g = torch.Generator().manual_seed(9)
    blank = 3
    cases = {}

    def rnd(N, ld):
        p = torch.randint(0, 9, (N, ld), generator=g, dtype=torch.int32)
        p[0] = torch.where(p[0] == blank, torch.full_like(p[0], 5), p[0])       # no accidental all-blank column
        return p
    cases["none"] = (rnd(7, 12), 12)
    p = rnd(7, 12); p[:, 0] = blank; cases["column 0"] = (p, 12)
    p = rnd(7, 12); p[:, 11] = blank; cases["last column"] = (p, 12)
    p = rnd(7, 12); p[:, 2] = blank; p[4, 2] = 6; p[:, 7] = blank; cases["all rows but one, then a true one"] = (p, 12)
    p = rnd(7, 12); p[:, 5] = blank; p[2, 1] = -1; p[3, 8:] = -1; cases["-1 entries"] = (p, 12)
    p = rnd(7, 12); p[:, 5] = blank; p[:, 6] = -1; p[0, 6] = 5; cases["a column of -1 is not blank"] = (p, 12)
    p = rnd(7, 20); p[:, 4] = blank; p[:, 15] = blank; cases["ldp > S"] = (p, 12)
    p = rnd(1, 32); p[0, 9] = blank; cases["N = 1"] = (p, 32)
    p = rnd(300, 32); p[:, 17] = blank; p[:, 30] = blank; cases["N = 300"] = (p, 32)
    p = rnd(300, 32); p[:, 17] = blank; p[299, 17] = 1; cases["N = 300, last row differs"] = (p, 32)
    p = rnd(5, 1); cases["S = 1"] = (p, 1)
    return blank, cases


def test_trim_matches_the_reference_loop():
    blank, cases = _trim_cases()
    for name, (p, S) in cases.items():
        ref = _trim_ref(p, S, blank)
        got = p.to(DEV)
        call("mr_decode_greedy_trim", ptr(got), got.stride(0), got.shape[0], S, blank)
        assert torch.equal(got.cpu(), ref), name
    changed = sum(int(not torch.equal(_trim_ref(p, S, blank), p)) for p, S in cases.values())
    assert changed >= 5                             # the cases do exercise the overwrite
