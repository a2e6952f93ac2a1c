"""mr_ctc2d_marginal and mr_ctc2d_char_rows (csrc/ctc2d_read.hip), `ctc2d_marginal` and `ctc2d_char_rows` against the numpy
restatement (tests/_ctc2d_read_ref.py).

The arithmetic of both kernels is fixed to the bit (every product rounded to f32, the reduction in ascending h, the log taken in
f64 and rounded once; integer outputs), so the bar is EQUALITY with the float32 restatement, whatever the layout of the inputs.
The C entry points are called with their outputs inside buffers pre-filled with garbage: equality shows that everything was
written, the cells around the outputs that nothing else was.  Only the comparison with the float64 2D-CTC oracle has a tolerance,
and it is not a number: a multiple of the float32 restatement's own error against that oracle, as tests/test_lexicon_ctc_gpu.py
bounds its kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ctc2d_read_ref as R  # noqa: E402
import _lexicon_ctc_ref as Q  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import ptr  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.ops import decode as decode_ops  # noqa: E402
from megreader_amd.ops.decode import (ctc2d_char_rows, ctc2d_greedy_decode, ctc2d_marginal, ctc_beam_search_decode,  # noqa: E402
                                      ctc_forced_align, ctc_greedy_decode)
from megreader_amd.ops.lexicon import Lexicon  # noqa: E402
from oracle import ctc2d as O  # noqa: E402

DEV = "cuda"
GARBAGE_I, GARBAGE_F = 12345, 777.0
SHAPES = [(1, 2, 1, 1), (2, 37, 3, 33), (3, 65, 8, 32), (1, 6000, 2, 5), (0, 5, 4, 4), (2, 5, 4, 0)]     # (N, C, H, W)
LAYOUTS = ("nhwc", "nchw", "strided")
CODE = {torch.float32: 0, torch.bfloat16: 1}


def random_head(seed, N, C, H, W):
    """f32 classify [N, C, H, W] (softmax over the classes) and mask [N, 1, H, W] (softmax over the heights)."""
    rng = np.random.RandomState(seed)
    z = rng.randn(N, C, H, W) * 2.0
    a = rng.randn(N, 1, H, W) * 2.0
    cl = np.exp(z - (z.max(axis=1, keepdims=True) if C else 0.0))
    cl /= cl.sum(axis=1, keepdims=True) if C else 1.0
    mk = np.exp(a - (a.max(axis=2, keepdims=True) if H else 0.0))
    mk /= mk.sum(axis=2, keepdims=True) if H else 1.0
    return cl.astype(np.float32), mk.astype(np.float32)


def lay(x, layout, dtype=torch.float32):
    """The values of x [N, C, H, W] (numpy f32) on the device in one of three layouts: "nhwc", the project's own head (an NHWC
    buffer viewed as NCHW: the class has unit stride); "nchw", a contiguous tensor (the column has unit stride); "strided", a slice
    with a step in the classes and in the columns of a larger tensor (neither)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)
    if layout == "nhwc":
        v = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert v.shape[1] <= 1 or v.numel() == 0 or v.stride(1) == 1
    elif layout == "nchw":
        v = t.contiguous()
    else:
        N, C, H, W = t.shape
        big = torch.full((N, 2 * C + 1, H, 3 * W + 2), 0.5, dtype=dtype, device=DEV)
        v = big[:, 1::2, :, 2::3]
        assert v.shape == t.shape
        v.copy_(t)
        assert W <= 1 or v.numel() == 0 or v.stride(3) == 3
    assert torch.equal(v, t)
    return v


def read_as_f32(t):
    """What the kernel reads of a device tensor, as numpy f32."""
    return t.float().cpu().numpy()


def raw_marginal(cl, mk, reduce=0, log_out=0, expect=0, override=()):
    """The C entry point on device tensors.  `out` is the [:, :C, :W] corner of a garbage-filled [N, C + 1, W + 3] buffer (its own
    three strides); the cells outside the corner must come back untouched.  Returns out as numpy (None when `expect` != 0)."""
    N, C, H, W = cl.shape
    buf = torch.full((N, C + 1, W + 3), GARBAGE_F, dtype=torch.float32, device=DEV)
    out = buf[:, :C, :W]
    cn, cc, ch, cw = cl.stride()
    mn, _, mh, mw = mk.stride()
    on, oc, ow = out.stride()
    a = dict(dtype=CODE[cl.dtype], classify=ptr(cl), cn=cn, cc=cc, ch=ch, cw=cw, mask=ptr(mk), mn=mn, mh=mh, mw=mw, N=N, C=C, H=H,
             W=W, reduce=reduce, log_out=log_out, out=out.data_ptr() if out.numel() else 0, on=on, oc=oc, ow=ow)
    a.update(dict(override))
    rc = _lib.load().mr_ctc2d_marginal(*[a[k] for k in ("dtype", "classify", "cn", "cc", "ch", "cw", "mask", "mn", "mh", "mw", "N",
                                                         "C", "H", "W", "reduce", "log_out", "out", "on", "oc", "ow")],
                                       _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.load().mr_last_error().decode())
    got = out.cpu().numpy().copy()
    buf[:, :C, :W] = GARBAGE_F
    assert bool((buf == GARBAGE_F).all()), "cells outside out were written"
    if expect != 0:
        assert np.all(got == GARBAGE_F), "an error return wrote to out"
        return None
    return got


def same_bits(got, want, name=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert len(bad) == 0, "%s: %d cells differ, first at %s: kernel %r, restatement %r" % (
        name, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- mr_ctc2d_marginal

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_marginal_equals_the_restatement_in_every_layout(shape, dtype):
    N, C, H, W = shape
    cl, mk = random_head(sum(shape), N, C, H, W)
    tensors = {layout: (lay(cl, layout, dtype), lay(mk, layout, dtype)) for layout in LAYOUTS}
    cl_read, mk_read = (read_as_f32(t) for t in tensors["nchw"])           # (bf16: the rounded values are what is reduced)
    for reduce in (0, 1):
        for log_out in (0, 1):
            want = R.marginal(cl_read, mk_read, 'max' if reduce else 'sum', bool(log_out))
            assert want.shape == (N, C, W) and not np.isnan(want).any()
            for layout in LAYOUTS:
                got = raw_marginal(*tensors[layout], reduce=reduce, log_out=log_out)
                same_bits(got, want, "%s %s reduce %d log %d %s" % (shape, dtype, reduce, log_out, layout))
    if N and W and H > 1:
        assert not np.array_equal(R.marginal(cl_read, mk_read, 'sum'), R.marginal(cl_read, mk_read, 'max'))


def test_marginal_sum_order_is_ascending_h():
    """Heights whose f32 sum depends on the order (1 + 2^-24 + 2^-24 is 1 from the left, 1 + 2^-23 from the right), in every
    layout and beyond one chunk of heights; products that an fma would not round."""
    H = 11
    col = np.array([1.0] + [2.0 ** -24] * (H - 1), dtype=np.float32)
    cl = np.stack([col, col[::-1]], axis=0).reshape(1, 2, H, 1).repeat(3, axis=3)
    mk = np.ones((1, 1, H, 3), dtype=np.float32)
    want = R.marginal(cl, mk)
    assert want[0, 0, 0] == np.float32(1.0) and want[0, 1, 0] > np.float32(1.0)
    rng = np.random.RandomState(4)
    cl2, mk2 = rng.rand(2, 9, 19, 7).astype(np.float32), rng.rand(2, 1, 19, 7).astype(np.float32)
    for layout in LAYOUTS:
        same_bits(raw_marginal(lay(cl, layout), lay(mk, layout)), want, layout)
        for reduce in (0, 1):
            same_bits(raw_marginal(lay(cl2, layout), lay(mk2, layout), reduce=reduce),
                      R.marginal(cl2, mk2, 'max' if reduce else 'sum'), "19 heights " + layout)


def test_marginal_exact_zeros():
    cl, mk = random_head(7, 2, 9, 4, 6)
    mk[0, 0, :, 2] = 0.0                                                       # a column whose mask is 0 everywhere
    cl[1, 3, :, :] = 0.0                                                       # a class that is impossible throughout
    cl[0, 5, 1, 4] = 0.0
    for layout in LAYOUTS:
        for reduce in (0, 1):
            plain = raw_marginal(lay(cl, layout), lay(mk, layout), reduce=reduce)
            logs = raw_marginal(lay(cl, layout), lay(mk, layout), reduce=reduce, log_out=1)
            same_bits(plain, R.marginal(cl, mk, 'max' if reduce else 'sum'))
            same_bits(logs, R.marginal(cl, mk, 'max' if reduce else 'sum', True))
            assert np.all(plain[0, :, 2] == 0.0) and np.all(logs[0, :, 2] == -np.inf)
            assert np.all(plain[1, 3, :] == 0.0) and np.all(logs[1, 3, :] == -np.inf)
            assert not np.isnan(logs).any() and np.isfinite(logs[0, 5, 4])


def test_marginal_python_layer():
    cl, mk = random_head(11, 3, 38, 4, 16)
    want = R.marginal(cl, mk)
    for layout in LAYOUTS:
        got = ctc2d_marginal(lay(cl, layout), lay(mk, layout))
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (3, 38, 16) and got.is_cuda
        same_bits(got.cpu().numpy(), want, layout)
    same_bits(ctc2d_marginal(lay(cl, "nhwc"), lay(mk, "nchw"), reduce='max', log=True).cpu().numpy(),
              R.marginal(cl, mk, 'max', True))
    same_bits(ctc2d_marginal(lay(cl, "nchw").double(), lay(mk, "nchw").double()).cpu().numpy(), want)    # other types: through f32
    half = (lay(cl, "nhwc", torch.bfloat16), lay(mk, "nchw", torch.bfloat16))
    same_bits(ctc2d_marginal(*half).cpu().numpy(), R.marginal(read_as_f32(half[0]), read_as_f32(half[1])))
    # the logs are the readers' own lp: the same bits out of the beam either way
    post, logs = ctc2d_marginal(lay(cl, "nhwc"), lay(mk, "nhwc")), ctc2d_marginal(lay(cl, "nhwc"), lay(mk, "nhwc"), log=True)
    a, b = ctc_beam_search_decode(post), ctc_beam_search_decode(logs, log_probs=True)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    empty = ctc2d_marginal(torch.zeros((0, 5, 4, 4), device=DEV), torch.zeros((0, 1, 4, 4), device=DEV))
    assert empty.shape == (0, 5, 4) and empty.is_cuda
    no_height = ctc2d_marginal(torch.zeros((2, 5, 0, 4), device=DEV), torch.zeros((2, 1, 0, 4), device=DEV))
    assert no_height.shape == (2, 5, 4) and bool((no_height == 0).all())


def test_greedy_of_the_max_marginal_is_the_2d_greedy_decode():
    cases = R.greedy_cases(50, (3, 6, 4, 9), seed=0)                           # the tie-free cases of tests/test_ctc2d_read_cpu.py
    assert all(R.tie_free(cl, mk) for cl, mk in cases)
    cl = np.concatenate([c for c, _ in cases])
    mk = np.concatenate([m for _, m in cases])
    for layout in ("nhwc", "nchw"):
        d_cl, d_mk = lay(cl, layout), lay(mk, layout)
        ids, lengths = ctc_greedy_decode(ctc2d_marginal(d_cl, d_mk, reduce='max'))
        ids2, lengths2 = ctc2d_greedy_decode(d_cl, d_mk)
        assert torch.equal(ids, ids2) and torch.equal(lengths, lengths2)
        assert int(lengths.min()) >= 0 and int(lengths.max()) > 1


def test_lexicon_scores_of_the_marginal_are_the_2d_ctc_likelihoods():
    """`Lexicon.transcribe(ctc2d_marginal(...), all_scores=True)` against -nll of oracle.ctc2d.ctc2d in float64 on the products the
    kernel reads.  Bound: 8 x the error of the float32 restatement (R.marginal, then the float32 alpha recursion) against the
    same oracle -- the method and the factor of tests/test_lexicon_ctc_gpu.py."""
    T, H, N, C = 16, 4, 5, 38
    cs = EnglishCharset()
    assert len(cs) == C
    _, log_mask, log_cls = O.synthetic_lp(T, H, N, C)
    cl = np.ascontiguousarray(np.exp(log_cls).astype(np.float32).transpose(2, 3, 1, 0))         # [N, C, H, W]
    mk = np.ascontiguousarray(np.exp(log_mask).astype(np.float32).transpose(2, 1, 0))[:, None]  # [N, 1, H, W]
    rng = np.random.RandomState(5)
    targets = [rng.randint(2, C, size=k).tolist() for k in (1, 3, 5, 8, 8)]
    others = [rng.randint(2, C, size=k).tolist() for k in (2, 4, 6, 7)]
    words = targets + others
    lex = Lexicon([cs.label_to_string(np.array(w)) for w in words], cs)
    assert [lex.sym[lex.off[i]:lex.off[i + 1]].tolist() for i in range(len(lex))] == words
    # the truth: the 2D-CTC log-likelihood of every word on every row, from the unclamped float64 products
    with np.errstate(divide='ignore'):
        lp64 = np.log(cl.astype(np.float64) * mk.astype(np.float64)).transpose(3, 2, 0, 1)      # [T, H, N, C]
    truth = np.zeros((N, len(words)))
    for l, w in enumerate(words):
        truth[:, l] = -O.ctc2d(lp64, np.tile(np.array(w), (N, 1)), [T] * N, [len(w)] * N, blank=cs.blank)['nll']
    assert np.all(np.isfinite(truth))
    y = np.ascontiguousarray(R.marginal(cl, mk).transpose(0, 2, 1))                             # [N, T, C] f32
    S32 = Q.score_table(Q.log_probs(y, np.float32), words, cs.blank, np.float32, cs.unknown)
    e32 = float(np.abs(S32.astype(np.float64) - truth).max())
    tol = 8.0 * e32
    worst = 0.0
    for layout in ("nhwc", "nchw"):
        found = lex.transcribe(ctc2d_marginal(lay(cl, layout), lay(mk, layout)), all_scores=True)
        got = found['scores'].cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(got - truth).max()))
        index = found['index'].cpu().numpy()
        assert np.all(truth[np.arange(N), index] >= truth.max(axis=1) - 2 * tol)
    print("e32 = %.3g, tol = %.3g, max |kernel - 2D oracle| = %.3g (%.2f e32)" % (e32, tol, worst, worst / e32))
    assert e32 > 0 and worst <= tol


# ---- mr_ctc2d_char_rows

def raw_char_rows(cl, mk, targets, lengths, pos, begin, end, blank=0, expect=0, override=()):
    """The C entry point; every output lies between two garbage rows of a larger buffer and starts as garbage itself."""
    N, C, H, W = cl.shape
    targets = np.asarray(targets, dtype=np.int32)
    S = targets.size // max(N, 1)
    targets = targets.reshape(N, S)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    tg, ln, ps, bg, en = dev(targets), dev(lengths), dev(pos), dev(begin), dev(end)
    bufs = {'rows': torch.full((N + 2, W), GARBAGE_I, dtype=torch.int32, device=DEV),
            'row_lo': torch.full((N + 2, max(S, 1)), GARBAGE_I, dtype=torch.int32, device=DEV),
            'row_hi': torch.full((N + 2, max(S, 1)), GARBAGE_I, dtype=torch.int32, device=DEV)}
    cn, cc, ch, cw = cl.stride()
    mn, _, mh, mw = mk.stride()
    a = dict(dtype=CODE[cl.dtype], classify=ptr(cl), cn=cn, cc=cc, ch=ch, cw=cw, mask=ptr(mk), mn=mn, mh=mh, mw=mw, N=N, C=C, H=H,
             W=W, blank=blank, targets=ptr(tg) if S else 0, S=S, target_len=ptr(ln), pos=ptr(ps), begin=ptr(bg) if S else 0,
             end=ptr(en) if S else 0, rows=bufs['rows'][1].data_ptr(), row_lo=bufs['row_lo'][1].data_ptr(),
             row_hi=bufs['row_hi'][1].data_ptr())
    a.update(dict(override))
    rc = _lib.load().mr_ctc2d_char_rows(*[a[k] for k in ("dtype", "classify", "cn", "cc", "ch", "cw", "mask", "mn", "mh", "mw", "N",
                                                          "C", "H", "W", "blank", "targets", "S", "target_len", "pos", "begin", "end",
                                                          "rows", "row_lo", "row_hi")], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.load().mr_last_error().decode())
    out = {}
    for key, buf in bufs.items():
        width = W if key == 'rows' else S
        flat = buf.cpu().numpy().reshape(-1)
        lo, hi = buf.shape[1], buf.shape[1] + N * width                      # (S == 0: the buffer is one column wide, unused)
        assert np.all(flat[:lo] == GARBAGE_I) and np.all(flat[hi:] == GARBAGE_I), "%s: cells around the output were written" % key
        out[key] = flat[lo:hi].reshape(N, width).copy()
        if expect != 0:
            assert np.all(out[key] == GARBAGE_I)
    return out


def aligned_case(seed, N, C, H, W, S, lengths, layout="nhwc", dtype=torch.float32, sharp=3.0):
    """A random head whose classes follow the targets along the columns (so that the rows align with a finite score), its
    sum-marginal aligned by `ctc_forced_align`.  Targets have no two equal neighbours.  Returns the device tensors, the numpy values
    as the kernel reads them, targets, lengths and the alignment as numpy."""
    rng = np.random.RandomState(seed)
    letters = np.arange(2, C)
    targets = np.zeros((N, max(S, 1)), dtype=np.int32)[:, :S]
    for n in range(N):
        for i in range(S):
            targets[n, i] = rng.choice(letters[letters != (targets[n, i - 1] if i else -1)])
    z = rng.randn(N, C, H, W) * 2.0
    for n in range(N):
        K = int(lengths[n])
        for w in range(W):
            if 0 < K <= S:
                z[n, targets[n, min(K - 1, w * K // W)], :, w] += sharp
    a = rng.randn(N, 1, H, W) * 2.0
    cl = np.exp(z - z.max(axis=1, keepdims=True))
    cl /= cl.sum(axis=1, keepdims=True)
    mk = np.exp(a - a.max(axis=2, keepdims=True))
    mk /= mk.sum(axis=2, keepdims=True)
    d_cl, d_mk = lay(cl.astype(np.float32), layout, dtype), lay(mk.astype(np.float32), layout, dtype)
    lengths = np.asarray(lengths, dtype=np.int32)
    tg, ln = torch.from_numpy(np.ascontiguousarray(targets)).to(DEV), torch.from_numpy(lengths).to(DEV)
    align = ctc_forced_align(ctc2d_marginal(d_cl, d_mk), tg, ln)
    return d_cl, d_mk, read_as_f32(d_cl), read_as_f32(d_mk), targets, lengths, align, tg, ln


def check_rows(case, blank=0, name=""):
    d_cl, d_mk, cl, mk, targets, lengths, align, tg, ln = case
    pos, begin, end = (align[k].cpu().numpy() for k in ('pos', 'begin', 'end'))
    want = R.char_rows(cl, mk, targets, lengths, pos, begin, end, blank)
    got = raw_char_rows(d_cl, d_mk, targets, lengths, pos, begin, end, blank)
    for key in ('rows', 'row_lo', 'row_hi'):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (name, key, got[key], want[key])
    wrapped = ctc2d_char_rows(d_cl, d_mk, tg, ln, align, blank=blank)
    assert sorted(wrapped) == ['row_hi', 'row_lo', 'rows']
    for key in wrapped:
        assert wrapped[key].dtype == torch.int32 and np.array_equal(wrapped[key].cpu().numpy(), want[key]), (name, key)
    return want, pos


@pytest.mark.parametrize("W", [12, 129])
@pytest.mark.parametrize("S", [1, 8, 70])
def test_char_rows_of_aligned_random_heads(S, W):
    N, C, H = 5, 9, 5
    lengths = [S, max(S - 1, 0), 0, min(S, 3), S]                              # full, shorter, empty, short, full
    layout = LAYOUTS[(S + W) % 3]
    want, pos = check_rows(aligned_case(S * 1000 + W, N, C, H, W, S, lengths, layout), name="S=%d W=%d %s" % (S, W, layout))
    alive = pos[:, 0] >= 0
    assert alive[2] and np.all(want['rows'][2] >= 0) and np.all(want['row_lo'][2] == -1)         # length 0: blanks have heights too
    if S <= W:
        assert alive.all() and np.all(want['row_lo'][0] >= 0) and np.all(want['row_hi'][0] >= want['row_lo'][0])
        assert want['rows'].max() > 0                                          # not every column on the lowest height
        if S < W:
            assert (want['row_hi'] > want['row_lo']).any()                     # a band of more than one height
    else:                                                                      # 70 symbols, 12 columns: unalignable, all -1
        assert not alive[0] and np.all(want['rows'][0] == -1) and np.all(want['row_lo'][0] == -1) and np.all(want['row_hi'][0] == -1)


def test_char_rows_wide_alphabet_bf16_and_another_blank():
    check_rows(aligned_case(1, 2, 6000, 2, 12, 8, [8, 5], "nhwc"), name="C = 6000 nhwc")
    check_rows(aligned_case(2, 2, 6000, 2, 12, 8, [8, 5], "nchw"), name="C = 6000 nchw")
    check_rows(aligned_case(3, 3, 9, 11, 20, 6, [6, 2, 4], "nchw", torch.bfloat16), name="bf16, 11 heights")
    case = aligned_case(4, 3, 9, 3, 20, 6, [6, 2, 4], "strided")
    d_cl, d_mk, cl, mk, targets, lengths, _, tg, ln = case
    align = ctc_forced_align(ctc2d_marginal(d_cl, d_mk), tg, ln, blank=1, unknown=0)            # (the targets are 2..8)
    check_rows(case[:6] + (align, tg, ln), blank=1, name="blank 1")


def test_char_rows_unaligned_rows_ties_and_no_symbols():
    d_cl, d_mk, cl, mk, targets, lengths, align, tg, ln = aligned_case(6, 3, 7, 4, 10, 4, [4, 4, 4])
    pos, begin, end = (align[k].cpu().numpy().copy() for k in ('pos', 'begin', 'end'))
    pos[1], begin[1], end[1] = -1, -1, -1                                      # as mr_ctc_align leaves a row it could not align
    got = raw_char_rows(d_cl, d_mk, targets, lengths, pos, begin, end)
    want = R.char_rows(cl, mk, targets, lengths, pos, begin, end)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    assert np.all(got['rows'][1] == -1) and np.all(got['row_lo'][1] == -1) and np.all(got['rows'][[0, 2]] >= 0)
    # every product of a column equal: the lowest height
    flat_cl, flat_mk = np.full_like(cl, 0.25), np.full_like(mk, 0.25)
    got = raw_char_rows(lay(flat_cl, "nchw"), lay(flat_mk, "nchw"), targets, lengths, pos, begin, end)
    assert np.all(got['rows'][[0, 2]] == 0) and np.all(got['row_hi'][[0, 2]] == 0)
    # positions and lengths that name nothing are -1, not a read outside the string
    wild = pos.copy()
    wild[0, :3] = [9, 2 * 4 + 1, 1 << 30]
    got = raw_char_rows(d_cl, d_mk, targets, [4, 4, 300], wild, begin, end)
    want = R.char_rows(cl, mk, targets, [4, 4, 300], wild, begin, end)
    assert all(np.array_equal(got[k], want[k]) for k in want) and got['rows'][0, :3].tolist() == [-1, -1, -1]
    # S == 0: no symbol, only the blanks' heights
    none = raw_char_rows(d_cl, d_mk, np.zeros((3, 0), dtype=np.int32), [0, 0, 0], np.zeros((3, 10), dtype=np.int32),
                         np.zeros((3, 0), dtype=np.int32), np.zeros((3, 0), dtype=np.int32))
    assert np.array_equal(none['rows'], R.char_rows(cl, mk, np.zeros((3, 0)), [0, 0, 0], np.zeros((3, 10)), None, None)['rows'])


def test_capturable_in_a_graph():
    d_cl, d_mk, cl, mk, targets, lengths, align, tg, ln = aligned_case(8, 4, 9, 4, 16, 5, [5, 3, 0, 5])
    other_cl, other_mk = d_cl.flip(0).contiguous(), d_mk.flip(0).contiguous()

    def run(c, m):
        post = ctc2d_marginal(c, m)
        found = ctc_forced_align(post, tg, ln)
        return dict(ctc2d_char_rows(c, m, tg, ln, found), post=post)

    eager = {k: v.clone() for k, v in run(d_cl, d_mk).items()}
    eager_other = {k: v.clone() for k, v in run(other_cl, other_mk).items()}
    s_cl, s_mk = d_cl.clone(), d_mk.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(s_cl, s_mk)
    for (c, m), want in (((d_cl, d_mk), eager), ((other_cl, other_mk), eager_other)):
        s_cl.copy_(c)
        s_mk.copy_(m)
        graph.replay()
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(out[key].view(torch.int32), want[key].view(torch.int32)), key
    assert not torch.equal(eager['rows'], eager_other['rows'])


# ---- what is refused, and before any launch

def test_entry_points_refuse_bad_arguments():
    cl, mk = (lay(x, "nchw") for x in random_head(9, 2, 5, 3, 4))
    for override in (dict(reduce=2), dict(log_out=-1), dict(N=-1), dict(H=-2), dict(classify=0), dict(mask=0), dict(out=0),
                     dict(cn=1 << 62)):
        raw_marginal(cl, mk, expect=1, override=override)
    raw_marginal(cl, mk, expect=2, override=dict(dtype=2))
    pos, none = np.zeros((2, 4), dtype=np.int32), np.full((2, 3), -1, dtype=np.int32)
    for override in (dict(N=-1), dict(H=0), dict(W=0), dict(C=0), dict(S=257), dict(S=-1), dict(blank=5), dict(blank=-1),
                     dict(classify=0), dict(pos=0), dict(rows=0), dict(row_lo=0), dict(targets=0), dict(mh=1 << 62)):
        raw_char_rows(cl, mk, np.full((2, 3), 2), [0, 0], pos, none, none, expect=1, override=override)
    raw_char_rows(cl, mk, np.full((2, 3), 2), [0, 0], pos, none, none, expect=2, override=dict(dtype=7))


def test_python_layer_refuses_before_any_launch(monkeypatch):
    cl, mk = (lay(x, "nchw") for x in random_head(10, 2, 5, 3, 4))
    tg = torch.full((2, 3), 2, dtype=torch.int32, device=DEV)
    ln = torch.tensor([3, 2], dtype=torch.int32, device=DEV)
    align = ctc_forced_align(ctc2d_marginal(cl, mk), tg, ln)
    monkeypatch.setattr(decode_ops, "call", lambda *a: pytest.fail("an entry point was reached: %s" % (a[0],)))
    for bad, error in ((lambda: ctc2d_marginal(cl[0], mk), RuntimeError),                       # wrong shapes
                       (lambda: ctc2d_marginal(cl, mk[:, :, :2]), RuntimeError),
                       (lambda: ctc2d_marginal(cl, mk.expand(2, 5, 3, 4)), RuntimeError),
                       (lambda: ctc2d_marginal(cl, mk, reduce='mean'), ValueError),
                       (lambda: ctc2d_marginal(cl.cpu(), mk.cpu()), NotImplementedError),       # wrong device
                       (lambda: ctc2d_marginal(cl, mk.cpu()), NotImplementedError),
                       (lambda: ctc2d_marginal(cl, mk.to(torch.bfloat16)), TypeError),          # mixed dtypes
                       (lambda: ctc2d_marginal(cl.double(), mk), TypeError),
                       (lambda: ctc2d_char_rows(cl, mk[:1], tg, ln, align), RuntimeError),
                       (lambda: ctc2d_char_rows(cl, mk, tg[:1], ln, align), ValueError),
                       (lambda: ctc2d_char_rows(cl, mk, tg, ln[:1], align), ValueError),
                       (lambda: ctc2d_char_rows(cl, mk, tg, ln, dict(align, pos=align['pos'][:, :2])), ValueError),
                       (lambda: ctc2d_char_rows(cl, mk, tg, ln, dict(align, begin=align['begin'][:, :2])), ValueError),
                       (lambda: ctc2d_char_rows(cl, mk, tg, ln, align, blank=5), ValueError),
                       (lambda: ctc2d_char_rows(cl, mk, tg.cpu(), ln, align), NotImplementedError),
                       (lambda: ctc2d_char_rows(cl, mk.to(torch.bfloat16), tg, ln, align), TypeError),
                       (lambda: ctc2d_char_rows(cl, mk, torch.zeros((2, 257), dtype=torch.int32, device=DEV), ln, align),
                        ValueError)):
        with pytest.raises(error):
            bad()
