"""Evaluation decode and metrics on the GPU: the reference does these in Python loops over every
sample and time step on the host (structure/representers/ctc_representer.py:20-34, ctc_representer2d.py:27-51,
structure/measurers/sequence_recognition_measurer.py:66-112).  Same rules, bit-exact results
(tests/test_decode_gpu.py against oracle/decode.py, which is pinned to the reference)."""
import math

import torch

from .._lib import _DEFINES, call, load, ptr, require_cuda

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float64: 2}


def _posterior(pred, who, native=(torch.float32, torch.bfloat16), blank=None, t_max=None, error=RuntimeError):
    """What every reader of a CTC posterior does first.  pred: [N, C, 1, T] or [N, C, T], any strides, else `error`; with `blank`
    / `t_max` also the ValueErrors for a blank that is no class (or C < 2) and for T outside 1..t_max.  A dtype that `who`'s
    entry point does not read (`native`) goes through f32 -- after the checks, so that no error comes behind a launch.
    Returns (the [N, C, T] view, (N, C, T), its element strides (sn, sc, st), the library's dtype code)."""
    if pred.dim() == 4 and pred.shape[2] == 1:
        pred = pred.select(2, 0)               # CTCRepresenter: pred.select(1, 0) after the arg-max over C
    if pred.dim() != 3:
        raise error("%s expects [N, C, 1, T] or [N, C, T], got %s" % (who, tuple(pred.shape)))
    N, C, T = pred.shape
    if blank is not None and (C < 2 or not 0 <= blank < C):
        raise ValueError("%s: blank=%d is not one of C=%d classes (C >= 2)" % (who, blank, C))
    if t_max is not None and not 1 <= T <= t_max:
        raise ValueError("%s: T=%d columns, 1..%d are taken" % (who, T, t_max))
    if pred.dtype not in native:
        pred = pred.float()
    return pred, (N, C, T), pred.stride(), _DT[pred.dtype]


def _workspace(nbytes, who, sizes, device):
    """The 8-byte aligned workspace of `nbytes`, the answer of the entry point's *_ws_bytes (0: more than it can address)."""
    if nbytes <= 0:
        raise ValueError("%s: %s need a workspace above 2 GiB; split the batch" % (who, sizes))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def ctc_greedy_decode(pred, blank=0, unknown=1):
    """pred: [N, C, 1, T] or [N, C, T] class scores on the GPU (any strides; f32 / bf16 / f64 are read as they are, other types
    go through f32).  Returns (ids i32 [N, T] blank padded, lengths i32 [N])."""
    require_cuda(pred)
    pred, (N, C, T), (sn, sc, st), code = _posterior(pred, "ctc_greedy_decode", native=tuple(_DT))
    out = torch.empty((N, T), dtype=torch.int32, device=pred.device)
    lengths = torch.empty((N,), dtype=torch.int32, device=pred.device)
    with torch.cuda.device(pred.device):
        call("mr_ctc_greedy_decode", code, ptr(pred), sn, sc, st, N, C, T, int(blank), int(unknown), ptr(out), ptr(lengths))
    return out, lengths


def ctc_beam_search_decode(pred, beam=8, nbest=1, top_classes=16, blank=0, unknown=1, log_probs=False, lm=None, lm_weight=1.0,
                           lm_bonus=0.0, lm_end=True):
    """CTC prefix beam search (mr_ctc_beam_search, include/megreader_hip.h): the `nbest` most probable STRINGS of every row with
    their log-probabilities, where `ctc_greedy_decode` returns the most probable path.  pred: [N, C, 1, T] or [N, C, T] on the GPU,
    any strides; probabilities (the eval head's softmax) or, with log_probs=True, their logs; f32 and bf16 are read as they are,
    other types go through f32.  Decoding is over the classes as given (no case folding: sum the posterior first, as
    `Lexicon` does).  `beam` hypotheses survive a column (1..64), each column offers its `top_classes` best symbols (1..64).
    Returns a dict of device tensors: ids i32 [N, nbest, T] blank padded, lengths i32 [N, nbest], scores f32 [N, nbest]
    (descending; a lower bound of log p(string | pred), exact when nothing was pruned), count i32 [N] (hypotheses returned; slots
    past it: length 0, score -inf).  One call, no host work that depends on device data (capturable in a graph after one call
    outside); the workspace is a fresh tensor per call.
    With `lm`, a `CharNgramLM` (ops/language_model.py) over the same classes, the search is mr_ctc_beam_search_lm: the strings are
    ranked by log p_ctc + lm_weight * log p_lm + lm_bonus * (symbols), with lm_end=True the model's end of string included.  The
    dict gains ctc_scores f32 [N, nbest], the pure CTC log-probability (the lower bound above), and lm_scores f32 [N, nbest], the
    model's weighted part; scores = ctc_scores + lm_scores is what the strings are ordered by.  The model may cover fewer classes
    than C (the others take its floor), not more, and its blank and unknown are the call's: ValueError otherwise.  The model's
    device image is uploaded on the first call per device and C (do that call outside a capture).  lm=None is the call above,
    unchanged."""
    who = "ctc_beam_search_decode"
    beam, nbest, top_classes, blank = int(beam), int(nbest), int(top_classes), int(blank)
    if not 1 <= beam <= _DEFINES["MR_CTC_BEAM_MAX"]:
        raise ValueError("%s: beam must be in 1..%d, got %d" % (who, _DEFINES["MR_CTC_BEAM_MAX"], beam))
    if not 1 <= nbest <= beam:
        raise ValueError("%s: nbest must be in 1..beam=%d, got %d" % (who, beam, nbest))
    if not 1 <= top_classes <= _DEFINES["MR_CTC_BEAM_TOP_MAX"]:
        raise ValueError("%s: top_classes must be in 1..%d, got %d" % (who, _DEFINES["MR_CTC_BEAM_TOP_MAX"], top_classes))
    pred, (N, C, T), (sn, sc, st), code = _posterior(pred, who, blank=blank, t_max=_DEFINES["MR_SEQ_MEASURE_MAX"])
    require_cuda(pred)
    dev = pred.device
    ids = torch.empty((N, nbest, T), dtype=torch.int32, device=dev)
    lengths = torch.empty((N, nbest), dtype=torch.int32, device=dev)
    scores = torch.empty((N, nbest), dtype=torch.float32, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    out = {'ids': ids, 'lengths': lengths, 'scores': scores, 'count': count}
    if lm is not None:
        lm_weight, lm_bonus = float(lm_weight), float(lm_bonus)
        if lm.classes > C or lm.blank != blank or lm.unknown != int(unknown):
            raise ValueError("%s: the model is over %d classes with blank=%d unknown=%d, the call has C=%d blank=%d unknown=%d"
                             % (who, lm.classes, lm.blank, lm.unknown, C, blank, int(unknown)))
        if not (math.isfinite(lm_weight) and math.isfinite(lm_bonus)):
            raise ValueError("%s: lm_weight=%r and lm_bonus=%r must be finite" % (who, lm_weight, lm_bonus))
        out['ctc_scores'] = torch.empty((N, nbest), dtype=torch.float32, device=dev)
        out['lm_scores'] = torch.empty((N, nbest), dtype=torch.float32, device=dev)
    if N == 0:
        return out
    ws = _workspace(load().mr_ctc_beam_ws_bytes(N, T, beam, top_classes), who,
                    "N=%d T=%d beam=%d top_classes=%d" % (N, T, beam, top_classes), dev)
    if lm is not None:
        m = lm._tensors(dev, C)
        with torch.cuda.device(dev):
            call("mr_ctc_beam_search_lm", code, ptr(pred), sn, sc, st, N, C, T, int(bool(log_probs)), blank, int(unknown), beam,
                 nbest, top_classes, ptr(m['keys']), ptr(m['arc_lp']), ptr(m['arc_next']), ptr(m['bow']), ptr(m['backoff']),
                 ptr(m['end_lp']), m['states'], m['slots'], m['max_probe'], m['start_state'], m['order'], lm_weight, lm_bonus,
                 int(bool(lm_end)), ptr(ids), ptr(lengths), ptr(scores), ptr(out['ctc_scores']), ptr(out['lm_scores']), ptr(count),
                 ptr(ws), ws.numel() * 8)
        return out
    with torch.cuda.device(dev):
        call("mr_ctc_beam_search", code, ptr(pred), sn, sc, st, N, C, T, int(bool(log_probs)), blank, int(unknown), beam, nbest,
             top_classes, ptr(ids), ptr(lengths), ptr(scores), ptr(count), ptr(ws), ws.numel() * 8)
    return out


def ctc_forced_align(pred, targets, target_lengths, blank=0, unknown=1, log_probs=False):
    """Forced CTC alignment (mr_ctc_align, include/megreader_hip.h): WHERE the symbols of a given string lie in the posterior -- the
    single most probable alignment of row n's string targets[n, :target_lengths[n]], traced back.  pred: [N, C, 1, T] or [N, C, T]
    on the GPU, any strides; probabilities (the eval head's softmax) or, with log_probs=True, their logs; f32 and bf16 are read as
    they are, other types go through f32.  targets: i32 [N, S] and target_lengths: i32 [N], on the device (S up to 256); the
    classes are taken as given (no case folding: sum the posterior first, as `Lexicon` does).  Returns a dict of device tensors:
    score f32 [N], the log-probability of the best alignment; pos i32 [N, T], the position of every column in the blank-extended
    string (2i + 1: symbol i, even: a blank); begin, end i32 [N, S], the columns [begin, end) of symbol i; sym_lp f32 [N, S], the
    sum of the symbol's log-probabilities over them; peak i32 [N, S], its most probable column.  Slots past the string: -1, -1,
    -inf, -1.  A row that cannot be aligned (a symbol that is blank, `unknown` or no class, a length outside [0, S], more symbols
    than columns) or only through zero probabilities: score -inf, pos -1, every slot as one past the string.  One call, no host
    work that depends on device data (capturable in a graph); the workspace is a fresh tensor per call."""
    who = "ctc_forced_align"
    blank = int(blank)
    pred, (N, C, T), (sn, sc, st), code = _posterior(pred, who, blank=blank, t_max=_DEFINES["MR_SEQ_MEASURE_MAX"])
    if targets.dim() != 2 or targets.shape[0] != N:
        raise ValueError("%s: targets must be [N=%d, S], got %s" % (who, N, tuple(targets.shape)))
    if tuple(target_lengths.shape) != (N,):
        raise ValueError("%s: target_lengths must be [N=%d], got %s" % (who, N, tuple(target_lengths.shape)))
    S = targets.shape[1]
    if S > _DEFINES["MR_CTC_ALIGN_MAX_SYMBOLS"]:
        raise ValueError("%s: S=%d symbols per row, 0..%d are taken" % (who, S, _DEFINES["MR_CTC_ALIGN_MAX_SYMBOLS"]))
    require_cuda(pred, targets, target_lengths)
    if targets.device != pred.device or target_lengths.device != pred.device:
        raise ValueError("%s: pred is on %s, targets on %s, target_lengths on %s"
                         % (who, pred.device, targets.device, target_lengths.device))
    targets = targets.to(torch.int32).contiguous()
    target_lengths = target_lengths.to(torch.int32).contiguous()
    dev = pred.device
    out = {'score': torch.empty((N,), dtype=torch.float32, device=dev),
           'pos': torch.empty((N, T), dtype=torch.int32, device=dev),
           'begin': torch.empty((N, S), dtype=torch.int32, device=dev),
           'end': torch.empty((N, S), dtype=torch.int32, device=dev),
           'sym_lp': torch.empty((N, S), dtype=torch.float32, device=dev),
           'peak': torch.empty((N, S), dtype=torch.int32, device=dev)}
    if N == 0:
        return out
    ws = _workspace(load().mr_ctc_align_ws_bytes(N, T, S), who, "N=%d T=%d S=%d" % (N, T, S), dev)
    with torch.cuda.device(dev):
        call("mr_ctc_align", code, ptr(pred), sn, sc, st, N, C, T, int(bool(log_probs)), blank, int(unknown), ptr(targets), S,
             ptr(target_lengths), ptr(out['score']), ptr(out['pos']), ptr(out['begin']), ptr(out['end']), ptr(out['sym_lp']),
             ptr(out['peak']), ptr(ws), ws.numel() * 8)
    return out


def ctc2d_greedy_decode(classify, mask, blank=0, unknown=1):
    """classify [N, C, H, W], mask [N, 1, H, W] on the GPU (any strides; converted to f32 if needed).
    Returns (ids i32 [N, W], lengths i32 [N])."""
    require_cuda(classify, mask)
    if classify.dtype != torch.float32:
        classify = classify.float()
    if mask.dtype != torch.float32:
        mask = mask.float()
    N, C, H, W = classify.shape
    if tuple(mask.shape) != (N, 1, H, W):
        raise RuntimeError("mask must be [N, 1, H, W]")
    out = torch.empty((N, W), dtype=torch.int32, device=classify.device)
    lengths = torch.empty((N,), dtype=torch.int32, device=classify.device)
    cn, cc, ch, cw = classify.stride()
    mn, _, mh, mw = mask.stride()
    call("mr_ctc2d_greedy_decode", ptr(classify), cn, cc, ch, cw, ptr(mask), mn, mh, mw, N, C, H, W, int(blank),
         int(unknown), ptr(out), ptr(lengths))
    return out, lengths


def _head2d(classify, mask, who):
    """What both readers of a 2-D head do first.  classify [N, C, H, W] and mask [N, 1, H, W] on one device, any strides, else the
    error; the two have one dtype (TypeError); f32 and bf16 are read as they are, other types go through f32 -- after the checks.
    Returns (classify, mask, (N, C, H, W), the library's dtype code)."""
    require_cuda(classify, mask)
    if classify.dim() != 4:
        raise RuntimeError("%s: classify must be [N, C, H, W], got %s" % (who, tuple(classify.shape)))
    N, C, H, W = classify.shape
    if tuple(mask.shape) != (N, 1, H, W):
        raise RuntimeError("%s: mask must be [N, 1, H, W] = %s, got %s" % (who, (N, 1, H, W), tuple(mask.shape)))
    if mask.device != classify.device:
        raise ValueError("%s: classify is on %s, mask on %s" % (who, classify.device, mask.device))
    if classify.dtype != mask.dtype:
        raise TypeError("%s: classify is %s, mask %s: one type for both" % (who, classify.dtype, mask.dtype))
    if classify.dtype not in (torch.float32, torch.bfloat16):
        classify, mask = classify.float(), mask.float()
    return classify, mask, (N, C, H, W), _DT[classify.dtype]


def ctc2d_marginal(classify, mask, reduce='sum', log=False):
    """The 1-D CTC posterior of a 2D-CTC head (mr_ctc2d_marginal, include/megreader_hip.h): f32 [N, C, W],
        q[n, c, w] = sum_h classify[n, c, h, w] * mask[n, 0, h, w]
    for classify [N, C, H, W] and mask [N, 1, H, W] on the GPU, the head's eval output (any strides; an f32 or a bf16 pair is read
    as it is, other types go through f32).  The 2D-CTC recursion sums alpha over the heights of the previous column before every
    step, so its string probabilities are exactly the 1-D CTC probabilities of q: `ctc_beam_search_decode`, `Lexicon.transcribe`
    and `ctc_forced_align` read q as any other posterior.  Two differences from the training loss `ctc_loss_2d`: it returns inf for
    an empty target (its recursion does not run), where the 1-D readers give the all-blank probability; and it clamps every
    product at `tiny` before the log, which the eval tensors are not.  reduce='max' takes the greatest product instead, and
    `ctc_greedy_decode` of that is the 2-D greedy rule of `ctc2d_greedy_decode` wherever no two products of a column tie.
    log=True returns the f32 nearest to the log (0 gives -inf): the readers' own lp, for their log_probs=True.
    The arithmetic is fixed (every product rounded to f32, added or maximised in ascending h), so the bits do not depend on the
    layout.  The result is contiguous, W fastest: a class's columns side by side, as the readers read the 1-D head's [N, C, 1, T].
    One launch, capturable."""
    who = "ctc2d_marginal"
    if reduce not in ('sum', 'max'):
        raise ValueError("%s: reduce must be 'sum' or 'max', got %r" % (who, reduce))
    classify, mask, (N, C, H, W), code = _head2d(classify, mask, who)
    out = torch.empty((N, C, W), dtype=torch.float32, device=classify.device)
    cn, cc, ch, cw = classify.stride()
    mn, _, mh, mw = mask.stride()
    on, oc, ow = out.stride()
    with torch.cuda.device(classify.device):
        call("mr_ctc2d_marginal", code, ptr(classify), cn, cc, ch, cw, ptr(mask), mn, mh, mw, N, C, H, W,
             int(reduce == 'max'), int(bool(log)), ptr(out), on, oc, ow)
    return out


def ctc2d_char_rows(classify, mask, targets, target_lengths, align, blank=0):
    """WHERE the symbols of an aligned string lie vertically in a 2D-CTC head (mr_ctc2d_char_rows, include/megreader_hip.h).
    classify, mask: as for `ctc2d_marginal`; targets i32 [N, S], target_lengths i32 [N] and `align`, the dict
    `ctc_forced_align(ctc2d_marginal(classify, mask), targets, target_lengths)` returned (its 'pos', 'begin' and 'end' are read).
    Given the alignment the heights of the columns are independent, so each column's most probable height is its own arg-max.
    Returns a dict of device tensors: rows i32 [N, W], per column the h with the greatest product classify * mask of the class the
    alignment gives the column (the blank at even positions, else the symbol; the lowest h among equal products; -1 where 'pos'
    is); row_lo, row_hi i32 [N, S], the least and the greatest of them over the symbol's columns [begin, end), -1 past the string
    and for a row that was not aligned.  One launch, no host work that depends on device data (capturable in a graph)."""
    who = "ctc2d_char_rows"
    blank = int(blank)
    classify, mask, (N, C, H, W), code = _head2d(classify, mask, who)
    if C < 1 or H < 1 or W < 1 or not 0 <= blank < C:
        raise ValueError("%s: C=%d H=%d W=%d blank=%d: at least one class, height and column, the blank a class"
                         % (who, C, H, W, blank))
    if targets.dim() != 2 or targets.shape[0] != N:
        raise ValueError("%s: targets must be [N=%d, S], got %s" % (who, N, tuple(targets.shape)))
    S = targets.shape[1]
    if S > _DEFINES["MR_CTC_ALIGN_MAX_SYMBOLS"]:
        raise ValueError("%s: S=%d symbols per row, 0..%d are taken" % (who, S, _DEFINES["MR_CTC_ALIGN_MAX_SYMBOLS"]))
    if tuple(target_lengths.shape) != (N,):
        raise ValueError("%s: target_lengths must be [N=%d], got %s" % (who, N, tuple(target_lengths.shape)))
    pos, begin, end = align['pos'], align['begin'], align['end']
    if tuple(pos.shape) != (N, W) or tuple(begin.shape) != (N, S) or tuple(end.shape) != (N, S):
        raise ValueError("%s: align must hold pos [N=%d, W=%d] and begin, end [N, S=%d], got %s, %s, %s"
                         % (who, N, W, S, tuple(pos.shape), tuple(begin.shape), tuple(end.shape)))
    require_cuda(targets, target_lengths, pos, begin, end)
    dev = classify.device
    if any(t.device != dev for t in (targets, target_lengths, pos, begin, end)):
        raise ValueError("%s: classify is on %s, targets, target_lengths and align on %s"
                         % (who, dev, ", ".join(str(t.device) for t in (targets, target_lengths, pos, begin, end))))
    targets, target_lengths, pos, begin, end = (t.to(torch.int32).contiguous() for t in (targets, target_lengths, pos, begin, end))
    out = {'rows': torch.empty((N, W), dtype=torch.int32, device=dev),
           'row_lo': torch.empty((N, S), dtype=torch.int32, device=dev),
           'row_hi': torch.empty((N, S), dtype=torch.int32, device=dev)}
    cn, cc, ch, cw = classify.stride()
    mn, _, mh, mw = mask.stride()
    with torch.cuda.device(dev):
        call("mr_ctc2d_char_rows", code, ptr(classify), cn, cc, ch, cw, ptr(mask), mn, mh, mw, N, C, H, W, blank, ptr(targets), S,
             ptr(target_lengths), ptr(pos), ptr(begin), ptr(end), ptr(out['rows']), ptr(out['row_lo']), ptr(out['row_hi']))
    return out


def _rows2d(t, who, name, dtype=None):
    """A [.., K] tensor whose last dimension is contiguous and whose leading dimensions are one even run of rows: its leading
    dimension in elements."""
    if t.dim() < 2 or t.stride(-1) != 1 or (dtype is not None and t.dtype != dtype):
        raise ValueError("%s: %s must be %s with a contiguous last dimension, got %s %s strides %s"
                         % (who, name, dtype or "a matrix", t.dtype, tuple(t.shape), t.stride()))
    ld = t.stride(-2)
    for d in range(t.dim() - 2):
        if t.shape[d] > 1 and t.stride(d) != t.stride(d + 1) * t.shape[d + 1]:
            raise ValueError("%s: the rows of %s are not evenly spaced (strides %s)" % (who, name, t.stride()))
    return ld


def attention_read(hproj, eproj, v, logits, words, blank, height, width, attention=False):
    """The replay read of an attention decoder (mr_attn_read, include/megreader_hip.h): what every step of a decode loop saw and
    said, from its hidden states, for all steps in parallel.  hproj [S, N, >= H] (the attention half of the hidden projection of
    H_all[0..S-1]; a column slice of a wider GEMM output is fine), eproj [N, T, H] contiguous, v [H], logits [S, N, >= C] (the
    output layer of H_all[1..S]) -- one dtype, f32 or bf16 -- and words int32 [N, >= S], the word emitted at every step; the grid
    height x width = T.  `C` is `logits.shape[2]` and `H` is `eproj.shape[2]`: pass views of exactly that many columns.
    Returns a dict of device tensors: sym_lp f32 [N, S], the log-probability of every emitted word; moments f32 [N, S, 4], the
    mean and standard deviation (cx, cy, sx, sy) of the attention map in grid cells; length i32 [N], the index of the first
    blank (S: none); score f32 [N], the log-probability of the string with its terminating blank; and with attention=True att
    f32 [N, S, T].  Two launches, capturable."""
    who = "attention_read"
    require_cuda(hproj, eproj, v, logits, words)
    if eproj.dim() != 3 or hproj.dim() != 3 or logits.dim() != 3 or words.dim() != 2:
        raise ValueError("%s: hproj [S, N, H], eproj [N, T, H], logits [S, N, C], words [N, S]; got %s %s %s %s"
                         % (who, tuple(hproj.shape), tuple(eproj.shape), tuple(logits.shape), tuple(words.shape)))
    N, T, H = eproj.shape
    S, C = logits.shape[0], logits.shape[2]
    if tuple(hproj.shape) != (S, N, H) or logits.shape[1] != N or words.shape[0] != N or words.shape[1] < S \
            or tuple(v.shape) != (H,):
        raise ValueError("%s: shapes do not agree: hproj %s eproj %s v %s logits %s words %s"
                         % (who, tuple(hproj.shape), tuple(eproj.shape), tuple(v.shape), tuple(logits.shape), tuple(words.shape)))
    dtype = eproj.dtype
    if dtype not in (torch.float32, torch.bfloat16) or hproj.dtype != dtype or logits.dtype != dtype:
        raise TypeError("%s: hproj, eproj and logits share one of float32 / bfloat16, got %s %s %s"
                        % (who, hproj.dtype, eproj.dtype, logits.dtype))
    if not eproj.is_contiguous():
        raise ValueError("%s: eproj must be contiguous" % who)
    ldh, ldl = _rows2d(hproj, who, "hproj"), _rows2d(logits, who, "logits")
    ldp = _rows2d(words, who, "words", torch.int32)
    vf = v.detach().float().contiguous()
    dev = eproj.device
    out = {'sym_lp': torch.empty((N, S), dtype=torch.float32, device=dev),
           'moments': torch.empty((N, S, 4), dtype=torch.float32, device=dev),
           'length': torch.empty((N,), dtype=torch.int32, device=dev),
           'score': torch.empty((N,), dtype=torch.float32, device=dev)}
    if attention:
        out['att'] = torch.empty((N, S, T), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("mr_attn_read", _DT[dtype], ptr(hproj), ldh, ptr(eproj), ptr(vf), ptr(logits), ldl, ptr(words), ldp, int(blank), N, S,
             T, H, C, int(height), int(width), ptr(out.get('att')), ptr(out['sym_lp']), ptr(out['moments']), ptr(out['length']),
             ptr(out['score']))
    return out


def attention_beam_step(logits, hprime, h_next, score, finished, length, parent, word, feed, s, blank, classes=None):
    """One selection step of the attention beam search (mr_attn_beam_step, include/megreader_hip.h), in place on the caller's
    buffers: logits [N * B, >= C] and hprime, h_next [N * B, H] of one dtype (f32 / bf16, contiguous rows); score f32, finished
    i32, length i32 [N, B]; parent, word i32 [S, N, B]; feed i64 [N, B]; step s.  `classes` = C when the logits rows are
    padded.  One launch, capturable."""
    who = "attention_beam_step"
    require_cuda(logits, hprime, h_next, score, finished, length, parent, word, feed)
    S, N, B = parent.shape
    C = logits.shape[1] if classes is None else int(classes)
    H = hprime.shape[1]
    state = ((score, torch.float32), (finished, torch.int32), (length, torch.int32), (feed, torch.int64))
    if any(tuple(t.shape) != (N, B) or t.dtype != dt or not t.is_contiguous() for t, dt in state) \
            or any(tuple(t.shape) != (S, N, B) or t.dtype != torch.int32 or not t.is_contiguous() for t in (parent, word)):
        raise ValueError("%s: score f32, finished i32, length i32, feed i64 [N, B] and parent, word i32 [S, N, B], contiguous" % who)
    if logits.shape[0] != N * B or tuple(hprime.shape) != (N * B, H) or tuple(h_next.shape) != (N * B, H) \
            or not (hprime.is_contiguous() and h_next.is_contiguous()) or logits.stride(1) != 1 \
            or hprime.dtype != logits.dtype or h_next.dtype != logits.dtype or logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("%s: logits [N * B, C] and hprime, h_next [N * B, H] of one dtype (f32 / bf16), rows contiguous" % who)
    with torch.cuda.device(logits.device):
        call("mr_attn_beam_step", _DT[logits.dtype], ptr(logits), logits.stride(0), ptr(hprime), ptr(h_next), H, ptr(score),
             ptr(finished), ptr(length), ptr(parent), ptr(word), ptr(feed), int(s), S, N, B, C, int(blank))


def attention_beam_trace(parent, word, score, finished, length, nbest, blank):
    """The hypotheses of a finished attention beam search (mr_attn_beam_trace, include/megreader_hip.h) from the buffers
    `attention_beam_step` filled: a dict of device tensors ids i32 [N, nbest, S] blank padded, lengths i32 [N, nbest], scores f32
    [N, nbest] descending, count i32 [N], path i32 [N, nbest, S + 1] (the row a hypothesis occupied entering every step).  One
    launch, capturable."""
    require_cuda(parent, word, score, finished, length)
    S, N, B = parent.shape
    nbest = int(nbest)
    dev = parent.device
    out = {'ids': torch.empty((N, nbest, S), dtype=torch.int32, device=dev),
           'lengths': torch.empty((N, nbest), dtype=torch.int32, device=dev),
           'scores': torch.empty((N, nbest), dtype=torch.float32, device=dev),
           'count': torch.empty((N,), dtype=torch.int32, device=dev),
           'path': torch.empty((N, nbest, S + 1), dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        call("mr_attn_beam_trace", ptr(parent), ptr(word), ptr(score), ptr(finished), ptr(length), S, N, B, nbest, int(blank),
             ptr(out['ids']), ptr(out['lengths']), ptr(out['scores']), ptr(out['count']), ptr(out['path']))
    return out


def sequence_measure(labels, preds, blank=0, unknown=1, fold=None):
    """labels i32 [N, S], preds i32 [N, S2] (device).  Returns dict of device tensors:
    accuracy (bool [N]), edit_distance (f64 [N], the reference's normalised score), distance (i32 [N], the Levenshtein
    distance of the two id sequences without blank / unknown), label_length (i32 [N]).  All four are exact for any
    number of symbols per row; S and S2 above MR_SEQ_MEASURE_MAX (4096, include/megreader_hip.h) raise."""
    require_cuda(labels, preds)
    labels = labels.to(torch.int32).contiguous()
    preds = preds.to(torch.int32).contiguous()
    N, S = labels.shape
    dev = labels.device
    acc = torch.empty((N,), dtype=torch.int32, device=dev)
    ed = torch.empty((N,), dtype=torch.int32, device=dev)
    ll = torch.empty((N,), dtype=torch.int32, device=dev)
    score = torch.empty((N,), dtype=torch.float64, device=dev)
    if fold is not None:
        fold = fold.to(device=dev, dtype=torch.int32).contiguous()
    call("mr_seq_measure", ptr(labels), S, ptr(preds), preds.shape[1], N, int(blank), int(unknown), ptr(fold), ptr(acc),
         ptr(ed), ptr(ll), ptr(score))
    return {'accuracy': acc.bool(), 'edit_distance': score, 'distance': ed, 'label_length': ll}
