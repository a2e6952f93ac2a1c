"""Evaluation decode and metrics on the GPU: the reference does these in Python loops over every
sample and time step on the host (structure/representers/ctc_representer.py:20-34, ctc_representer2d.py:27-51,
structure/measurers/sequence_recognition_measurer.py:66-112).  Same rules, bit-exact results
(tests/test_decode_gpu.py against oracle/decode.py, which is pinned to the reference)."""
import torch

from .._lib import _DEFINES, call, load, ptr, require_cuda

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float64: 2}


def ctc_greedy_decode(pred, blank=0, unknown=1):
    """pred: [N, C, 1, T] or [N, C, T] class scores on the GPU (f32 / bf16 / f64, any strides).
    Returns (ids i32 [N, T] blank padded, lengths i32 [N])."""
    require_cuda(pred)
    if pred.dim() == 4:
        if pred.shape[2] != 1:
            raise RuntimeError("ctc_greedy_decode expects [N, C, 1, T]")
        pred = pred.select(2, 0)           # CTCRepresenter: pred.select(1, 0) after the arg-max over C
    if pred.dtype not in _DT:
        raise TypeError("ctc_greedy_decode: unsupported dtype %s" % pred.dtype)
    N, C, T = pred.shape
    out = torch.empty((N, T), dtype=torch.int32, device=pred.device)
    lengths = torch.empty((N,), dtype=torch.int32, device=pred.device)
    sn, sc, st = pred.stride()
    call("mr_ctc_greedy_decode", _DT[pred.dtype], ptr(pred), sn, sc, st, N, C, T, int(blank), int(unknown), ptr(out),
         ptr(lengths))
    return out, lengths


def ctc_beam_search_decode(pred, beam=8, nbest=1, top_classes=16, blank=0, unknown=1, log_probs=False):
    """CTC prefix beam search (mr_ctc_beam_search, include/megreader_hip.h): the `nbest` most probable STRINGS of every row with
    their log-probabilities, where `ctc_greedy_decode` returns the most probable path.  pred: [N, C, 1, T] or [N, C, T] on the GPU,
    any strides; probabilities (the eval head's softmax) or, with log_probs=True, their logs; f32 and bf16 are read as they are,
    other types go through f32.  Decoding is over the classes as given (no case folding: sum the posterior first, as
    `Lexicon` does).  `beam` hypotheses survive a column (1..64), each column offers its `top_classes` best symbols (1..64).
    Returns a dict of device tensors: ids i32 [N, nbest, T] blank padded, lengths i32 [N, nbest], scores f32 [N, nbest]
    (descending; a lower bound of log p(string | pred), exact when nothing was pruned), count i32 [N] (hypotheses returned; slots
    past it: length 0, score -inf).  One call, no host work that depends on device data (capturable in a graph after one call
    outside); the workspace is a fresh tensor per call."""
    if pred.dim() == 4:
        if pred.shape[2] != 1:
            raise RuntimeError("ctc_beam_search_decode expects [N, C, 1, T]")
        pred = pred.select(2, 0)
    if pred.dim() != 3:
        raise RuntimeError("ctc_beam_search_decode expects [N, C, 1, T] or [N, C, T], got %d dimensions" % pred.dim())
    N, C, T = pred.shape
    defines = _DEFINES
    beam, nbest, top_classes, blank = int(beam), int(nbest), int(top_classes), int(blank)
    if not 1 <= beam <= defines["MR_CTC_BEAM_MAX"]:
        raise ValueError("ctc_beam_search_decode: beam must be in 1..%d, got %d" % (defines["MR_CTC_BEAM_MAX"], beam))
    if not 1 <= nbest <= beam:
        raise ValueError("ctc_beam_search_decode: nbest must be in 1..beam=%d, got %d" % (beam, nbest))
    if not 1 <= top_classes <= defines["MR_CTC_BEAM_TOP_MAX"]:
        raise ValueError("ctc_beam_search_decode: top_classes must be in 1..%d, got %d"
                         % (defines["MR_CTC_BEAM_TOP_MAX"], top_classes))
    if C < 2 or not 0 <= blank < C:
        raise ValueError("ctc_beam_search_decode: blank=%d is not one of C=%d classes (C >= 2)" % (blank, C))
    if not 1 <= T <= defines["MR_SEQ_MEASURE_MAX"]:
        raise ValueError("ctc_beam_search_decode: T=%d columns, 1..%d are taken" % (T, defines["MR_SEQ_MEASURE_MAX"]))
    require_cuda(pred)
    if pred.dtype not in (torch.float32, torch.bfloat16):
        pred = pred.float()
    dev = pred.device
    ids = torch.empty((N, nbest, T), dtype=torch.int32, device=dev)
    lengths = torch.empty((N, nbest), dtype=torch.int32, device=dev)
    scores = torch.empty((N, nbest), dtype=torch.float32, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    out = {'ids': ids, 'lengths': lengths, 'scores': scores, 'count': count}
    if N == 0:
        return out
    nbytes = load().mr_ctc_beam_ws_bytes(N, T, beam, top_classes)
    if nbytes <= 0:
        raise ValueError("ctc_beam_search_decode: N=%d T=%d beam=%d top_classes=%d need a workspace above 2 GiB; split the batch"
                         % (N, T, beam, top_classes))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    sn, sc, st = pred.stride()
    call("mr_ctc_beam_search", 0 if pred.dtype == torch.float32 else 1, ptr(pred), sn, sc, st, N, C, T, int(bool(log_probs)),
         blank, int(unknown), beam, nbest, top_classes, ptr(ids), ptr(lengths), ptr(scores), ptr(count), ptr(ws), ws.numel() * 8)
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
    if pred.dim() == 4:
        if pred.shape[2] != 1:
            raise RuntimeError("ctc_forced_align expects [N, C, 1, T]")
        pred = pred.select(2, 0)
    if pred.dim() != 3:
        raise RuntimeError("ctc_forced_align expects [N, C, 1, T] or [N, C, T], got %d dimensions" % pred.dim())
    N, C, T = pred.shape
    defines = _DEFINES
    blank = int(blank)
    if targets.dim() != 2 or targets.shape[0] != N:
        raise ValueError("ctc_forced_align: targets must be [N=%d, S], got %s" % (N, tuple(targets.shape)))
    if tuple(target_lengths.shape) != (N,):
        raise ValueError("ctc_forced_align: target_lengths must be [N=%d], got %s" % (N, tuple(target_lengths.shape)))
    S = targets.shape[1]
    if S > defines["MR_CTC_ALIGN_MAX_SYMBOLS"]:
        raise ValueError("ctc_forced_align: S=%d symbols per row, 0..%d are taken" % (S, defines["MR_CTC_ALIGN_MAX_SYMBOLS"]))
    if C < 2 or not 0 <= blank < C:
        raise ValueError("ctc_forced_align: blank=%d is not one of C=%d classes (C >= 2)" % (blank, C))
    if not 1 <= T <= defines["MR_SEQ_MEASURE_MAX"]:
        raise ValueError("ctc_forced_align: T=%d columns, 1..%d are taken" % (T, defines["MR_SEQ_MEASURE_MAX"]))
    require_cuda(pred, targets, target_lengths)
    if targets.device != pred.device or target_lengths.device != pred.device:
        raise ValueError("ctc_forced_align: pred is on %s, targets on %s, target_lengths on %s"
                         % (pred.device, targets.device, target_lengths.device))
    if pred.dtype not in (torch.float32, torch.bfloat16):
        pred = pred.float()
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
    nbytes = load().mr_ctc_align_ws_bytes(N, T, S)
    if nbytes <= 0:
        raise ValueError("ctc_forced_align: N=%d T=%d S=%d need a workspace above 2 GiB; split the batch" % (N, T, S))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    sn, sc, st = pred.stride()
    with torch.cuda.device(dev):
        call("mr_ctc_align", 0 if pred.dtype == torch.float32 else 1, ptr(pred), sn, sc, st, N, C, T, int(bool(log_probs)),
             blank, int(unknown), ptr(targets), S, ptr(target_lengths), ptr(out['score']), ptr(out['pos']), ptr(out['begin']),
             ptr(out['end']), ptr(out['sym_lp']), ptr(out['peak']), ptr(ws), ws.numel() * 8)
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
