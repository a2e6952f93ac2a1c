"""1-D CTC with a wide alphabet (5 360 classes, csrc/ctc.hip: mr_ctc_wide) on the GPU, device events throughout.
  python tools/microbench_ctc_wide.py [--parent-lib PATH] [--out FILE] [--sections 1,2,4,5]

  1  mr_ctc_fwd and mr_ctc_bwd (the two calls behind F.ctc_loss_logits), separately: time, bytes from shapes / time, share of the
     achievable HBM rate
  2  forward A/B against a libmegreader_hip.so built from the parent commit (--parent-lib), alternating, with the outputs compared
  4  one CRNN training pass (forward + backward, eager) at N = 256, 32x128, bf16 with 5 360 and with 38 classes, and the share of the
     classifier GEMMs and of the CTC kernels
  5  softmax_eval_nc1t and ctc_greedy_decode
Every figure is the median over ROUNDS rounds of REPS calls with the smallest and the largest round behind it (the spread)."""
import argparse
import ctypes
import statistics
import sys

import torch

sys.path.insert(0, ".")
import megreader_amd as mr  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr  # noqa: E402
from megreader_amd.nn import functional as F  # noqa: E402

HBM = 6.3e12          # achievable bytes / s (MI355X: 8 TB/s peak)
ROUNDS, REPS = 7, 20
SHAPES = [(33, 256, 5360, 32, torch.bfloat16), (26, 16, 5360, 32, torch.float32)]
DEV = "cuda"
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def one_round(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per call


def rounds(*fns, reps=REPS):
    """[us per call] per function, the functions alternating round by round after a warm-up of each"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            out[i].append(one_round(fn, reps))
    return out


def fmt(us):
    return "%8.1f us (min %.1f, max %.1f)" % (statistics.median(us), min(us), max(us))


def problem(T, N, C, S, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, N, C, generator=g) * 2).to(dtype).to(DEV)
    lengths = torch.randint(3, 11, (N,), generator=g)
    targets = torch.zeros(N, S, dtype=torch.int32)
    for i, L in enumerate(lengths.tolist()):
        targets[i, :L] = torch.randint(2, C, (L,), generator=g, dtype=torch.int32)
    return logits, targets.to(DEV), lengths.to(DEV)


def esize(dtype):
    return 4 if dtype == torch.float32 else 2


def buffers(T, N, C, S):
    return dict(lp=torch.empty((T, N, C), dtype=torch.float32, device=DEV),
                lp64=torch.empty((T, N, C), dtype=torch.float64, device=DEV),
                alpha=torch.empty((N, T, 2 * S + 1), dtype=torch.float64, device=DEV),
                beta=torch.empty((N, T, 2 * S + 1), dtype=torch.float64, device=DEV),
                nll=torch.empty((N,), dtype=torch.float64, device=DEV),
                loss=torch.empty((), dtype=torch.float64, device=DEV))


def fwd_args(b, logits, targets, in_len, lengths, T, N, C, S):
    return (dtype_code(logits.dtype), ptr(logits), C, ptr(targets), 0, ptr(in_len), ptr(lengths), 1, T, N, C, S, 0, 1, ptr(b["lp"]),
            ptr(b["alpha"]), ptr(b["beta"]), ptr(b["nll"]), ptr(b["loss"]), ptr(b["lp64"]))


def section_1():
    say("== 1. the two C-ABI calls behind F.ctc_loss_logits at 5 360 classes: mr_ctc_fwd (lp and lp64 written) and mr_ctc_bwd")
    for T, N, C, S, dtype in SHAPES:
        logits, targets, lengths = problem(T, N, C, S, dtype)
        assert _lib.load().mr_ctc_wide(C, S) == 1
        in_len = torch.full((N,), T, dtype=torch.int64, device=DEV)
        lengths = lengths.long()
        b = buffers(T, N, C, S)
        grad = torch.empty((T, N, C), dtype=dtype, device=DEV)
        gout = torch.ones((), dtype=torch.float64, device=DEV)

        def fwd():
            call("mr_ctc_fwd", *fwd_args(b, logits, targets, in_len, lengths, T, N, C, S))

        def bwd():
            call("mr_ctc_bwd", dtype_code(dtype), ptr(b["lp"]), ptr(b["alpha"]), ptr(b["beta"]), ptr(b["nll"]), ptr(targets), 0,
                 ptr(in_len), ptr(lengths), 1, ptr(gout), T, N, C, S, 0, 1, ptr(grad), C)

        f_us, = rounds(fwd)
        b_us, = rounds(bwd)
        n = T * N * C
        fb, bb = n * (esize(dtype) + 4 + 8), n * (4 + esize(dtype))
        for name, us, nbytes in (("forward ", f_us, fb), ("backward", b_us, bb)):
            rate = nbytes / (statistics.median(us) * 1e-6)
            say("  (%d, %d, %d, %d) %-8s %s: %s  %6.1f MB -> %.2f TB/s = %4.1f %% of %.1f TB/s" %
                (T, N, C, S, str(dtype).replace("torch.", ""), name, fmt(us), nbytes / 1e6, rate / 1e12, 100 * rate / HBM, HBM / 1e12))


def bind_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("mr_ctc_fwd", "mr_init", "mr_last_error"):
        restype, argtypes, _ = _lib.FUNCTIONS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.mr_init() != 0:
        raise RuntimeError("parent library: mr_init failed: %s" % lib.mr_last_error().decode())
    return lib


def section_2(parent_path):
    say("== 2. mr_ctc_fwd A/B at 5 360 classes: this tree (row-parallel log-softmax + recursion) | parent commit (softmax inside the "
        "per-sample kernel), alternating")
    parent = bind_parent(parent_path)
    verdict = []
    for T, N, C, S, dtype in SHAPES:
        logits, targets, lengths = problem(T, N, C, S, dtype)
        in_len = torch.full((N,), T, dtype=torch.int64, device=DEV)
        lengths = lengths.long()
        bufs = {"new": buffers(T, N, C, S), "old": buffers(T, N, C, S)}

        def args(b):
            return fwd_args(b, logits, targets, in_len, lengths, T, N, C, S)

        def new():
            call("mr_ctc_fwd", *args(bufs["new"]))

        def old():
            rc = parent.mr_ctc_fwd(*args(bufs["old"]), _lib.stream_ptr())
            if rc != 0:
                raise RuntimeError("parent mr_ctc_fwd failed: %s" % parent.mr_last_error().decode())

        new_us, old_us = rounds(new, old)
        dlp = float((bufs["new"]["lp"] - bufs["old"]["lp"]).abs().max())
        dnll = float(((bufs["new"]["nll"] - bufs["old"]["nll"]).abs() / bufs["old"]["nll"].abs().clamp(min=1)).max())
        say("  (%d, %d, %d, %d) %-8s new %s | parent %s | x%.2f   max |lp - lp_parent| %.2e, nll rel %.2e" %
            (T, N, C, S, str(dtype).replace("torch.", ""), fmt(new_us), fmt(old_us),
             statistics.median(old_us) / statistics.median(new_us), dlp, dnll))
        verdict.append(max(new_us) < min(old_us))
    say("  the row-parallel log-softmax is faster than the parent beyond the spread at both shapes: %s" % all(verdict))


def section_4():
    say("== 4. CRNN forward + backward (eager, no optimizer), N = 256, 32x128, bf16: 5 360 classes next to 38")
    from megreader_amd.backbones import crnn_backbone
    from megreader_amd.charsets import Charset, EnglishCharset
    from megreader_amd.decoders import CRNNDecoder
    from oracle.crnn import synthetic_batch
    mr.set_compute_dtype(torch.bfloat16)
    for classes in (5360, 38):
        charset = EnglishCharset() if classes == 38 else Charset([chr(0x4E00 + i) for i in range(classes - 2)])
        torch.manual_seed(0)
        backbone, decoder = crnn_backbone().to(DEV).train(), CRNNDecoder(charset=charset, in_channels=512).to(DEV).train()
        batch = synthetic_batch(256, 32, 128, seed=0, num_classes=classes)
        img, lab, ln = batch['image'].to(DEV), batch['label'].to(DEV), batch['length'].to(DEV).long()
        params = list(backbone.parameters()) + list(decoder.parameters())

        def step():
            for p in params:
                p.grad = None
            loss, _ = decoder(backbone(img), targets=lab, lengths=ln, train=True)
            loss.mean().backward()

        us, = rounds(step, reps=5)
        _lib.TIMER = timer = _lib.KernelTimer(("mr_ctc_fwd", "mr_ctc_bwd", "mr_gemm_nt", "mr_gemm_tn"))
        step()
        torch.cuda.synchronize()
        _lib.TIMER = None
        cp = -(-classes // 8) * 8
        gemm = sum(ms for n, a, ms in timer.results() if n.startswith("mr_gemm") and (classes in a or cp in a))
        ctc = {n: sum(ms for n2, _, ms in timer.results() if n2 == n) for n in ("mr_ctc_fwd", "mr_ctc_bwd")}
        tot = statistics.median(us) / 1e3
        flop = 3 * 2 * 8448 * classes * 512
        say("  %4d classes: %s   classifier GEMMs (3 passes, %.1f GFLOP) %.3f ms = %.1f %%   mr_ctc_fwd %.3f ms = %.1f %%   "
            "mr_ctc_bwd %.3f ms = %.1f %%   (bracketed calls of one extra pass)" %
            (classes, fmt(us), flop / 1e9, gemm, 100 * gemm / tot, ctc["mr_ctc_fwd"], 100 * ctc["mr_ctc_fwd"] / tot,
             ctc["mr_ctc_bwd"], 100 * ctc["mr_ctc_bwd"] / tot))


def section_5():
    say("== 5. eval side at 5 360 classes: softmax_eval_nc1t and ctc_greedy_decode (record only)")
    from megreader_amd.ops.decode import ctc_greedy_decode
    for T, N, C, _, dtype in SHAPES:
        logits, _, _ = problem(T, N, C, 32, dtype)
        probs = F.softmax_eval_nc1t(logits)
        s_us, d_us = rounds(lambda: F.softmax_eval_nc1t(logits), lambda: ctc_greedy_decode(probs))
        n = T * N * C
        say("  (%d, %d, %d) %-8s softmax_eval_nc1t %s = %.2f TB/s of (logits read + f32 written)   ctc_greedy_decode %s = %.2f TB/s "
            "of f32 read" % (T, N, C, str(dtype).replace("torch.", ""), fmt(s_us),
                             n * (esize(dtype) + 4) / (statistics.median(s_us) * 1e-6) / 1e12, fmt(d_us),
                             n * 4 / (statistics.median(d_us) * 1e-6) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--sections", default="1,2,4,5")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_ctc_wide.py measures on the GPU; there is none")
    _lib.load()
    say("%s, %d rounds of %d calls per figure" % (torch.cuda.get_device_name(0), ROUNDS, REPS))
    want = set(a.sections.split(","))
    if "1" in want:
        section_1()
    if "2" in want:
        if not a.parent_lib:
            raise SystemExit("section 2 needs --parent-lib (libmegreader_hip.so built from the parent commit)")
        section_2(a.parent_lib)
    if "4" in want:
        section_4()
    if "5" in want:
        section_5()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
