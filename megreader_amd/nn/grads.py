"""Gradient plumbing of the autograd layer; nn/functional.py re-exports every name here.  The gradient-sink protocol of the fused
optimizers (grad_sink, notify_grad_ready, GradDest), the pre-zeroed scratch arena and batched fills shared with `zero_grad()`, and
the deferred, grouped weight-gradient launches (_TnDefer, _wgrad).  All state lives on the classes."""
import contextlib
import ctypes
import os

import torch

from .._lib import call, load


def grad_sink(param, physical_shape=None):
    """Gradient sink protocol.  megreader_amd.optim attaches to every parameter it owns a persistent f32 view of its
    flat gradient buffer (`param._mr_grad_sink`, also installed as `param.grad`).  Backward kernels that accumulate
    (`+=`) anyway -- the split-P wgrad GEMMs and column sums -- write straight into that view and the autograd
    Function returns None for the parameter: no temporary gradient, no zero-fill, no `grad += tmp` kernel.
    Returns the sink tensor if it exists and its memory is dense in the layout the kernel writes
    (`physical_shape`: e.g. KRSC for a channels_last OIHW conv weight), else None (normal autograd path)."""
    sink = getattr(param, "_mr_grad_sink", None)
    if sink is None or sink.dtype != torch.float32 or not sink.is_cuda:
        return None
    # only while the sink IS param.grad: after `model.zero_grad()` (grad=None) or a user-assigned .grad the normal
    # autograd accumulation path must run, otherwise stale sums would survive in the flat buffer
    if param.grad is None or param.grad.data_ptr() != sink.data_ptr():
        return None
    if physical_shape == "strided":   # the kernel takes explicit strides
        return sink
    if physical_shape is not None:
        if len(physical_shape) == 4:
            phys = sink.permute(0, 2, 3, 1)
            if tuple(phys.shape) != tuple(physical_shape) or not phys.is_contiguous():
                return None
        elif tuple(sink.shape) != tuple(physical_shape) or not sink.is_contiguous():
            return None
    elif not sink.is_contiguous():
        return None
    return sink


def notify_grad_ready(param):
    """Tell data-parallel wrappers that `param`'s gradient was accumulated through its sink (the autograd
    post-accumulate hook does not fire when a Function returns None)."""
    for hook in getattr(param, "_mr_grad_ready_hooks", ()):
        hook(param)


class GradDest(object):
    """Where the gradient of ONE parameter goes in a backward pass, in two phases.  Construction looks the sink up (grad_sink;
    only when a gradient is wanted); a call site may still drop it (`d.sink = None`) for a rule of its own.  `into(fallback)`
    then fixes the buffer the kernel accumulates into: the sink, else `fallback()` -- a ZEROED scratch of the caller's (its own
    torch.zeros or a slice of a shared zero fill; never a ZeroArena slice: it becomes somebody's .grad) --, None when no gradient
    is wanted.  After the launch `grad(view)` is what autograd gets (None when sunk or unwanted, else view(buffer)) and `notify()`
    reports a sunk parameter ready (not after a launch that _wgrad recorded: the flush does that)."""
    __slots__ = ("param", "want", "sink", "buf")

    def __init__(self, param, want, physical_shape=None):
        self.param, self.want, self.buf = param, bool(want), None
        self.sink = grad_sink(param, physical_shape) if self.want else None

    @property
    def sunk(self):
        return self.sink is not None

    def into(self, fallback):
        if self.want:
            self.buf = self.sink if self.sink is not None else fallback()
        return self.buf

    def grad(self, view=None):
        if not self.want or self.sink is not None:
            return None
        return self.buf if view is None else view(self.buf)

    def notify(self):
        if self.sink is not None:
            notify_grad_ready(self.param)


class ZeroArena(object):
    """Pre-zeroed f64 scratch for the per-channel reduction buffers of BatchNorm (mr_bn_scratch_doubles(C) per call,
    forward and backward).  Each call used to zero its own buffer with a memset (120 tiny launches per ResNet-50 step).  Slices
    are handed out once per zeroing by a bump pointer; `reset()` -- called by the fused optimizers' `zero_grad()` --
    re-zeroes the used prefix with ONE fill and rewinds.  When the arena is exhausted (nobody calls reset: eval
    loops, foreign optimizers) `take` returns None and the caller falls back to its own memset."""
    SIZE = 1 << 24  # doubles (128 MB: the offset / mask gradients of the 13 DCN layers of a detector step take ~32 MB; ResNet-50 takes ~34 doubles per BN channel per step, ~1 M; the four persistent-LSTM
                    # exchange rings of a CRNN step 3.2 M)
    arenas = {}

    def __init__(self, device):
        self.buf = torch.zeros((ZeroArena.SIZE,), dtype=torch.float64, device=device)
        self.offset = 0

    @staticmethod
    def take(device, n):
        a = ZeroArena.arenas.get(device)
        if a is None:
            a = ZeroArena.arenas[device] = ZeroArena(device)
        n = (n + 31) // 32 * 32
        if a.offset + n > ZeroArena.SIZE:
            return None
        out = a.buf[a.offset:a.offset + n]
        a.offset += n
        return out

    @staticmethod
    def reset(device):
        a = ZeroArena.arenas.get(device)
        if a is not None and a.offset:
            a.buf[:a.offset].zero_()
            a.offset = 0

    @staticmethod
    def rewind(device):
        """(data pointer, bytes) of the used prefix -- which the CALLER zeroes (zero_tensors: one launch together with the flat
        gradient buffers) -- and rewind; None when nothing was handed out."""
        a = ZeroArena.arenas.get(device)
        if a is None or not a.offset:
            return None
        used = a.offset
        a.offset = 0
        return a.buf.data_ptr(), used * 8


def zero_segments(segments):
    """Zero fill of (data pointer, bytes) pairs, 8 per launch (mr_zero_multi); 16-byte aligned, sizes multiples of 16."""
    for i in range(0, len(segments), 8):
        chunk = segments[i:i + 8]
        n = len(chunk)
        call("mr_zero_multi", n, (ctypes.c_void_p * n)(*[p for p, _ in chunk]), (ctypes.c_longlong * n)(*[b for _, b in chunk]))


def accumulate_multi(pairs):
    """dst += src for a list of (dst, src) dense f32 tensor pairs, 8 pairs per launch (mr_accumulate_multi)."""
    for i in range(0, len(pairs), 8):
        chunk = pairs[i:i + 8]
        n = len(chunk)
        dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in chunk])
        src = (ctypes.c_void_p * n)(*[s.data_ptr() for _, s in chunk])
        cnt = (ctypes.c_longlong * n)(*[s.numel() for _, s in chunk])
        call("mr_accumulate_multi", n, dst, src, cnt)


class _TnDefer(object):
    """Deferred, grouped weight-gradient launches (include/megreader_hip.h: mr_tn_defer / mr_tn_flush).  Nothing later in a
    backward pass reads a weight gradient that goes to a gradient sink, so the small weight-gradient GEMMs (ResNet 1x1 / strided
    layers, LSTM / Linear layers) and the 3x3 layers of the all-taps kernel (conv2..conv5 of the CRNN, the ResNet bottlenecks)
    are recorded while backward runs and launched several problems per launch: at the latest from
    an autograd-engine callback at the end of the backward pass, earlier as soon as one of the two kernels has a full launch
    waiting (mr_tn_capacity: 16 problems of the 128x128 TN GEMM kernel, dense and conv together, or 12 of the all-taps kernel),
    so that a deep network does not keep every layer's operands until the end.  The CRNN step records 13 + 4 and flushes once.
    The operands of the recorded problems are kept alive here until the flush; parameters are reported to data-parallel
    wrappers (notify_grad_ready) only after the launch that completes their gradient.  A node may flush earlier itself when
    such a wrapper listens to its parameters (listening(); BiLSTMFn.backward): without one nothing reads a gradient before the
    optimizer, and on the single backward stream an early flush overlaps nothing -- it only costs a launch.
    The flush runs under the device of the kept operands: the end-of-backward callback runs on the thread that called
    backward(), whose current device may be another one than the model's, and the library's queue is per device.
    MEGREADER_TN_DEFER=0 (or mr_tuning.tn_defer = 0): every launch immediate (A/B).
    Every launch stays on the backward stream: forking weight-gradient launches onto side streams was measured slower in
    every step (CHANGELOG.md, "Retired: the side-stream weight-gradient switches")."""
    enabled = os.environ.get("MEGREADER_TN_DEFER", "1") != "0"
    keep = []
    notify = []
    queued = False
    task = -1      # graph task (one backward() call) the end-of-backward callback is registered with
    mark = 0

    @staticmethod
    def _task_id():
        fn = getattr(torch._C, "_current_graph_task_id", None)
        return fn() if fn is not None else -1

    @staticmethod
    def abort():
        """Forget everything recorded and not yet launched: the backward pass that recorded it raised -- the autograd
        engine skips its final callbacks then, so `queued` would stay set, the records would point at operands about to be
        released and a later step would add stale problems into its gradients.  Called from the recording sites when a call
        between begin() and end() raises, from begin() when it finds the state of ANOTHER graph task, and from the optimizers'
        zero_grad() / the capture fallbacks of the graphed step."""
        lib = load()
        lib.mr_tn_defer(0)
        lib.mr_tn_discard()
        del _TnDefer.keep[:]
        del _TnDefer.notify[:]
        _TnDefer.queued = False
        _TnDefer.task = -1

    @staticmethod
    def begin():
        """Start recording for the calls that follow (until end()); False when deferral is not possible here (switched off,
        or not inside a backward pass -- the end-of-backward flush could not be registered)."""
        if not _TnDefer.enabled:
            return False
        tid = _TnDefer._task_id()
        if _TnDefer.queued and tid != _TnDefer.task:
            _TnDefer.abort()          # left over from a backward pass that never reached its callback
        if not _TnDefer.queued:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(_TnDefer.flush)
            except RuntimeError:
                return False
            _TnDefer.queued = True
            _TnDefer.task = tid
        lib = load()
        _TnDefer.mark = lib.mr_tn_pending()
        lib.mr_tn_defer(1)
        return True

    @staticmethod
    def record(launch, tensors, params):
        """begin() was True: run `launch` (the library calls to record) and end(); a raise in between drops the recording state
        instead of leaving mr_tn_defer(1) on for whatever this thread launches next."""
        try:
            launch()
        except BaseException:
            _TnDefer.abort()
            raise
        return _TnDefer.end(tensors, params)

    @staticmethod
    def end(tensors, params):
        """Stop recording.  True when the calls since begin() were recorded (the caller must then NOT report its parameters
        ready: the flush does); False when the library launched them at once (f32, mr_tuning.tn_defer = 0 or tn_splits != 0)."""
        lib = load()
        lib.mr_tn_defer(0)
        if lib.mr_tn_pending() == _TnDefer.mark:
            return False
        _TnDefer.keep.extend(t for t in tensors if t is not None)
        _TnDefer.notify.extend(params)
        if any(lib.mr_tn_pending_of(kind) >= lib.mr_tn_capacity(kind) for kind in (0, 1)):
            _TnDefer.flush(final=False)
        return True

    @staticmethod
    def listening(params):
        """True when a data-parallel wrapper waits for the gradient of one of `params` (its hooks fire from notify_grad_ready)."""
        return any(getattr(p, "_mr_grad_ready_hooks", None) for p in params)

    @staticmethod
    def flush(final=True):
        """Launch what is recorded and report its parameters ready; final: the end-of-backward callback of the graph task."""
        dev = next((t.device for t in _TnDefer.keep if t.is_cuda), None)
        with (torch.cuda.device(dev) if dev is not None else contextlib.nullcontext()):     # nothing kept: nothing recorded
            if load().mr_tn_pending():
                call("mr_tn_flush")
        ready, _TnDefer.notify = _TnDefer.notify, []
        del _TnDefer.keep[:]
        if final:
            _TnDefer.queued = False
            _TnDefer.task = -1
        for p in ready:
            notify_grad_ready(p)


def _wgrad(launch, may_defer, keep, params, immediate=None):
    """The weight-gradient launch of one layer.  may_defer (every gradient it writes goes to a sink) and _TnDefer.begin()
    succeeds: `launch` under recording, `keep` alive and `params` reported ready by the flush; True when the problems were
    really recorded.  Otherwise `immediate` (default: `launch`) now and False: the caller reports its parameters itself."""
    if may_defer and _TnDefer.begin():
        return _TnDefer.record(launch, keep, params)
    (immediate or launch)()
    return False


def discard_deferred_wgrads():
    """Drop every recorded, not yet launched weight-gradient problem (a backward pass that raised; a failed capture)."""
    _TnDefer.abort()


def flush_deferred_wgrads():
    """Launch every recorded weight-gradient problem now (data-parallel wrappers call this before they finalise a backward
    pass; harmless when nothing is recorded)."""
    _TnDefer.flush(final=False)
