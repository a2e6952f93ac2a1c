"""ctypes binding of libmegreader_hip.so (the C ABI declared in include/megreader_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C megreader_amd/csrc``).  There is no
CPU fallback: if the shared object is missing or a kernel reports an error, the caller gets an exception.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MEGREADER_HIP_LIB") or os.path.join(_HERE, "csrc", "libmegreader_hip.so")   # tools/ablate_*.py
# point MEGREADER_HIP_LIB at the separate -DMR_ABLATION build
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "megreader_hip.h")

MR_F32 = 0
MR_BF16 = 1

# The binding is DERIVED from the header: the closed tables below are all this file knows about C.  A type that is not in them
# raises -- a silent default (ctypes' own is `int`) would turn a new `long long` into a truncated size.
_PARAM_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
                "hipStream_t": ctypes.c_void_p}
_RETURN_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}


def _ctype(decl, context, array_ok=False):
    """(name, ctypes type, is a hipStream_t) of one parameter `TYPE name` or struct field `TYPE name` / `TYPE name[N]` /
    `TYPE name[N][M]`."""
    m = re.fullmatch(r"(.*?)(\w+)((?:\[\d+\])*)", decl.strip(), re.S)
    base = " ".join(m.group(1).split()) if m else ""
    ctype = ctypes.c_void_p if "*" in base else _PARAM_TYPES.get(base)
    if ctype is None or (m.group(3) and not array_ok):
        raise TypeError("cannot bind %r in `%s`: no ctypes mapping for that type" % (decl.strip(), " ".join(context.split())))
    for n in reversed(re.findall(r"\d+", m.group(3))):             # double top[18][2]: 18 arrays of 2
        ctype = ctype * int(n)
    return m.group(2), ctype, base == "hipStream_t"


def parse_header(text):
    """Read a C-ABI header of this project: ({function: (restype, [argtypes], takes a trailing hipStream_t)},
    {struct: [(field, ctypes type)]}, {integer #define: value}).  Everything that is not a comment, a preprocessor line, the
    extern "C" bracket, a `typedef struct X {...} X;` or a declaration `RET mr_name(PARAMS);` over the closed type tables raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
    structs = {}

    def struct(m):
        fields = structs[m.group(1)] = []
        for stmt in filter(None, (s.strip() for s in m.group(2).split(";"))):
            where = "struct %s { %s; }" % (m.group(1), stmt)
            first, *more = stmt.split(",")                                   # `long long s0, s1, s2, s3`
            name, ctype, _ = _ctype(first, where, True)
            fields.append((name, ctype))
            fields.extend(_ctype(first[:first.rindex(name)] + item, where, True)[:2] for item in more)
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    functions = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        if stmt == "}":                                                      # closes extern "C"
            continue
        m = re.fullmatch(r"(.*?)\b(mr_\w+)\s*\((.*)\)", stmt, re.S)
        ret = re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())) if m else None
        if ret not in _RETURN_TYPES or m.group(2) in functions:
            raise TypeError("cannot bind `%s`: not a declaration `int | long long | const char* mr_name(...)`"
                            % " ".join(stmt.split()))
        params = [] if m.group(3).strip() in ("", "void") else [_ctype(p, stmt) for p in m.group(3).split(",")]
        functions[m.group(2)] = (_RETURN_TYPES[ret], [p[1] for p in params], bool(params) and params[-1][2])
    return functions, structs, defines


def _read_header(path):
    if not os.path.exists(path):
        raise RuntimeError("C ABI header not found at %s -- the ctypes binding is derived from it (there is no fallback table)"
                           % path)
    with open(path) as f:
        return parse_header(f.read())


FUNCTIONS, STRUCTS, _DEFINES = _read_header(HEADER_PATH)
ABI_VERSION = _DEFINES["MR_ABI_VERSION"]
TUNING_FIELDS = tuple(name for name, _ in STRUCTS["mr_tuning"] if name != "reserved")
_STREAMED = frozenset(name for name, (_, _, streamed) in FUNCTIONS.items() if streamed)     # what call() may launch

_lib = None


class Tuning(ctypes.Structure):
    """struct mr_tuning (include/megreader_hip.h): the library's only process-wide switches."""
    _fields_ = STRUCTS["mr_tuning"]


def get_tuning():
    """Current process-wide tuning state as a dict."""
    t = Tuning()
    if load().mr_tuning_get(ctypes.byref(t)) != 0:
        raise RuntimeError("mr_tuning_get failed: %s" % load().mr_last_error().decode())
    return {name: getattr(t, name) for name in TUNING_FIELDS}


def set_tuning(**fields):
    """Replace the named fields of the process-wide tuning state (mr_tuning_set); returns their previous values.  A/B and test
    hook: every field selects between kernels that compute the same result (include/megreader_hip.h)."""
    lib = load()
    t = Tuning()
    if lib.mr_tuning_get(ctypes.byref(t)) != 0:
        raise RuntimeError("mr_tuning_get failed: %s" % lib.mr_last_error().decode())
    old = {}
    for name, value in fields.items():
        if name not in TUNING_FIELDS:
            raise KeyError("mr_tuning has no field %r" % name)
        old[name] = getattr(t, name)
        setattr(t, name, int(value))
    if lib.mr_tuning_set(ctypes.byref(t)) != 0:
        raise RuntimeError("mr_tuning_set failed: %s" % lib.mr_last_error().decode())
    return old


def _install_setter_shims(lib):
    """Rounds 1-3 exported one `mr_set_<field>(value) -> previous value` function per switch; tests and tools still spell their
    A/B toggles that way.  The C ABI now has ONE struct (mr_tuning_get / mr_tuning_set): these are Python callables of the old
    names on the loaded library object, nothing more."""
    def one(field, clamp=None):
        def setter(value):
            value = int(value)
            if clamp is not None and not clamp(value):
                return get_tuning()[field]          # the old setters ignored out-of-range values
            return set_tuning(**{field: value})[field]
        return setter
    lib.mr_set_nt_variant = one("nt_variant", lambda v: v in (1, 2))
    lib.mr_set_nt_deep = one("nt_deep", lambda v: 0 <= v <= 2)
    lib.mr_set_nt_big = one("nt_big", lambda v: -1 <= v <= 13)
    lib.mr_set_nt_p8 = one("nt_p8")
    lib.mr_set_gemm_skinny = lambda v: one("gemm_skinny")(1 if v else 0)
    lib.mr_set_tn_big = one("tn_big", lambda v: -1 <= v <= 2)
    lib.mr_set_tn_buf = one("tn_buf", lambda v: v in (0, 1))
    lib.mr_set_tn_taps = one("tn_taps", lambda v: v in (0, 1))
    lib.mr_set_tn_taps_group = one("tn_taps_group", lambda v: v >= 0)
    lib.mr_set_tn_group = one("tn_group", lambda v: v >= 0)
    lib.mr_set_tn_fin = one("tn_fin", lambda v: v in (0, 2))
    lib.mr_set_tn_taps_fin = one("tn_taps_fin", lambda v: 0 <= v <= 2)
    lib.mr_set_tn_taps_w8 = one("tn_taps_w8", lambda v: v in (0, 1))
    lib.mr_set_tn_model = lambda v: one("tn_model")(1 if v else 0)
    lib.mr_set_tn_splits = lambda v: one("tn_splits")(max(0, int(v)))
    lib.mr_set_bn_fused = one("bn_fused", lambda v: v in (0, 1))
    lib.mr_set_dcn_fused = lambda v: one("dcn_fused")(1 if v else 0)
    lib.mr_set_dcn_v1_bwd = lambda v: one("dcn_v1_bwd")(1 if v else 0)

    def set_lstm_persist(on):
        set_tuning(lstm_persist=int(on) if int(on) in (0, 1, 2) else 1)
        return 0
    lib.mr_set_lstm_persist = set_lstm_persist

    def set_lstm_variant(fwd_bn, bwd_bn):
        f = {}
        if fwd_bn >= 0:
            f["lstm_fwd_bn"] = fwd_bn
        if bwd_bn >= 0:
            f["lstm_bwd_bn"] = bwd_bn
        set_tuning(**f)
        return 0
    lib.mr_set_lstm_variant = set_lstm_variant

    def force_nt_tile(bm, bn):
        set_tuning(nt_force_bm=bm, nt_force_bn=bn if bm else 0)
        return 0
    lib.mr_force_nt_tile = force_nt_tile


def header_symbols():
    """Names of all entry points declared in include/megreader_hip.h."""
    return sorted(FUNCTIONS)


def _bind(lib, functions, optional=False):
    for name, (restype, argtypes, _) in functions.items():
        if optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


def load():
    """Load the shared library (once) and attach the argument types the header declares.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmegreader_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C megreader_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    if lib.mr_abi_version() != ABI_VERSION:             # int mr_abi_version(void): ctypes' defaults are its signature
        raise RuntimeError("%s implements C ABI version %d, this binding expects %d -- rebuild it (`make -C megreader_amd/csrc`)"
                           % (LIB_PATH, lib.mr_abi_version(), ABI_VERSION))
    _bind(lib, FUNCTIONS)
    # only libmegreader_hip_abl.so (tools build) exports what include/megreader_hip_ablation.h declares
    _bind(lib, _read_header(os.path.join(os.path.dirname(HEADER_PATH), "megreader_hip_ablation.h"))[0], optional=True)
    _install_setter_shims(lib)
    _lib = lib
    if torch.cuda.is_available():
        if lib.mr_init() != 0:
            raise RuntimeError("mr_init failed: %s" % lib.mr_last_error().decode())
    elif lib.mr_init() != 0:
        # no GPU (build container, host-only queries such as mr_nt_kernel_code): mr_init still applies MEGREADER_TUNING before
        # it touches the device, so a malformed variable is reported here too; the device part failing is expected
        err = lib.mr_last_error().decode()
        if "MEGREADER_TUNING" in err:
            raise RuntimeError("mr_init failed: %s" % err)
    return lib


def dtype_code(dtype):
    if dtype == torch.float32:
        return MR_F32
    if dtype == torch.bfloat16:
        return MR_BF16
    raise TypeError("megreader_amd kernels support float32 and bfloat16, got %s" % dtype)


def vec_of(dtype):
    return 4 if dtype == torch.float32 else 8


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


class KernelTimer(object):
    """Optional HIP-event bracketing of selected C-ABI calls on the stream they are launched on (bench.py uses it
    to measure the dominant kernel's launch durations live inside the timed region)."""

    def __init__(self, names, track_deferred=False):
        self.names = set(names)
        self.records = []  # (name, args, start_event, end_event)
        # track_deferred: calls that the library only RECORDS (mr_tn_defer: deferred weight-gradient problems) are collected and
        # attributed to the mr_tn_flush that launches them as one grouped kernel -- ("mr_tn_flush", [(name, args), ...], e0, e1)
        self.track_deferred = track_deferred
        self.deferred = []

    def results(self):
        """[(name, args, milliseconds)] -- call after torch.cuda.synchronize()."""
        return [(n, a, s.elapsed_time(e)) for n, a, s, e in self.records]


TIMER = None  # set to a KernelTimer to enable

_TN_WS = {}
_TN_WS_CALLS = frozenset(("mr_gemm_tn", "mr_gemm_tn2", "mr_conv2d_wgrad", "mr_conv2d_wgrad_tab",
                          # (the split reduction of the NT kernels, mr_tuning.nt_ksplit, uses the same workspace)
                          "mr_conv2d_fwd", "mr_conv2d_fwd_stats", "mr_conv2d_dgrad", "mr_conv2d_dgrad_add", "mr_conv2d_dgrad_bnb",
                          "mr_gemm_nt"))


def ensure_tn_workspace(device=None):
    """Register (once per device) the workspace of the weight-gradient kernels' in-launch split reduction
    (mr_set_tn_taps_workspace): 16 KB of tickets + one 147456-byte slab per workgroup of a full launch (2 per CU; the grouped
    all-taps launches of mr_tn_flush are planned to fit the same slabs).  Launches that use it must be stream-ordered with each
    other."""
    if device is None:
        idx = torch.cuda.current_device()
    else:
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
    ws = _TN_WS.get(idx)
    if ws is None:
        lib = load()
        cus = torch.cuda.get_device_properties(idx).multi_processor_count
        nbytes = 16384 + (2 * cus + 64) * 147456
        ws = _TN_WS[idx] = torch.zeros(nbytes, dtype=torch.uint8, device=torch.device("cuda", idx))
        with torch.cuda.device(idx):   # the library keeps one workspace per device, keyed by the current device
            rc = lib.mr_set_tn_taps_workspace(ws.data_ptr(), nbytes)
        if rc != 0:
            raise RuntimeError("mr_set_tn_taps_workspace failed: %s" % lib.mr_last_error().decode())
    return ws


def _bracketed(fn, args):
    """fn(*args, stream) between two timing events on the current stream: (return code, start event, end event)."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn(*args, stream_ptr())
    e1.record()
    return rc, e0, e1


def call(name, *args):
    """Invoke a C entry point on torch's current HIP stream; raise RuntimeError on a non-zero return code."""
    if name not in _STREAMED:
        raise TypeError("%s is not an entry point with a trailing hipStream_t (include/megreader_hip.h): call() appends the "
                        "stream; call host-only functions as load().%s(...)" % (name, name))
    lib = load()
    if name in _TN_WS_CALLS and torch.cuda.current_device() not in _TN_WS:
        ensure_tn_workspace()
    timer = TIMER
    if timer is not None and name in timer.names:
        pend = lib.mr_tn_pending() if timer.track_deferred else 0
        rc, e0, e1 = _bracketed(getattr(lib, name), args)
        if timer.track_deferred and lib.mr_tn_pending() > pend:
            timer.deferred.append((name, args))          # recorded, not launched: its time is the flush's
        else:
            timer.records.append((name, args, e0, e1))
    elif timer is not None and timer.track_deferred and name == "mr_tn_flush" and timer.deferred:
        group, timer.deferred = timer.deferred, []
        rc, e0, e1 = _bracketed(getattr(lib, name), args)
        timer.records.append(("mr_tn_flush", group, e0, e1))
    else:
        rc = getattr(lib, name)(*args, stream_ptr())
    if rc != 0:
        raise RuntimeError("%s failed (code %d): %s" % (name, rc, lib.mr_last_error().decode()))


def dcn_workspace(dtype, N, H, W, C, Co, kh, kw, Ho, Wo, backward, device):
    """Caller-owned workspace of mr_dcn2_fwd / mr_dcn2_bwd (include/megreader_hip.h: mr_dcn2_ws_bytes): None when the
    fused forward needs none, else an uninitialised byte buffer (CSR of the scatter pattern / column matrix)."""
    n = load().mr_dcn2_ws_bytes(dtype_code(dtype), N, H, W, C, Co, kh, kw, Ho, Wo, 1 if backward else 0)
    if n <= 0:
        return None
    return torch.empty((n,), dtype=torch.uint8, device=device)


_DCN_WS = {}


def dcn_backward_workspace(dtype, N, H, W, C, Co, kh, kw, Ho, Wo, device):
    """(workspace, flags) for mr_dcn2_bwd2.  Fused path: ONE persistent buffer per geometry, zeroed when it is created -- the CSR
    build returns its counters to zero by itself, so later calls pass flags bit 0 and no memset node runs in front of them (13
    DCN layers per detector step; layers of one geometry share the buffer, stream-ordered).  General path: a fresh buffer, 0."""
    if not load().mr_dcn2_fused(dtype_code(dtype), H, W, C, Co, kh, kw):
        return dcn_workspace(dtype, N, H, W, C, Co, kh, kw, Ho, Wo, True, device), 0
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), dtype, N, H, W, C, Co, kh, kw, Ho, Wo)
    ws = _DCN_WS.get(key)
    if ws is None:
        n = load().mr_dcn2_ws_bytes(dtype_code(dtype), N, H, W, C, Co, kh, kw, Ho, Wo, 1)
        # (never evicted: captured hipGraphs hold raw pointers into these buffers -- ADVICE r5; one entry per layer geometry)
        ws = _DCN_WS[key] = torch.zeros((max(int(n), 16),), dtype=torch.uint8, device=dev)
    return ws, 1


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError(
                "megreader_amd ops run only on an AMD GPU (HIP); got a %s tensor. There is no CPU fallback." % t.device)
