"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol the header declares,
the ctypes binding derived from the header agrees with it position by position, module parameters mirror the
reference's state_dict, and the product path refuses CPU tensors instead of silently falling back."""
import ctypes
import os
import re

import pytest
import torch

from megreader_amd import _lib


I, L, P, F, D = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_float, ctypes.c_double


def _header_code():
    """The header without comments and struct bodies -- this file's own reading, independent of _lib.parse_header."""
    with open(_lib.HEADER_PATH) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", code, flags=re.S)


def test_library_exports_every_header_symbol():
    lib = _lib.load()
    syms = _lib.header_symbols()
    # no declaration is skipped, whatever it returns: one name per `mr_xxx(` of the header
    assert len(syms) == len(set(syms)) == len(re.findall(r"mr_\w+\s*\(", _header_code())) >= 130
    for s in syms:
        assert hasattr(lib, s), "libmegreader_hip.so does not export %s" % s
    assert lib.mr_abi_version() == 3 == _lib.ABI_VERSION


LONG_LONG_FUNCTIONS = {"mr_db_loss_ws_bytes", "mr_bn_scratch_doubles", "mr_stem_bwd_workspace", "mr_lstm_ws_bytes",
                       "mr_dcn2_ws_bytes", "mr_decode_persist_ws_bytes", "mr_decode_persist_bwd_ws_bytes"}


def test_bound_signatures_match_header():
    """restype and argtypes of EVERY entry point of the loaded library, host-only ones included, against the declaration text."""
    lib = _lib.load()
    code = _header_code()
    seen_long_long = set()
    for name in _lib.header_symbols():
        found = re.findall(r"\b(int|long long|const char\s*\*)\s*%s\s*\(([^;]*?)\)\s*;" % name, code, re.S)
        assert len(found) == 1, name
        ret, decl = found[0]
        fn = getattr(lib, name)
        if ret == "long long":
            seen_long_long.add(name)
            assert fn.restype is L, name
        else:
            assert fn.restype is (I if ret == "int" else ctypes.c_char_p), name
        params = [] if decl.strip() in ("", "void") else [a.strip() for a in decl.split(",")]
        assert len(params) == len(fn.argtypes), (name, len(params), len(fn.argtypes))
        # pointer / integer / float kinds agree position by position
        for bound, arg in zip(fn.argtypes, params):
            if "*" in arg or arg.startswith("hipStream_t"):
                assert bound is P, (name, arg)
            elif arg.startswith("long long"):
                assert bound is L, (name, arg)
            elif arg.startswith("float"):
                assert bound is F, (name, arg)
            elif arg.startswith("double"):
                assert bound is D, (name, arg)
            else:
                assert arg.startswith("int ") and bound is I, (name, arg)
    assert seen_long_long == LONG_LONG_FUNCTIONS
    assert lib.mr_last_error.restype is ctypes.c_char_p


# full signatures written out by hand: every parameter type, the longest declarations, every formerly unchecked class
PINNED = {
    "mr_gemm_nt": (I, [I, P, L, P, I, P, L, P, I, I, I, I, P]),
    "mr_dcn2_bwd3": (I, [I, P, P, P, P, L, P, L, P, P, P, I, P, P, P, P, P] + [I] * 12 + [P]),
    "mr_decode_persist_fwd": (I, [P, P, P, L, P, L, P, P, P, P, I] + [P] * 9 + [L, I, I, I, I, P]),
    "mr_resize_normalize": (I, [P, P, I, I, I, D, D, D, P, P]),
    "mr_db_loss_fwd": (I, [P] * 10 + [I, L, F, F, F, F, P]),
    "mr_dcn2_ws_bytes": (L, [I] * 11),
    "mr_conv2d_fwd_pool_ok": (I, [I] * 23),
    "mr_phase_read": (I, [I, P, P]),
    "mr_tn_pending": (I, []),
    "mr_last_error": (ctypes.c_char_p, []),
    "mr_tuning_set": (I, [P]),
    "mr_set_tn_taps_workspace": (I, [P, L]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    fn = getattr(_lib.load(), name)
    restype, argtypes = PINNED[name]
    assert fn.restype is restype
    assert list(fn.argtypes) == argtypes


def test_reader_refuses_what_it_does_not_know():
    ok = _lib.parse_header("int mr_x(int v, hipStream_t stream);\nlong long mr_y(void);")[0]
    assert ok == {"mr_x": (I, [I, P], True), "mr_y": (L, [], False)}
    for bad in ("int mr_x(unsigned short v, hipStream_t stream);",      # unknown parameter type
                "float mr_x(int v);",                                   # unknown return type
                "int mr_x(int);",                                       # no parameter name: nothing says `int` is the type
                "int mr_x(int v[4]);",                                  # arrays only in structs
                "typedef struct mr_s { short a; } mr_s;",               # unknown field type
                "int mr_x(int v); int mr_x(long long v);",              # declared twice
                "static int helper(int v);"):                           # not an entry point
        with pytest.raises(TypeError) as e:
            _lib.parse_header(bad)
        assert "mr_" in str(e.value) or "helper" in str(e.value)        # the declaration is in the message


def test_call_refuses_entry_points_without_a_stream(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("call() reached the library"))
    for name in ("mr_tn_pending", "mr_dcn2_ws_bytes", "mr_no_such_function"):
        with pytest.raises(TypeError):
            _lib.call(name)


def test_pointer_parameters_take_byref_and_integers_refuse_floats():
    lib = _lib.load()
    ms, work = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    assert lib.mr_phase_timer(0) in (0, 1)
    assert lib.mr_phase_read(0, ctypes.byref(ms), ctypes.byref(work)) == 0     # timer off: no records
    assert (ms.value, work.value) == (0.0, 0.0)
    t = _lib.Tuning()
    assert lib.mr_tuning_get(ctypes.byref(t)) == 0 and t.nt_variant in (1, 2)
    with pytest.raises(ctypes.ArgumentError):
        lib.mr_nt_tile_code(128.0, 128)


def test_no_torch_types_in_header():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # strip comments
    assert "torch" not in code.lower() and "at::" not in code and "Tensor" not in code


def test_modules_mirror_reference_state_dict(golden_dir):
    from megreader_amd.backbones import crnn_backbone
    from megreader_amd.decoders import CRNNDecoder
    golden = torch.load(os.path.join(golden_dir, "crnn_golden.pt"), weights_only=False)

    class BasicModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = crnn_backbone()
            self.decoder = CRNNDecoder(in_channels=512)

    torch.manual_seed(golden['weight_seed'])
    m = BasicModel()
    state = m.state_dict()
    assert list(state.keys()) == golden['state_keys']
    for k, v in state.items():
        assert tuple(v.shape) == golden['state_shapes'][k], k
        # same default initialisation (same RNG consumption order) as the reference modules
        s, a = golden['state_checksums'][k]
        assert abs(float(v.double().sum()) - s) <= 1e-9 * max(1.0, a), k


def test_product_path_has_no_cpu_fallback():
    from megreader_amd.backbones import crnn_backbone
    from megreader_amd.nn import functional as F
    with pytest.raises(NotImplementedError):
        crnn_backbone()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError):
        F.ctc_loss_logits(torch.zeros(4, 1, 5), torch.zeros(1, 2, dtype=torch.int64), None, torch.tensor([1]))


def test_product_code_never_imports_oracle():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "megreader_amd")
    for dirpath, _, files in os.walk(root):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                with open(os.path.join(dirpath, fn)) as f:
                    src = f.read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(dirpath, fn)


def test_decode_persist_host_queries_without_a_gpu():
    """Host-only entry points of the persistent decode kernels (include/megreader_hip.h): workspace sizes follow the group layout of
    csrc/decode_persist.hip (groups of 4 rows up to 32 samples, of 8 beyond; + the XCC-id exchange + 256 status bytes), and without
    a device (or with too few CUs) `mr_decode_persist_ok` says no, so the decoder keeps its per-step launches."""
    lib = _lib.load()
    w4, w8, w32, w33 = (lib.mr_decode_persist_ws_bytes(n) for n in (4, 8, 32, 33))
    group4 = w4 - 4096 - 256
    assert group4 > 0 and w8 == 2 * group4 + 4096 + 256 and w32 == 8 * group4 + 4096 + 256
    assert (w33 - 4096 - 256) % 5 == 0 and (w33 - 4096 - 256) // 5 > group4          # 5 groups of 8 rows
    b4 = lib.mr_decode_persist_bwd_ws_bytes(4)
    assert lib.mr_decode_persist_bwd_ws_bytes(32) == 8 * (b4 - 4096 - 256) + 4096 + 256
    assert lib.mr_decode_persist_bwd_ws_bytes(33) == 0                                # the backward kernel stops at 32 samples
    if not torch.cuda.is_available():
        assert lib.mr_decode_persist_ok(_lib.dtype_code(torch.bfloat16), 16, 64, 512, 552) == 0
        assert lib.mr_decode_persist_bwd_ok(_lib.dtype_code(torch.bfloat16), 16, 64, 512, 552) == 0


def test_persistent_workspace_sizes_are_pinned():
    """The workspace of the persistent kernels is [granule slots][XCC-id exchange][256 status bytes] (csrc/persist_xch.h); callers
    size their buffers by these three queries and find the status block at the end, so the values are part of the ABI.  The
    literals were read from a build of the commit BEFORE the layout moved into one helper, not from the code under test."""
    lib = _lib.load()
    lstm = {1: 393600, 4: 393600, 5: 393600, 16: 393600, 17: 786944, 32: 786944, 33: 1180288, 64: 1573632, 250: 6293760,
            256: 6293760}
    fwd = {1: 174336, 4: 174336, 5: 344320, 16: 684288, 17: 854272, 32: 1364224, 33: 1704192, 64: 2724096}
    bwd = {1: 2265344, 4: 2265344, 5: 4526336, 16: 9048320, 17: 11309312, 32: 18092288, 33: 0, 64: 0}   # 0 above 32 rows
    for n, want in lstm.items():
        assert lib.mr_lstm_ws_bytes(1, 33, n, 256) == want, n
        assert lib.mr_lstm_ws_bytes(1, 2, n, 256) == want, n            # the size does not depend on T
        assert lib.mr_lstm_ws_bytes(0, 33, n, 256) == 0, n              # f32: one launch per step, no workspace
    for n, want in fwd.items():
        assert lib.mr_decode_persist_ws_bytes(n) == want, n
    for n, want in bwd.items():
        assert lib.mr_decode_persist_bwd_ws_bytes(n) == want, n
