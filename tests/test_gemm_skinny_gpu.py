"""gemm_nt_skinny_kernel (csrc/gemm_skinny.hip), the M <= 32 kernel behind every decode-step GEMM of the attention decoder, called
directly through mr_gemm_nt on EXACT operands, in the style of tests/test_nt_epilogue_gpu.py: A in [-3, 3], B in [-2, 2], bias a
multiple of 0.25, K <= 2048, so every partial sum is exact in f32 whatever the order (|A B^T| <= 6 * 2048 < 2^24) and the stored
value must EQUAL round_to_dtype(relu(A B^T + bias)) computed in float64.  Rows: one MFMA row tile, both, a ragged second one;
columns: a full 16-column group, whole vectors, element-wise stores under an odd leading dimension, many workgroups; K: a single
partial chunk (three of the four waves idle), a last chunk that is not full, the 8-deep instantiation.  C has pad columns and
spare rows filled with a sentinel that must survive, and the tile kernels (gemm_skinny = 0) must give the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd import _lib  # noqa: E402
from megreader_amd._lib import call, dtype_code, ptr  # noqa: E402

DEV = "cuda"
SENTINEL = 2048.0     # exact in bf16; compared only where nothing may be written

MS = (1, 15, 16, 17, 32)
N_KINDS = {"n16": (16, 24), "n40": (40, 48), "n38_ld43": (38, 43), "n2048": (2048, 2056)}      # N, ldc
KS = {torch.bfloat16: (8, 32, 72, 512, 1536, 2048), torch.float32: (4, 16, 40, 512)}
# skinny_depth 0 / 4 / 8, and the tile kernels as a fourth "depth"
VARIANTS = (dict(skinny_depth=0), dict(skinny_depth=4), dict(skinny_depth=8), dict(gemm_skinny=0))


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _quarters(shape, g):
    return torch.randint(-32, 33, shape, generator=g).float() * 0.25     # multiples of 0.25 in [-8, 8]


def _launch(dtype, A, lda, B, ldb, C, ldc, bias, relu, M, N, K, tuning):
    old = _lib.set_tuning(**tuning)
    try:
        call("mr_gemm_nt", dtype_code(dtype), ptr(A), lda, ptr(B), ldb, ptr(C), ldc, ptr(bias), relu, M, N, K)
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning(**old)


def _check(C, ref, M, N, what):
    bad = C[:M, :N] != ref
    assert not bool(bad.any()), (what, int(bad.sum()), "first (m, n)", bad.nonzero()[:4].tolist())
    assert bool((C[:M, N:] == SENTINEL).all()), (what, "pad columns written")
    assert bool((C[M:] == SENTINEL).all()), (what, "rows past M written")


def _reference(prod, bias, relu, dtype):
    ref = prod if bias is None else prod + bias.double()
    if relu:
        ref = torch.relu(ref)
    return ref.float().to(dtype)          # exact in f32, then the one rounding of the store


@pytest.mark.parametrize("nkind", list(N_KINDS))
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_skinny_gemm_is_exact(dtype, M, nkind):
    N, ldc = N_KINDS[nkind]
    g = torch.Generator().manual_seed(1000 * M + N)
    bias_buf = _quarters((N + 1,), g).to(DEV)            # bias_buf[1:] starts one float past a 16-byte boundary
    assert bias_buf.data_ptr() % 16 == 0
    for K in KS[dtype]:
        A = _ints((M, K), -3, 3, g).to(DEV, dtype)
        B = _ints((N, K), -2, 2, g).to(DEV, dtype)
        prod = A.double() @ B.double().t()
        for bias in (None, bias_buf[:N], bias_buf[1:]):
            for relu in (0, 1):
                ref = _reference(prod, bias, relu, dtype)
                outs = []
                for tuning in VARIANTS:
                    C = torch.full((M + 3, ldc), SENTINEL, device=DEV, dtype=dtype)
                    _launch(dtype, A, K, B, K, C, ldc, bias, relu, M, N, K, tuning)
                    _check(C, ref, M, N, (M, nkind, K, "bias %s" % ("none" if bias is None else bias.data_ptr() % 16), relu, tuning))
                    outs.append(C)
                for C in outs[1:]:
                    assert torch.equal(C, outs[0])       # pad columns and spare rows included: the same bits


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_skinny_gemm_with_padded_operand_rows(dtype):
    """lda and ldb above K: A and B are column slices of wider matrices whose other columns hold a value that would leave the
    integer range of the result."""
    M, (N, ldc), K = 17, N_KINDS["n40"], (72 if dtype == torch.bfloat16 else 40)
    vec = 8 if dtype == torch.bfloat16 else 4
    g = torch.Generator().manual_seed(K)
    lda, ldb = K + vec, K + 2 * vec
    Aw = torch.full((M, lda), 1000.0, device=DEV, dtype=dtype)
    Bw = torch.full((N, ldb), 1000.0, device=DEV, dtype=dtype)
    Aw[:, :K] = _ints((M, K), -3, 3, g).to(DEV, dtype)
    Bw[:, :K] = _ints((N, K), -2, 2, g).to(DEV, dtype)
    bias = _quarters((N,), g).to(DEV)
    ref = _reference(Aw[:, :K].double() @ Bw[:, :K].double().t(), bias, 1, dtype)
    for tuning in VARIANTS:
        C = torch.full((M + 3, ldc), SENTINEL, device=DEV, dtype=dtype)
        _launch(dtype, Aw, lda, Bw, ldb, C, ldc, bias, 1, M, N, K, tuning)
        _check(C, ref, M, N, ("padded rows", lda, ldb, tuning))
