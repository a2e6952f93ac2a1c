"""Where the parameter gradients of every weight-carrying autograd node go (megreader_amd/nn/functional.py, assets/ops/dcn).

One table over: both compute dtypes x gradient sinks on / off (FusedSGD lr = 0) x deferred weight-gradient launches on / off
(F._TnDefer.enabled) x which parameters require a gradient --
    "wb"  weight(s) and bias(es);
    "w"   the weight only: bias=None where the node takes that, else (batch_norm, bilstm: the biases are positional tensors)
          the biases frozen;
    "b"   the bias(es) only, the weight(s) frozen.
Each case holds the input and parameter gradients to the float64 reference with the bars the node already has in
tests/test_kernels_gpu.py (tests/test_dcn_gpu.py for the deformable convolution), and pins the sink protocol: gradients with
sinks == gradients without (f32), .grad stays the optimizer's view, the ready hooks fire once per backward for exactly the
parameters whose gradient went through a sink, a second backward doubles the gradient, nothing is left recorded.
"""
import math

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd._lib import load  # noqa: E402
from megreader_amd.assets.ops.dcn import modulated_deform_conv  # noqa: E402
from megreader_amd.nn import functional as F  # noqa: E402
from megreader_amd.optim import FusedSGD  # noqa: E402
from oracle.dcn import modulated_deform_conv2d  # noqa: E402
from test_conv_pool_gpu import CASES as POOL_CASES  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
LSTM_NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w_ih_r", "w_hh_r", "b_ih_r", "b_hh_r")


@pytest.fixture(autouse=True)
def _reset_dtype():
    yield
    mr.set_compute_dtype(torch.bfloat16)


def _tol(dtype, k=1):     # tests/test_kernels_gpu.py
    return (2e-5 * math.sqrt(k) + 1e-6) if dtype == torch.float32 else (1.6e-2)


def _rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _bars(dtype, f32, bf16_input, bf16_param):
    return (f32, f32) if dtype == torch.float32 else (bf16_input, bf16_param)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _round_ste(z, dtype):
    """z rounded to the compute dtype, gradient passed straight through (the nodes store their activation in that dtype and
    pick the pooling arg-max on the stored values)."""
    return z + (z.detach().to(dtype).double() - z.detach())


class Spec(object):
    """One node at one shape.  inputs: [(cpu tensor, wants a gradient)]; params: {name: cpu f32 tensor}, biases = names that
    start with "b"; ref(inputs64, params64) / hip(inputs on the device, params on the device): the output; a bias that the case
    leaves out arrives as None in both.  bars: (input gradients, parameter gradients) relative to the largest element.
    sunk(name, trainable names) -> does this parameter's gradient go through its sink when it has one."""

    def __init__(self, inputs, params, gy, ref, hip, bars, sunk, optional_bias=True, f32_weights=False):
        self.inputs, self.params, self.gy, self.ref, self.hip, self.bars, self.sunk = inputs, params, gy, ref, hip, bars, sunk
        self.optional_bias = optional_bias
        self.f32_weights = f32_weights       # the kernels read the weights as f32 (BatchNorm's gamma), not as a compute-dtype image


def _independent(name, trainable):
    return True


def _all_or_nothing(count):
    return lambda name, trainable: len(trainable) == count


def conv_spec(dtype, K, R, stride, pad):
    g = torch.Generator().manual_seed(16 * 7 + K + R)
    N, C, H, W = 2, 16, 5, 7
    x = _cl(torch.randn(N, C, H, W, generator=g).to(dtype))
    w = _cl(torch.randn(K, C, R, R, generator=g) * 0.1)       # physical KRSC, the layout nn.Conv2d keeps (sinks need it)
    b = torch.randn(K, generator=g)
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    gy = torch.randn(N, K, Ho, Wo, generator=g).to(dtype)
    tol = _tol(dtype, C * R * R)
    return Spec([(x, True)], {"w": w, "b": b}, gy,
                lambda i, p: TF.conv2d(i[0], p["w"], p["b"], stride, pad),
                lambda i, p: F.conv2d(i[0], p["w"], p["b"], (stride, stride), (pad, pad)),
                _bars(dtype, tol, tol, 2e-2), _independent)


def linear_spec(dtype, O):
    g = torch.Generator().manual_seed(3 + O)
    T, N, K = 5, 7, 64
    x = torch.randn(T, N, K, generator=g).to(dtype)
    w = torch.randn(O, K, generator=g) / 8
    b = torch.randn(O, generator=g)
    gy = torch.randn(T, N, O, generator=g).to(dtype)
    tol = _tol(dtype, K)
    return Spec([(x, True)], {"w": w, "b": b}, gy, lambda i, p: TF.linear(i[0], p["w"], p["b"]),
                lambda i, p: F.linear(i[0], p["w"], p["b"]), _bars(dtype, tol, tol, 2e-2), _independent)


def _dyadic(g, lo, hi, shape, scale=1.0):
    # exact in every precision: no near-tie of a ReLU / pooling arg-max flips between the f64 reference and the kernels
    return torch.randint(lo, hi + 1, shape, generator=g).float() * scale


def stem_spec(dtype, C):
    g = torch.Generator().manual_seed(200 + C)
    N, H, W = 2, 32, 16
    x = _dyadic(g, -3, 3, (N, C, H, W))
    w = _dyadic(g, -4, 4, (64, C, 3, 3), 0.125)
    b = _dyadic(g, -8, 8, (64,), 0.125)
    gy = _dyadic(g, -4, 4, (N, 64, H // 2, W // 2))
    return Spec([(x, False)], {"w": w, "b": b}, gy,
                lambda i, p: TF.max_pool2d(_round_ste(torch.relu(TF.conv2d(i[0], p["w"], p["b"], 1, 1)), dtype), 2, 2),
                lambda i, p: F.stem_conv_relu_pool(i[0], p["w"], p["b"]),
                _bars(dtype, 1e-4, 2e-2, 2e-2), _independent)


def _pool_geometry():
    """The smallest geometry of tests/test_conv_pool_gpu.py::CASES that takes the fused launch (None: none does, e.g. in f32)."""
    for name, N, Cin, H, W, Cout, pk, ps, pp in sorted(POOL_CASES, key=lambda c: c[1] * c[2] * c[3] * c[4] * c[5]):
        x = torch.empty((N, Cin, H, W), dtype=torch.bfloat16, device=DEV)
        w = torch.empty((Cout, Cin, 3, 3), device=DEV)
        if F.conv_relu_pool_eligible(x, w, (1, 1), (1, 1), (1, 1), pk, ps, pp):
            return N, Cin, H, W, Cout, pk, ps, pp
    return None


def conv_relu_pool_spec(dtype):
    geom = _pool_geometry()
    if geom is None:
        pytest.skip("no geometry of test_conv_pool_gpu.CASES takes the fused conv + ReLU + max-pool launch in %s" % dtype)
    N, Cin, H, W, Cout, pk, ps, pp = geom
    g = torch.Generator().manual_seed(N + Cin + W)
    x = _cl(_dyadic(g, -3, 3, (N, Cin, H, W)).to(dtype))
    w = _cl(_dyadic(g, -4, 4, (Cout, Cin, 3, 3), 1.0 / 64))
    b = _dyadic(g, -8, 8, (Cout,), 0.125)
    PH, PW = (H + 2 * pp[0] - pk[0]) // ps[0] + 1, (W + 2 * pp[1] - pk[1]) // ps[1] + 1
    gy = _dyadic(g, -4, 4, (N, Cout, PH, PW)).to(dtype)
    return Spec([(x, True)], {"w": w, "b": b}, gy,
                lambda i, p: TF.max_pool2d(_round_ste(torch.relu(TF.conv2d(i[0], p["w"], p["b"], 1, 1)), dtype), pk, ps, pp),
                lambda i, p: F.conv_relu_pool(i[0], p["w"], p["b"], (1, 1), pk, ps, pp),
                _bars(dtype, 1e-4, 2e-2, 2e-2), _independent)


def batch_norm_spec(dtype):
    g = torch.Generator().manual_seed(5)
    N, C, H, W = 2, 16, 5, 7
    x = _cl((torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(dtype))
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    gy = torch.randn(N, C, H, W, generator=g).to(dtype)

    def hip(i, p):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        return F.batch_norm(i[0], p["w"], p["b"], rm, rv, True, 0.1, 1e-5)
    return Spec([(x, True)], {"w": gamma, "b": beta}, gy,
                lambda i, p: TF.batch_norm(i[0], None, None, p["w"], p["b"], True, 0.1, 1e-5), hip,
                _bars(dtype, 1e-4, 2e-2, 1e-2), _all_or_nothing(2), optional_bias=False, f32_weights=True)


def bilstm_spec(dtype, T, N, I, H):
    torch.manual_seed(17)
    ref = torch.nn.LSTM(I, H, bidirectional=True)
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
             "bias_ih_l0_reverse", "bias_hh_l0_reverse")
    params = {k: getattr(ref, n).detach().clone() for k, n in zip(LSTM_NAMES, names)}
    x = torch.randn(T, N, I).to(dtype)
    gy = torch.randn(T, N, 2 * H).to(dtype)

    def run_ref(i, p):
        return torch.func.functional_call(ref.double(), {n: p[k] for k, n in zip(LSTM_NAMES, names)}, (i[0],))[0]
    bar = 2e-4 if dtype == torch.float32 else 4e-2
    return Spec([(x, True)], params, gy, run_ref, lambda i, p: F.bilstm(i[0], *[p[k] for k in LSTM_NAMES]),
                (bar, bar), _all_or_nothing(8), optional_bias=False)


def dcn_spec(dtype):
    N, C, Co, H, W, stride, pad, dil, oscale = 3, 8, 8, 5, 6, 1, 1, 1, 4.0      # the smallest of tests/test_dcn_gpu.py::CASES
    g = torch.Generator().manual_seed(C + H)
    x = _cl(torch.randn(N, C, H, W, generator=g).to(dtype))
    off = torch.randn(N, 18, H, W, generator=g) * oscale
    off = torch.floor(off) + 0.25 + 0.5 * torch.rand(off.shape, generator=g)    # away from the kinks of the bilinear kernel
    msk = torch.rand(N, 9, H, W, generator=g)
    w = _cl(torch.randn(Co, C, 3, 3, generator=g) * 0.2)
    b = torch.randn(Co, generator=g)
    gy = torch.randn(N, Co, H, W, generator=g).to(dtype)
    return Spec([(x, True), (off, True), (msk, True)], {"w": w, "b": b}, gy,
                lambda i, p: modulated_deform_conv2d(i[0], i[1], i[2], p["w"], p["b"], stride, pad, dil),
                lambda i, p: modulated_deform_conv(i[0], i[1], i[2], p["w"], p["b"], stride, pad, dil, 1, 1),
                _bars(dtype, 1e-4, 3e-2, 3e-2), _independent)


NODES = {
    "conv3x3_k16": lambda dt: conv_spec(dt, 16, 3, 1, 1),
    "conv3x3_k27": lambda dt: conv_spec(dt, 27, 3, 1, 1),        # output padded to 32 (bf16) / 28 (f32) channels
    "conv1x1_s2": lambda dt: conv_spec(dt, 16, 1, 2, 0),
    "linear_o38": lambda dt: linear_spec(dt, 38),                # logits in a 40-column buffer
    "linear_o40": lambda dt: linear_spec(dt, 40),
    "stem_c1": lambda dt: stem_spec(dt, 1),
    "stem_c3": lambda dt: stem_spec(dt, 3),
    "conv_relu_pool": conv_relu_pool_spec,
    "batch_norm": batch_norm_spec,
    "bilstm_t5": lambda dt: bilstm_spec(dt, 5, 3, 64, 32),
    "bilstm_t1": lambda dt: bilstm_spec(dt, 1, 3, 64, 32),       # never defers
    "dcn": dcn_spec,
}

_SPECS, _REFS = {}, {}


def _spec(node, dtype):
    key = (node, dtype)
    if key not in _SPECS:
        _SPECS[key] = NODES[node](dtype)
    return _SPECS[key]


def _is_bias(name):
    return name.startswith("b")


def _reference(node, dtype, spec, with_bias):
    """float64 gradients on the operands the kernels see (inputs and weights rounded to the compute dtype, biases f32); computed
    once per (node, dtype, with / without bias) and shared by every case."""
    key = (node, dtype, with_bias)
    if key not in _REFS:
        ins = [t.double().requires_grad_(need) for t, need in spec.inputs]
        ps = {k: (None if (_is_bias(k) and not with_bias) else
                  (v.double() if (_is_bias(k) or spec.f32_weights) else v.to(dtype).double()).requires_grad_(True)) for k, v in spec.params.items()}
        spec.ref(ins, ps).backward(spec.gy.double())
        _REFS[key] = ([t.grad for t in ins], {k: (None if v is None else v.grad) for k, v in ps.items()})
    return _REFS[key]


def _run_hip(spec, dtype, sinks, which, passes):
    """`passes` forward + backward runs of the node; (input gradients of the last pass, parameter gradients, ready-hook counts,
    parameters on the device)."""
    with_bias = not (which == "w" and spec.optional_bias)
    params = {}
    for k, v in spec.params.items():
        if _is_bias(k) and not with_bias:
            params[k] = None
            continue
        params[k] = v.to(DEV).requires_grad_(which == "wb" or (which == "b") == _is_bias(k))
    trainable = [k for k, p in params.items() if p is not None and p.requires_grad]
    if sinks:
        opt = FusedSGD([params[k] for k in trainable], lr=0.0)
        opt.zero_grad()
    counts = {k: 0 for k in trainable}
    for k in trainable:
        def hook(p, k=k):
            counts[k] += 1
        if not hasattr(params[k], "_mr_grad_ready_hooks"):
            params[k]._mr_grad_ready_hooks = []
        params[k]._mr_grad_ready_hooks.append(hook)
    for _ in range(passes):
        ins = [t.to(DEV).requires_grad_(need) for t, need in spec.inputs]
        y = spec.hip(ins, params)
        gy = spec.gy.to(DEV).to(dtype)
        y.backward(_cl(gy) if (gy.dim() == 4 and gy.shape[1] % 8 == 0) else gy)
        assert load().mr_tn_pending() == 0          # no recorded weight-gradient problem survives backward()
    torch.cuda.synchronize()
    return [t.grad for t in ins], {k: params[k].grad for k in trainable}, counts, params


@pytest.mark.parametrize("which", ["wb", "w", "b"])
@pytest.mark.parametrize("defer", [True, False], ids=["defer", "nodefer"])
@pytest.mark.parametrize("sinks", [False, True], ids=["autograd", "sinks"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("node", list(NODES))
def test_parameter_gradient_paths(node, dtype, sinks, defer, which):
    mr.set_compute_dtype(dtype)
    spec = _spec(node, dtype)
    with_bias = not (which == "w" and spec.optional_bias)
    ref_in, ref_p = _reference(node, dtype, spec, with_bias)
    old = F._TnDefer.enabled
    F._TnDefer.enabled = defer
    try:
        gin, gp, counts, params = _run_hip(spec, dtype, sinks, which, 1)
        _, gp2, counts2, _ = _run_hip(spec, dtype, sinks, which, 2)
        plain = _run_hip(spec, dtype, False, which, 1)[1] if (sinks and dtype == torch.float32) else None
    finally:
        F._TnDefer.enabled = old
    in_bar, p_bar = spec.bars
    errs = {}
    for i, (g, r) in enumerate(zip(gin, ref_in)):
        if r is not None:
            errs["input%d" % i] = (_rel_err(g, r), in_bar)
    assert gp, "no trainable parameter"
    for k, g in gp.items():
        assert g is not None, k
        errs[k] = (_rel_err(g, ref_p[k]), p_bar)
    print("%s %s sinks=%d defer=%d %s: %s" % (node, str(dtype).split(".")[-1], sinks, defer, which,
                                             ", ".join("%s %.2e" % (k, e) for k, (e, _) in errs.items())))
    for k, (e, bar) in errs.items():
        assert e < bar, (k, e, bar)
    for k, g in gp.items():
        # accumulate semantics: a second backward into the same gradient doubles it (f32 sums either way: round-off of their order)
        scale = 2.0 * float(g.abs().max())
        assert float((gp2[k] - 2.0 * g).abs().max()) <= 2e-5 * scale + 1e-7, k
        sunk = sinks and spec.sunk(k, list(gp))
        assert counts[k] == (1 if sunk else 0) and counts2[k] == (2 if sunk else 0), (k, counts, counts2)
        if sinks:
            assert g.data_ptr() == params[k]._mr_grad_sink.data_ptr(), k      # still the optimizer's view
        if plain is not None:       # the rule of tests/test_crnn_gpu.py::test_gradient_sinks_match_autograd_accumulation
            assert float((plain[k] - g).abs().max()) <= 2e-5 * float(plain[k].abs().max()) + 1e-7, k
