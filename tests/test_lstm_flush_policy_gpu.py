"""When the weight gradients of a BiLSTM layer are launched (nn/functional.py: BiLSTMFn.backward, nn/grads.py: _TnDefer).

Without a data-parallel wrapper nothing reads a weight gradient before the optimizer: the layer's four GEMMs and the Linear
behind it stay recorded when the node returns and run in the end-of-backward flush, grouped with everything else.  With a
wrapper listening to one of the layer's parameters (`_mr_grad_ready_hooks`) the node flushes itself, so that the gradients are
reported as they complete.  Either way every gradient meets the float64 bars tests/test_kernels_gpu.py sets for the BiLSTM
and Linear backward in bf16.  Shapes: the smallest the persistent recurrence kernels take (T = 3, N = 16, H = 256).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd.nn import grads as G  # noqa: E402

T, N, I, H, O = 3, 16, 64, 256, 38
LSTM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
              "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def _rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


_REFERENCE = {}


def _reference():
    """float64 torch LSTM + Linear on the bf16-rounded weights and inputs; computed once, never modified"""
    if not _REFERENCE:
        torch.manual_seed(23)
        lstm = torch.nn.LSTM(I, H, bidirectional=True).double()
        lin = torch.nn.Linear(2 * H, O).double()
        with torch.no_grad():
            for n_, p in list(lstm.named_parameters()) + [("weight", lin.weight)]:
                if n_.startswith("weight"):
                    p.copy_(p.float().bfloat16().double())
        x = torch.randn(T, N, I).bfloat16()
        gy = torch.randn(T, N, O).bfloat16()
        xr = x.double().requires_grad_(True)
        y = lin(lstm(xr)[0])
        y.backward(gy.double())
        _REFERENCE.update(lstm=lstm, lin=lin, x=x, gy=gy, dx=xr.grad)
    return _REFERENCE


def _model(dev):
    from megreader_amd.decoders.crnn import BidirectionalLSTM
    from megreader_amd.optim import FusedAdam
    ref = _reference()
    net = BidirectionalLSTM(I, H, O)
    with torch.no_grad():
        for n_ in LSTM_NAMES:
            getattr(net.rnn, n_).copy_(getattr(ref["lstm"], n_).float())
        net.embedding.weight.copy_(ref["lin"].weight.float())
        net.embedding.bias.copy_(ref["lin"].bias.float())
    net.to(dev).train()
    opt = FusedAdam(net.parameters(), lr=0.0)      # gradient sinks: the weight gradients may be recorded
    opt.zero_grad()
    return net, opt


def _check_grads(net, dx):
    ref = _reference()
    assert _rel_err(dx, ref["dx"]) < 4e-2
    for n_ in LSTM_NAMES:
        assert _rel_err(getattr(net.rnn, n_).grad, getattr(ref["lstm"], n_).grad) < 4e-2, n_
    assert _rel_err(net.embedding.weight.grad, ref["lin"].weight.grad) < 2e-2
    assert _rel_err(net.embedding.bias.grad, ref["lin"].bias.grad) < 2e-2


def _backward(net, dev, at_node_return):
    """forward + backward; at_node_return() runs when the BiLSTM node has handed back dx"""
    ref = _reference()
    xin = ref["x"].to(dev).requires_grad_(True)
    xin.register_hook(lambda g: at_node_return())
    y = net(xin)
    y.backward(ref["gy"].to(dev))
    torch.cuda.synchronize()
    return xin.grad


@pytest.fixture(autouse=True)
def _bf16():
    mr.set_compute_dtype(torch.bfloat16)
    yield
    G.discard_deferred_wgrads()
    mr.set_compute_dtype(torch.bfloat16)


def test_without_a_listener_the_layer_waits_for_the_end_of_backward():
    lib = _lib.load()
    net, _ = _model("cuda")
    seen = []
    dx = _backward(net, "cuda", lambda: seen.append((lib.mr_tn_pending(), lib.mr_tn_pending_of(0))))
    # W_ih x 2, W_hh x 2 and the Linear before them: recorded, not launched, when the node returned
    assert len(seen) == 1 and seen[0][0] == seen[0][1] >= 4
    assert lib.mr_tn_pending() == 0 and not G._TnDefer.keep and not G._TnDefer.notify
    _check_grads(net, dx)


@pytest.mark.parametrize("listen", ["weight_ih_l0", "bias_hh_l0_reverse", "all"])
def test_with_a_listener_the_layer_flushes_inside_its_node(listen):
    lib = _lib.load()
    net, _ = _model("cuda")
    fired, seen = [], []
    for n_ in LSTM_NAMES if listen == "all" else (listen,):
        p = getattr(net.rnn, n_)
        p._mr_grad_ready_hooks = [lambda q, n_=n_: fired.append(n_)]
    # when the node returns: nothing pending, nothing kept, every parameter of the flush reported, the hooks have fired
    dx = _backward(net, "cuda", lambda: seen.append((lib.mr_tn_pending(), len(G._TnDefer.keep), len(G._TnDefer.notify), list(fired))))
    want = list(LSTM_NAMES) if listen == "all" else [listen]
    assert len(seen) == 1 and seen[0][:3] == (0, 0, 0) and sorted(seen[0][3]) == sorted(want)
    assert sorted(fired) == sorted(want)             # ... and exactly once
    assert lib.mr_tn_pending() == 0
    _check_grads(net, dx)


def test_backward_from_a_thread_on_another_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    lib = _lib.load()
    with torch.cuda.device(1):
        net, _ = _model("cuda:1")
        ref = _reference()
        xin = ref["x"].to("cuda:1").requires_grad_(True)
        y = net(xin)
        gy = ref["gy"].to("cuda:1")
    assert torch.cuda.current_device() == 0
    y.backward(gy)                   # the end-of-backward flush runs here, on a thread whose current device is 0
    torch.cuda.synchronize(1)
    with torch.cuda.device(1):
        assert lib.mr_tn_pending() == 0
    _check_grads(net, xin.grad)
