"""The CTC heads with a 5 360-class charset (the size of the reference's ChineseCharset) against their oracles: CRNN
(crnn_backbone + CRNNDecoder; N = 4, 32x64 images, T = 17) in fp32 -- loss, log-probabilities, every parameter gradient against
the float64 oracle (tests/_parity.py), state_dict layout, eval output -- and in bf16 with FusedAdam; CTCDecoder for one
training step.  The charset is built from a code-point range: no dictionary file is needed."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd import _lib  # noqa: E402
from megreader_amd.backbones import crnn_backbone  # noqa: E402
from megreader_amd.charsets import Charset  # noqa: E402
from megreader_amd.decoders import CRNNDecoder, CTCDecoder  # noqa: E402
from megreader_amd.optim import FusedAdam  # noqa: E402
from oracle.crnn import CRNNOracle, synthetic_batch  # noqa: E402
from oracle.ctc_decoder import CTCDecoderOracle  # noqa: E402

from _parity import f64_grads, grad_report  # noqa: E402

DEV = "cuda"
CLASSES = 5360


def wide_charset():
    cs = Charset([chr(0x4E00 + i) for i in range(CLASSES - 2)])
    assert len(cs) == CLASSES
    return cs


class BasicModel(torch.nn.Module):
    """reference structure/model.py:16-24: decoder(backbone(data), *args, **kwargs)."""

    def __init__(self):
        super().__init__()
        self.backbone = crnn_backbone()
        self.decoder = CRNNDecoder(charset=wide_charset(), in_channels=512, inner_channels=256)

    def forward(self, data, *args, **kwargs):
        return self.decoder(self.backbone(data), *args, **kwargs)


@pytest.fixture(autouse=True)
def _reset_dtype():
    yield
    mr.set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope="module")
def case():
    """oracle weights, batch and the oracle's own f32 / f64 passes, computed once on the CPU"""
    assert _lib.load().mr_ctc_wide(CLASSES, 32) == 1
    torch.manual_seed(7)
    ora = CRNNOracle(num_classes=CLASSES).train()
    state0 = copy.deepcopy(ora.state_dict())
    batch = synthetic_batch(4, 32, 64, seed=3, num_classes=CLASSES)
    lengths = batch['length'].long()

    def forward(model, dtype):
        loss, _ = model(batch['image'].to(dtype), targets=batch['label'], lengths=lengths, train=True)
        return loss.mean()

    grads64 = f64_grads(ora, forward)
    ora.zero_grad()
    loss, logp = ora(batch['image'], targets=batch['label'], lengths=lengths, train=True)
    loss.mean().backward()
    grads32 = {k: p.grad.detach().clone() for k, p in ora.named_parameters()}
    state1 = copy.deepcopy(ora.state_dict())          # BatchNorm statistics moved by the one training forward
    ora.eval()
    with torch.no_grad():
        ev = ora(batch['image'], train=False)
    return dict(state0=state0, state1=state1, batch=batch, loss=float(loss.detach()), logp=logp.detach(), grads32=grads32,
                grads64=grads64, eval=ev)


def _to_dev(batch):
    return batch['image'].to(DEV), batch['label'].to(DEV), batch['length'].to(DEV).long()


def test_state_dict_layout_matches_the_oracle(case):
    model = BasicModel()
    sd = model.state_dict()
    assert list(sd.keys()) == list(case["state0"].keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(case["state0"][k].shape), k
    assert tuple(sd["decoder.rnn.1.embedding.weight"].shape) == (CLASSES, 512)
    model.load_state_dict(case["state0"], strict=True)


def test_fp32_training_and_eval_parity(case):
    mr.set_compute_dtype(torch.float32)
    model = BasicModel()
    model.load_state_dict(case["state0"])
    model.to(DEV).train()
    img, lab, ln = _to_dev(case["batch"])
    loss, pred = model(img, targets=lab, lengths=ln, train=True)
    assert loss.dtype == torch.float64 and pred.dtype == torch.float64 and tuple(pred.shape) == (17, 4, CLASSES)
    lerr = abs(float(loss) - case["loss"])
    perr = float((pred.cpu() - case["logp"]).abs().max())
    print("CRNN fp32, %d classes: loss %.6f |d| %.2e, log-prob max|d| %.2e" % (CLASSES, float(loss), lerr, perr))
    assert lerr < 1e-4
    assert perr < 1e-4
    loss.mean().backward()
    grad_report(list(model.named_parameters()), case["grads32"], case["grads64"], "CRNN fp32 %d classes" % CLASSES)
    model.eval()
    with torch.no_grad():
        ev = model(img, train=False)
    assert tuple(ev.shape) == tuple(case["eval"].shape) == (4, CLASSES, 1, 17)
    # (no decode comparison at random initialisation: the class probabilities are ~1.9e-4, arg-max margins carry no information)
    eerr = float((ev.cpu().double().log() - case["eval"].double().log()).abs().max())
    print("CRNN fp32, %d classes: eval max |log p - log p_oracle| %.2e" % (CLASSES, eerr))
    assert eerr < 1e-4


def test_bf16_fused_adam_steps(case):
    """three FusedAdam steps in bf16: finite losses; the first step's drift against the oracle within the bars of
    tests/test_crnn_gpu.py::test_bf16_training_close_to_oracle (loss 0.1, gradient norms 25 %)"""
    mr.set_compute_dtype(torch.bfloat16)
    model = BasicModel()
    model.load_state_dict(case["state0"])
    model.to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    img, lab, ln = _to_dev(case["batch"])
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss, _ = model(img, targets=lab, lengths=ln, train=True)
        loss.mean().backward()
        if step == 0:
            torch.cuda.synchronize()
            for k, p in model.named_parameters():
                norm = float(case["grads32"][k].double().norm())
                if norm < 1e-5:
                    continue  # conv bias feeding a BatchNorm: mathematically zero gradient, only round-off
                rel = abs(float(p.grad.double().norm()) - norm) / norm
                assert rel < 0.25, (k, rel, norm)
        opt.step()
        losses.append(float(loss))
    print("CRNN bf16, %d classes: losses %s (oracle first step %.6f)" % (CLASSES, losses, case["loss"]))
    assert all(l == l and abs(l) < 1e4 for l in losses), losses
    assert abs(losses[0] - case["loss"]) < 0.1


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def test_ctc_decoder_one_training_step():
    """decoders.CTCDecoder with 5 360 classes: the bars of tests/test_ctc_decoder_gpu.py::test_fp32_parity_vs_oracle"""
    mr.set_compute_dtype(torch.float32)
    n, cin, inner, h, w = 6, 64, 64, 16, 64
    torch.manual_seed(11)
    ora = CTCDecoderOracle(cin, num_classes=CLASSES, inner_channels=inner).train()
    g = torch.Generator().manual_seed(4)
    feat = torch.randn(n, cin, h, w, generator=g)
    lengths = torch.randint(2, 9, (n,), generator=g)
    labels = torch.zeros((n, 32), dtype=torch.long)
    for i in range(n):
        labels[i, :lengths[i]] = torch.randint(1, CLASSES, (int(lengths[i]),), generator=g)
    labels[0, 0], labels[1, 0] = CLASSES - 1, 2
    model = CTCDecoder(in_channels=cin, charset=wide_charset(), inner_channels=inner)
    model.load_state_dict(ora.state_dict(), strict=True)
    model.to(DEV).train()
    ora64 = copy.deepcopy(ora).double()
    x64 = feat.double().requires_grad_(True)
    l64, _ = ora64(x64, targets=labels, lengths=lengths, train=True)
    l64.backward()
    xo = feat.clone().requires_grad_(True)
    lo, po = ora(xo, targets=labels, lengths=lengths, train=True)
    lo.backward()
    xd = feat.to(DEV).requires_grad_(True)
    loss, pred = model(xd, targets=labels.to(DEV), lengths=lengths.to(DEV), train=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and pred.shape == po.shape and pred.dtype == torch.float32
    assert abs(float(loss) - float(lo)) < 1e-4 * max(1.0, abs(float(lo)))
    assert float((pred.cpu() - po).abs().max()) < 1e-4
    loss.backward()
    g64 = dict(ora64.named_parameters())
    g32 = dict(ora.named_parameters())
    worst = 0.0
    for k, p in model.named_parameters():
        scale = float(g64[k].grad.abs().max())
        if scale < 1e-9:      # conv biases in front of a BatchNorm: zero gradient
            continue
        e_hip, e_cpu = _rel(p.grad, g64[k].grad), _rel(g32[k].grad, g64[k].grad)
        worst = max(worst, e_hip)
        assert e_hip < max(4 * e_cpu, 1e-3), (k, e_hip, e_cpu)
    assert _rel(xd.grad, x64.grad) < max(4 * _rel(xo.grad, x64.grad), 1e-3)
    print("CTCDecoder fp32, %d classes: loss |d| %.2e, log-prob max|d| %.2e, worst gradient error vs f64 %.2e" %
          (CLASSES, abs(float(loss) - float(lo)), float((pred.cpu() - po).abs().max()), worst))
