"""csrc/db_loss.hip (L1BalanceCELoss in seven launches forward, one backward) against the float64 reference of
tests/_db_loss_ref.py in every branch of its radix selection: k = 0, k = every negative, fewer positive-valued losses than k,
a threshold decided inside one 12-bit or one 24-bit bin, the BCE clamps, a non-integer ratio, mask values that truncate to 0,
an upstream gradient other than 1, grid-striding kernels and a partial workgroup.  tests/test_db_loss_ref_cpu.py shows that the
inputs reach those branches and that an off-by-one selection would move bce by 20x the tolerance used here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd.decoders import L1BalanceCELoss  # noqa: E402
from megreader_amd.decoders import seg_detector_loss as sdl  # noqa: E402

from _db_loss_ref import LOSS_TOL, REGIMES, UPSTREAM, case_and_reference  # noqa: E402

DEV = "cuda"
GRAD_TOL = 1e-5      # the project's max-norm bound for float32 element-wise kernels


@pytest.fixture(autouse=True)
def _fused(monkeypatch):
    monkeypatch.setattr(sdl, "FUSED_DB_LOSS", True)


def _run(case):
    crit = L1BalanceCELoss(eps=case['eps'], l1_scale=case['l1_scale'], bce_scale=case['bce_scale'])
    crit.bce_loss.negative_ratio = case['negative_ratio']
    pred = {k: v.to(DEV).requires_grad_(True) for k, v in case['pred'].items()}
    batch = {k: v.to(DEV) for k, v in case['batch'].items()}
    assert sdl._fused_ok(pred, batch) and crit.dice_loss.eps == crit.bce_loss.eps      # the HIP path, not the restatement
    loss, metrics = crit(pred, batch)
    (loss * UPSTREAM).backward()
    vals = dict(loss=float(loss), bce=float(metrics['bce_loss']), l1=float(metrics['l1_loss']),
                dice=float(metrics['thresh_loss']))
    grads = {k: v.grad.detach().double().cpu() for k, v in pred.items()}
    return vals, grads, loss


def _rel(a, b, keep=None):
    d = (a - b).abs()
    if keep is not None:
        d, b = d[keep], b[keep]
    if d.numel() == 0:
        return 0.0
    return float(d.max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("name", REGIMES)
def test_fused_db_loss_vs_f64_reference(name):
    case, ref = case_and_reference(name)
    vals, grads, _ = _run(case)
    p, gt = case['pred']['binary'].double(), case['batch']['gt'].double()
    g_ref, g_got = ref['g_binary'], grads['binary']

    err = {k: abs(vals[k] - ref[k]) / max(1.0, abs(ref[k])) for k in ("loss", "bce", "l1", "dice")}
    e_th, e_tb = _rel(grads['thresh'], ref['g_thresh']), _rel(grads['thresh_binary'], ref['g_tbinary'])
    if name == "zero_losses":
        keep = ref['l'] > 0               # l = 0: dl/dp = 0 on both sides whatever the selection takes
    elif name == "adjacent_floats":
        keep = torch.zeros_like(ref['near'])
    else:
        keep = ~ref['near']
    e_b = _rel(g_got, g_ref, keep)
    s_ref = float(g_ref.abs().sum())
    e_sum = abs(float(g_got.sum()) - float(g_ref.sum())) / s_ref if s_ref > 0 else abs(float(g_got.sum()))
    print("%s: pc %d nc %d near %d | loss %.2e bce %.2e l1 %.2e dice %.2e (bound %.0e) | g_thresh %.2e g_tbinary %.2e "
          "g_binary %.2e (bound %.0e) | sum g_binary %.2e (bound 1e-04)"
          % (name, ref['pc'], ref['nc'], int(ref['near'].sum()), err['loss'], err['bce'], err['l1'], err['dice'], LOSS_TOL,
             e_th, e_tb, e_b, GRAD_TOL, e_sum))

    for k in err:
        assert err[k] < LOSS_TOL, (k, vals[k], ref[k])
    for k in grads:
        assert bool(torch.isfinite(grads[k]).all()), k
    assert e_th < GRAD_TOL and e_tb < GRAD_TOL
    if name in ("no_positives", "positives_all_masked"):
        assert vals['bce'] == 0.0 and not g_got.any()
    if name == "exact_l1_zero":
        assert not grads['thresh'][:, 0][case['l1_zero']].any()
    assert e_b < GRAD_TOL
    assert e_sum <= 1e-4
    if name == "clamped":
        # the two clamped groups carry (p - t) / 1e-12 and set the max norm alone: the rest once more on its own scale
        plain = keep & (p > 0) & (p < 1)
        e_plain = _rel(g_got, g_ref, plain)
        print("clamped: g_binary on the unclamped elements %.2e" % e_plain)
        assert e_plain < GRAD_TOL

    if name == "adjacent_floats":
        # Element-wise the selection weight is 1 above the kernel's threshold, one constant share on the elements equal to it and
        # 0 below.  The kernel's l is a function of (p, t) alone, so among the negatives every one of the 7 values of p carries
        # ONE weight; recover it from the gradient: g = UPSTREAM bce_scale inv dl (P + Q sel), P / Q = the element's number of
        # positive / negative entries in the broadcast.
        inv = 1.0 / (ref['pc'] + ref['nc'] + case['eps'])
        dl = (p - gt) / torch.clamp((1 - p) * p, min=1e-12)
        Q, P = ref['Q'], ref['P']
        has = Q > 0
        assert bool((gt[has] == 0).all())
        sel = (g_got / (UPSTREAM * case['bce_scale'] * inv * dl) - P) / Q
        weights = []
        for lv in case['levels']:
            s = sel[has & (p == float(lv))]
            assert s.numel() > 0 and float(s.max() - s.min()) < 1e-5, (float(lv), float(s.min()), float(s.max()))
            weights.append(float(s.mean()))
        print("adjacent_floats: selection weight per value of p:", ["%.6f" % w for w in weights])
        frac = [w for w in weights if 1e-5 < w < 1 - 1e-5]
        assert all(-1e-5 < w < 1 + 1e-5 for w in weights)
        assert not frac or max(frac) - min(frac) < 1e-5, frac                 # one share
        assert abs(float((sel * Q)[has].sum()) - ref['nc']) < 1e-4 * ref['nc']       # nc entries in all


def test_grid_stride_is_repeatable():
    """The reductions are atomics on doubles, whose order differs from run to run; the four float32 results are each rounded
    once from a double, so two calls are expected to agree to the bit."""
    case, ref = case_and_reference("grid_stride")
    outs = []
    for _ in range(2):
        pred = {k: v.to(DEV) for k, v in case['pred'].items()}
        b = {k: v.to(DEV) for k, v in case['batch'].items()}
        outs.append(sdl._DBLossFn.apply(pred['binary'], pred['thresh'], pred['thresh_binary'], b['gt'], b['mask'], b['thresh_map'],
                                        b['thresh_mask'], case['negative_ratio'], case['eps'], case['l1_scale'],
                                        case['bce_scale'])[0:4].clone())
    spread = (outs[0].double() - outs[1].double()).abs() / outs[0].double().abs().clamp(min=1.0)
    print("grid_stride: two calls differ by", spread.tolist())
    for o in outs:
        for i, k in enumerate(("loss", "bce", "l1", "dice")):
            assert abs(float(o[i]) - ref[k]) < LOSS_TOL * max(1.0, abs(ref[k])), (k, float(o[i]), ref[k])
    assert torch.equal(outs[0], outs[1])
