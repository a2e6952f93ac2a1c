"""What can be settled without a GPU about the float64 reference of the DB loss and its inputs (tests/_db_loss_ref.py): every
builder reaches the branch of csrc/db_loss.hip it is named after, the selection threshold is isolated, a selection that is
off by one element or ignores the cross-sample broadcast would show, and the package's device-count restatement agrees."""
import pytest
import torch

from _db_loss_ref import LOSS_TOL, REGIMES, TIE_REGIMES, UPSTREAM, balanced_bce, case_and_reference


def _ulps_apart(lo, hi):
    a = torch.tensor([lo, hi], dtype=torch.float32).view(torch.int32)
    return int(a[1] - a[0])


def test_each_builder_reaches_its_regime():
    R = {n: case_and_reference(n) for n in REGIMES}
    for n, (c, r) in R.items():
        print("%-22s N*HW %6d pc %6d nc %6d negatives %7d near-threshold %d elements (%d entries)"
              % (n, c['pred']['binary'].numel(), r['pc'], r['nc'], r['n_neg'], int(r['near'].sum()), r['near_entries']))
    selecting = ("generic", "clamped", "one_top_bin", "adjacent_floats", "ratio_2_5", "half_mask", "three_samples",
                 "grid_stride", "tiny", "exact_l1_zero")
    for n in selecting:
        r = R[n][1]
        assert 0 < r['nc'] < r['n_neg'] and r['n_pos_valued'] >= r['nc'], n
    c, r = R['generic']
    assert c['pred']['binary'].shape == (2, 1, 20, 23) and (20 * 23) % 256 != 0
    assert not torch.equal(c['batch']['gt'][0], c['batch']['gt'][1])
    assert not torch.equal(c['batch']['mask'][0], c['batch']['mask'][1])
    c, r = R['no_positives']
    assert r['pc'] == 0 and r['nc'] == 0 and r['bce'] == 0.0 and not r['g_binary'].any()
    c, r = R['positives_all_masked']
    assert c['batch']['gt'].sum() > 0 and r['pc'] == 0 and r['nc'] == 0 and r['bce'] == 0.0 and not r['g_binary'].any()
    assert r['l1'] > 0 and r['g_thresh'].any() and r['n_neg'] > 0
    assert r['dice'] == 1.0 and not r['g_tbinary'].any()    # gt * mask = 0: no intersection, and none to gain
    c, r = R['all_negatives']
    assert r['nc'] == r['n_neg'] > 0 and r['n_pos_valued'] == r['n_neg']
    c, r = R['zero_losses']
    assert r['nc'] == r['n_neg'] and 0 < r['n_pos_valued'] < r['nc'] and r['v'] == 0.0
    p, gt = c['pred']['binary'], c['batch']['gt']
    assert int(((p == 0) & (gt == 0)).sum()) == int((gt == 0).sum()) // 2 and int(((p == 1) & (gt == 1)).sum()) == 12
    c, r = R['clamped']
    p, gt = c['pred']['binary'], c['batch']['gt']
    assert int(((p == 1) & (gt == 0)).sum()) == 20 and int(((p == 0) & (gt == 1)).sum()) == 20
    assert float(r['l'][(p == 1) & (gt == 0)].min()) == 100.0 and float(r['l'][(p == 0) & (gt == 1)].min()) == 100.0
    assert float(r['g_binary'].abs().max()) > 1e8              # (p - t) / 1e-12 reaches the gradient
    c, r = R['one_top_bin']
    assert 1.0 <= float(r['neg_values'].min()) and float(r['neg_values'].max()) < 1.125    # one 12-bit bin of the float
    c, r = R['adjacent_floats']
    assert _ulps_apart(float(r['neg_values'].min()), float(r['neg_values'].max())) <= 64    # one 24-bit bin or its neighbour
    assert torch.equal(torch.unique(c['pred']['binary']), c['levels'])
    for n in ('one_top_bin', 'adjacent_floats'):
        gt = R[n][0]['batch']['gt']
        assert int((gt[0] != gt[1]).sum()) == 24 and int(R[n][0]['flipped'].sum()) == 24
    c, r = R['ratio_2_5']
    assert c['negative_ratio'] == 2.5 and r['pc'] % 2 == 1 and r['nc'] == (5 * r['pc'] - 1) // 2
    c, r = R['half_mask']
    for k in ('mask', 'thresh_mask'):
        assert sorted(torch.unique(c['batch'][k]).tolist()) == [0.0, 0.5, 1.0], k
    full = dict(c['batch'], mask=(c['batch']['mask'] > 0).float())      # a kernel that did not truncate would count these
    assert int((full['gt'] * full['mask']).sum()) != int((c['batch']['gt'] * c['batch']['mask']).byte().sum())
    c, r = R['three_samples']
    assert c['pred']['binary'].shape == (3, 1, 37, 41) and (c['l1_scale'], c['bce_scale']) != (10, 5)
    c, r = R['grid_stride']
    assert c['pred']['binary'].numel() == 5 * 240 * 240 > 262144
    c, r = R['tiny']
    assert c['pred']['binary'].shape == (3, 1, 1, 7)
    c, r = R['exact_l1_zero']
    hit = c['l1_zero']
    assert int(hit.sum()) >= 4 and not r['g_thresh'][:, 0][hit].any()
    assert torch.equal(c['pred']['thresh'][:, 0][hit], c['batch']['thresh_map'][hit])


@pytest.mark.parametrize("name", [n for n in REGIMES if n not in TIE_REGIMES])
def test_threshold_is_isolated(name):
    """The elements a float32 evaluation may put on either side of the threshold are excluded from the element-wise gradient
    comparison, so they must be few: 0.1 % of the N * HW elements.  The threshold element itself always belongs to the set
    (|v - v| = 0), so the bound is max(1, N*HW / 1000): at the shapes below 1000 elements, the threshold element alone."""
    c, r = case_and_reference(name)
    n = c['pred']['binary'].numel()
    near = int(r['near'].sum())
    assert near <= max(1, n // 1000), (near, n)
    if r['nc'] == 0:
        assert near == 0


@pytest.mark.parametrize("name", [n for n in REGIMES if n not in ("no_positives", "positives_all_masked")])
def test_inputs_tell_the_selection_apart(name):
    """nc - 1 or nc + 1 elements, or a selection without the [N, N, H, W] broadcast, move bce by more than 20x the tolerance
    of the GPU comparison.  Where every negative is taken (nc = their number) there is no nc + 1, and the broadcast cancels
    out of bce: sum_ab l[b] mask[b] (gt[a] + 1 - gt[a]) / sum_ab mask[b] -- those two reruns apply to the selecting regimes."""
    c, r = case_and_reference(name)
    p, b = c['pred']['binary'].double(), {k: v.double() for k, v in c['batch'].items()}
    args = (p, b['gt'], b['mask'], c['negative_ratio'], c['eps'])
    base = float(balanced_bce(*args))
    assert base == r['bce']                       # the restatement with a movable count IS the reference at k_delta = 0
    bar = 20 * LOSS_TOL * max(1.0, abs(base))
    deltas = [-1] + ([1] if r['nc'] < r['n_neg'] else [])
    for d in deltas:
        assert abs(float(balanced_bce(*args, k_delta=d)) - base) > bar, (d, base)
    if r['nc'] < r['n_neg']:
        assert abs(float(balanced_bce(*args, broadcast=False)) - base) > bar


@pytest.mark.parametrize("name", REGIMES)
def test_device_count_restatement_agrees(name):
    """BalanceCrossEntropyLoss(host_counts=False) -- sort and take the first nc, counts as tensors -- on float64 CPU tensors."""
    from megreader_amd.decoders.seg_detector_loss import BalanceCrossEntropyLoss
    c, r = case_and_reference(name)
    p = c['pred']['binary'].double().requires_grad_(True)
    b = {k: v.double() for k, v in c['batch'].items()}
    bce = BalanceCrossEntropyLoss(negative_ratio=c['negative_ratio'], eps=c['eps'], host_counts=False)(p, b['gt'], b['mask'])
    assert abs(float(bce.detach()) - r['bce']) <= 1e-12 * max(1.0, abs(r['bce']))
    (bce * c['bce_scale'] * UPSTREAM).backward()
    keep = ~r['near'] if name != "zero_losses" else (r['l'] > 0)
    scale = float(r['g_binary'].abs().max())
    assert float(((p.grad - r['g_binary']) * keep).abs().max()) <= 1e-12 * scale
    assert abs(float(p.grad.sum()) - float(r['g_binary'].sum())) <= 1e-9 * float(r['g_binary'].abs().sum()) + 1e-300
