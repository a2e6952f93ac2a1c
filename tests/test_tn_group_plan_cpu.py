"""Host-side launch planner of the recorded 128x128 TN weight-gradient GEMMs (mr_tn_group_plan; csrc/gemm_conv.hip: tn_group_plan).

mr_tn_flush launches dense problems (LSTM / Linear weight gradients) and row-table conv problems (1x1, strided and non-3x3 layers)
together, up to mr_tn_capacity(0) per launch, and cuts every problem into splits of its own.  The model, in dense p-steps: a launch
costs ceil(workgroups / (2 * CUs)) * (longest workgroup + 20) * (1.3 when workgroups share CUs), a conv p-step counts 1.02.  Every
property here is the kernel's contract (igemm_tn_glds_grouped_kernel): a problem's workgroup range starts at a multiple of 8, holds
tiles * splits workgroups, no workgroup is empty.  The cap: the merged plan is never modelled dearer than the partition it
replaces -- dense and conv problems in launches of their own, up to 12 each, one common p-step count L per launch.
"""
import ctypes

import pytest

from megreader_amd import _lib

CUS = 256       # MI355X


def cdiv(a, b):
    return (a + b - 1) // b


def _arr(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _plan(problems, cus=CUS):
    """problems: (tiles, steps, mode) in recording order -> (launches, launch[], splits[], begin[], cost)"""
    n = len(problems)
    launch, splits, begin = _arr([0] * n), _arr([0] * n), _arr([0] * n)
    cost = ctypes.c_double(-1.0)
    launches = _lib.load().mr_tn_group_plan(cus, n, _arr([p[0] for p in problems]), _arr([p[1] for p in problems]),
                                           _arr([p[2] for p in problems]), launch, splits, begin, ctypes.byref(cost))
    assert launches >= 1, _lib.load().mr_last_error()
    return launches, list(launch), list(splits), list(begin), cost.value


def _cost(problems, splits, cus=CUS):
    cost = ctypes.c_double(-1.0)
    n = len(problems)
    rc = _lib.load().mr_tn_group_cost(cus, n, _arr([p[0] for p in problems]), _arr([p[1] for p in problems]),
                                      _arr([p[2] for p in problems]), _arr(splits), ctypes.byref(cost))
    assert rc == 0, _lib.load().mr_last_error()
    return cost.value


def _dense(NA, NB, P):
    return (cdiv(NA, 128) * cdiv(NB, 128), cdiv(P, 64), 0)


def _conv(Cout, Cin, RS, P):
    return (cdiv(Cout, 128) * cdiv(Cin * RS, 128), cdiv(P, 64), 2)


def _crnn():
    """The flagship step (batch 256, T = 33): conv6 (2x2, 512 -> 512, 33 x 256 positions), BiLSTM-2 with the class Linear, BiLSTM-1
    with its Linear, conv1 (3x3, 64 channels stored for 3, 32 x 128 positions per image) -- in backward order."""
    T, N, H = 33, 256, 256
    lstm2 = [_dense(38, 512, T * N), _dense(38, 8, T * N)] + [_dense(4 * H, 256, T * N)] * 2 + [_dense(4 * H, H, (T - 1) * N)] * 2
    lstm1 = [_dense(256, 512, T * N)] + [_dense(4 * H, 512, T * N)] * 2 + [_dense(4 * H, H, (T - 1) * N)] * 2
    return lstm2 + lstm1 + [_conv(512, 512, 4, T * N), _conv(64, 64, 9, 256 * 32 * 32)]


def _resnet50(N, size):
    """1x1 and downsample layers of the four ResNet-50 stages at N x size x size, last layer first: the problem kinds the
    Res50-PPM step records (the 3x3 layers go to the all-taps kernel)."""
    out = []
    for planes, blocks, res in ((512, 3, size // 32), (256, 6, size // 16), (128, 4, size // 8), (64, 3, size // 4)):
        P = N * res * res
        for b in reversed(range(blocks)):
            cin = planes * 4 if b else (planes * 2 if planes > 64 else 64)
            out.append(_conv(planes * 4, planes, 1, P))                      # conv3
            out.append(_conv(planes, cin, 1, P if b or planes == 64 else P * 4))   # conv1 (first block: before the stride)
            if b == 0:
                out.append(_conv(planes * 4, cin, 1, P))                     # downsample
    return out


def _fpn_attention():
    """FPN laterals (1x1 to 256 channels at strides 4..32 of a 32 x 512 x 512 batch), the 1x1 output convs, and the Linear
    layers of the attention decoder (64 samples x 32 steps)."""
    lat = [_conv(256, c, 1, 32 * (512 // s) ** 2) for c, s in ((2048, 32), (1024, 16), (512, 8), (256, 4))]
    outs = [_conv(64, 256, 1, 32 * (512 // s) ** 2) for s in (32, 16, 8, 4)]
    attn = [_dense(552, 512, 64 * 32), _dense(2048, 512, 64 * 32), _dense(2048, 768, 64 * 32), _dense(512, 512, 64 * 32),
            _dense(512, 256, 64 * 32 * 8)]
    return attn + lat + outs


def _sets():
    cap = _lib.load().mr_tn_capacity(0)
    r50 = _resnet50(32, 224)
    return {
        "crnn": _crnn(),
        "res50ppm_head": r50[:cap],            # what one early flush holds: a full launch
        "res50ppm_all": r50,                   # more than one launch
        "fpn_attention": _fpn_attention(),
        "single_dense": [_dense(1024, 256, 8448)],
        "single_conv": [_conv(64, 64, 9, 262144)],
        "over_capacity": (_crnn() * 2)[:cap + 1],
        "tiny": [_dense(8, 8, 40), _conv(24, 8, 4, 10)],
    }


SET_NAMES = ["crnn", "res50ppm_head", "res50ppm_all", "fpn_attention", "single_dense", "single_conv", "over_capacity", "tiny"]


def test_capacity_holds_the_crnn_step():
    lib = _lib.load()
    assert lib.mr_tn_capacity(0) >= 13 and lib.mr_tn_capacity(1) == 12 and lib.mr_tn_capacity(2) == 0
    assert len(_crnn()) == 13 and sum(1 for p in _crnn() if p[2] == 0) == 11
    assert lib.mr_tn_pending_of(0) == 0 and lib.mr_tn_pending_of(1) == 0        # no device, nothing recorded


@pytest.mark.parametrize("name", SET_NAMES)
def test_plan_invariants(name):
    problems = _sets()[name]
    cap = _lib.load().mr_tn_capacity(0)
    launches, launch, splits, begin, cost = _plan(problems)
    # runs of at most `cap` records; a run is one launch, or one launch per mode; launches are numbered by first problem
    assert cdiv(len(problems), cap) <= launches <= 2 * cdiv(len(problems), cap)
    firsts = [launch.index(l) for l in range(launches)]
    assert firsts == sorted(firsts) and set(launch) == set(range(launches))
    total_cost = 0.0
    for l in range(launches):
        idx = [i for i in range(len(problems)) if launch[i] == l]
        assert 1 <= len(idx) <= cap
        if launches > cdiv(len(problems), cap) and len({problems[i][2] for i in idx}) > 1:
            assert all(launch[i] == l for i in range(idx[0], idx[-1] + 1))       # a mixed launch is a whole run of records
        ranges = []
        for i in idx:
            tiles, steps, _ = problems[i]
            assert 1 <= splits[i] <= steps
            per = cdiv(steps, splits[i])
            assert (splits[i] - 1) * per < steps, "problem %d: an empty workgroup" % i     # splits == cdiv(steps, per)
            assert begin[i] % 8 == 0
            ranges.append((begin[i], begin[i] + cdiv(tiles * splits[i], 8) * 8))
        ranges.sort()
        assert ranges[0][0] == 0
        for (b0, e0), (b1, e1) in zip(ranges, ranges[1:]):
            assert e0 == b1, "ranges overlap or leave a hole"
        blocks = ranges[-1][1]
        launch_cost = _cost([problems[i] for i in idx], [splits[i] for i in idx])
        total_cost += launch_cost
        # within one round of workgroup slots -- unless the plan prices the rounds it takes: then every cut of the same launch
        # that does fit one round (the fewest splits that do) is modelled no cheaper
        rounds = cdiv(blocks, 2 * CUS)
        if rounds > 1 and len(idx) > 1:
            sub = [problems[i] for i in idx]
            one_round = None
            for L in range(1, max(p[1] for p in sub) + 1):
                cut = [cdiv(p[1], min(L, p[1])) for p in sub]
                if sum(cdiv(p[0] * s, 8) * 8 for p, s in zip(sub, cut)) <= 2 * CUS:
                    one_round = cut
                    break
            if one_round is not None:
                assert launch_cost <= _cost(sub, one_round) + 1e-9
    assert cost == pytest.approx(total_cost, rel=1e-12)
    # deterministic, and the cached plan is the same plan
    assert _plan(problems) == (launches, launch, splits, begin, cost)
    assert _plan(list(problems)) == (launches, launch, splits, begin, cost)


def _legacy_cost(problems):
    """The partition this planner replaces: per mode, launches of up to 12 problems in recording order, ONE p-step count L per
    launch (the L that minimises rounds * (L + 20) * 1.3), a lone problem as an immediate launch -- priced by the same model."""
    total = 0.0
    for mode in (0, 2):
        q = [p for p in problems if p[2] == mode]
        for i0 in range(0, len(q), 12):
            sub = q[i0:i0 + 12]
            if len(sub) == 1:
                total += _cost(sub, _plan(sub)[2])
                continue
            best, best_l = None, None
            for L in range(1, max(p[1] for p in sub) + 1):
                blocks = sum(cdiv(p[0] * cdiv(p[1], L), 8) * 8 for p in sub)
                c = cdiv(blocks, 2 * CUS) * (L + 20.0) * (1.3 if blocks > CUS else 1.0)
                if best is None or c < best:
                    best, best_l = c, L
            cut = []
            for p in sub:
                s = cdiv(p[1], best_l)
                cut.append(cdiv(p[1], cdiv(p[1], s)))
            total += _cost(sub, cut)
    return total


@pytest.mark.parametrize("name", SET_NAMES)
def test_merged_plan_is_modelled_no_dearer_than_the_partition_by_mode(name):
    problems = _sets()[name]
    merged = _plan(problems)[4]
    legacy = _legacy_cost(problems)
    print("%s: merged %.1f, by mode %.1f dense p-steps" % (name, merged, legacy))
    assert merged <= legacy + 1e-9


def test_crnn_step_is_one_launch_of_one_round():
    launches, launch, splits, begin, cost = _plan(_crnn())
    assert launches == 1
    blocks = max(b + cdiv(p[0] * s, 8) * 8 for p, s, b in zip(_crnn(), splits, begin))
    assert blocks <= 2 * CUS
    # the longest workgroups are dispatched first
    order = sorted(range(13), key=lambda i: begin[i])
    times = [cdiv(_crnn()[i][1], splits[i]) * (1.0 if _crnn()[i][2] == 0 else 1.02) for i in order]
    assert times == sorted(times, reverse=True)


def test_cost_model_by_hand():
    # one dense problem, 16 tiles x 128 steps in 8 splits: 128 workgroups of 16 steps on 256 CUs, nothing shared
    assert _cost([(16, 128, 0)], [8]) == pytest.approx(16 + 20.0)
    # 32 splits: 512 workgroups share the CUs
    assert _cost([(16, 128, 0)], [32]) == pytest.approx((4 + 20.0) * 1.3)
    # one more workgroup than slots: two rounds
    assert _cost([(16, 128, 0), (1, 4, 0)], [32, 1]) == pytest.approx(2 * (4 + 20.0) * 1.3)
    # a conv step counts 1.02 dense steps; ranges are padded to 8 workgroups
    assert _cost([(5, 4096, 2)], [64]) == pytest.approx((64 * 1.02 + 20.0) * 1.3)
    assert _cost([(1, 64, 2), (1, 64, 0)], [1, 1]) == pytest.approx(64 * 1.02 + 20.0)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    one, out = _arr([1] * 65), [_arr([0] * 65) for _ in range(3)]
    zero, mode1 = _arr([0] * 65), _arr([1] * 65)
    modes = _arr([0] * 65)
    assert lib.mr_tn_group_plan(256, 65, one, one, modes, *out, None) < 0
    assert lib.mr_tn_group_plan(256, 0, one, one, modes, *out, None) < 0
    assert lib.mr_tn_group_plan(0, 2, one, one, modes, *out, None) < 0
    assert lib.mr_tn_group_plan(256, 2, zero, one, modes, *out, None) < 0
    assert lib.mr_tn_group_plan(256, 2, one, zero, modes, *out, None) < 0
    assert lib.mr_tn_group_plan(256, 2, one, one, mode1, *out, None) < 0
    assert lib.mr_tn_group_plan(256, 2, one, one, modes, None, out[1], out[2], None) < 0
    assert lib.mr_tn_group_plan(256, 2, one, one, modes, *out, None) == 1
    cost = ctypes.c_double()
    assert lib.mr_tn_group_cost(256, 2, one, one, modes, _arr([2, 1]), ctypes.byref(cost)) != 0      # more splits than steps
