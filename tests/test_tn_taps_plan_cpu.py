"""Host-side launch planner of the recorded all-taps weight gradients (mr_tn_taps_plan; csrc/tn_taps.hip: taps_plan).

mr_tn_flush partitions the recorded 3x3 weight-gradient problems into launches and cuts each into splits.  The model, in
chunk-times: a launch costs ceil(sum tiles * splits / (2 * CUs)) * (largest chunks-per-workgroup of its problems + 12).
No GPU is needed: CU and slab counts are arguments.
"""
import ctypes
import itertools
import random

import pytest

from megreader_amd import _lib

FIXED = 12.0
TICKETS = 4096


def cdiv(a, b):
    return (a + b - 1) // b


def plan(cus, slabs, tiles, chunks):
    n = len(tiles)
    arr = ctypes.c_int * n
    launch, splits, cps, cost = arr(), arr(), arr(), ctypes.c_double()
    launches = _lib.load().mr_tn_taps_plan(cus, slabs, n, arr(*tiles), arr(*chunks), launch, splits, cps, ctypes.byref(cost))
    assert launches >= 1
    return launches, list(launch), list(splits), list(cps), cost.value


def launch_cost(cus, members):
    """members: [(tiles, splits, cps)] of one launch."""
    blocks = sum(t * s for t, s, _ in members)
    return cdiv(blocks, 2 * cus) * (max(c for _, _, c in members) + FIXED)


def single_splits(cus, tiles, chunks):
    """The split count launch_tn_taps chooses for a problem that has the launch to itself (4-wave kernel)."""
    best, splits = 1e300, 1
    for s in range(1, chunks + 1):
        blocks = tiles * s
        cost = cdiv(blocks, 2 * cus) * (cdiv(chunks, s) + FIXED)
        if cost < best:
            best, splits = cost, s
        if blocks > 8 * cus:
            break
    cps = cdiv(chunks, splits)
    return cdiv(chunks, cps), cps


def group_of(splits):
    return 4 if splits >= 4 else (2 if splits >= 2 else 1)


def check(cus, slabs, tiles, chunks):
    n = len(tiles)
    launches, launch, splits, cps, cost = plan(cus, slabs, tiles, chunks)
    # every problem in exactly one launch, launches numbered without gaps by their first problem
    assert sorted(set(launch)) == list(range(launches))
    firsts = [launch.index(l) for l in range(launches)]
    assert firsts == sorted(firsts)
    total, singles = 0.0, 0.0
    for i in range(n):
        assert splits[i] >= 1 and cps[i] >= 1
        assert splits[i] * cps[i] >= chunks[i]                       # the reduction is covered ...
        assert (splits[i] - 1) * cps[i] < chunks[i]                  # ... and no workgroup is empty
        s1, c1 = single_splits(cus, tiles[i], chunks[i])
        singles += launch_cost(cus, [(tiles[i], s1, c1)])
    for l in range(launches):
        idx = [i for i in range(n) if launch[i] == l]
        assert len(idx) <= 8                                         # problems per grouped launch
        total += launch_cost(cus, [(tiles[i], splits[i], cps[i]) for i in idx])
        if len(idx) == 1:
            assert (splits[idx[0]], cps[idx[0]]) == single_splits(cus, tiles[idx[0]], chunks[idx[0]])
            continue
        grouped = [i for i in idx if slabs > 0 and group_of(splits[i]) > 1]
        if grouped:                                                  # one slab per workgroup, unique tickets
            assert sum(tiles[i] * splits[i] for i in idx) <= slabs
            assert sum(tiles[i] * cdiv(splits[i], group_of(splits[i])) for i in grouped) <= TICKETS
    assert cost == pytest.approx(total)
    assert total <= singles + 1e-9                                   # never worse than one launch per problem
    return launches, launch, splits, cps, total, singles


CRNN = ([64, 32, 16, 8], [544, 544, 1056, 1056])     # conv5, conv4, conv3, conv2 at batch 256


def test_crnn_layers_are_modelled_cheaper_grouped_than_launched_one_by_one():
    launches, launch, splits, cps, total, singles = check(256, 2 * 256 + 64, *CRNN)
    assert singles == 80 + 46 + 45 + 29                              # today's four launches: 8 / 16 / 32 / 63 splits
    assert total < singles
    assert launches < 4
    # the partition the model prefers: conv5 / conv4 / conv3 fill the 512 slots together, conv2 keeps its own launch
    assert launch == [0, 0, 0, 1] and splits[:3] == [4, 4, 8] and cps[:3] == [136, 136, 132]
    assert (splits[3], cps[3]) == single_splits(256, 8, 1056)
    assert total == (136 + FIXED) + 29


@pytest.mark.parametrize("tiles,chunks", [(64, 544), (32, 544), (16, 1056), (8, 1056), (1, 2), (4, 187), (1, 1), (300, 7),
                                          (5000, 3)])
def test_a_single_problem_keeps_the_split_count_of_the_immediate_launch(tiles, chunks):
    launches, launch, splits, cps, cost = plan(256, 576, [tiles], [chunks])
    assert launches == 1 and launch == [0]
    assert (splits[0], cps[0]) == single_splits(256, tiles, chunks)


@pytest.mark.parametrize("cus,slabs", [(256, 576), (256, 0), (304, 672), (8, 80), (1, 2)])
def test_random_problem_sets(cus, slabs):
    rng = random.Random(cus * 1000 + slabs)
    for _ in range(40):
        n = rng.randint(1, 12)                                       # above 8: the greedy merge
        tiles = [rng.choice([1, 2, 4, 8, 16, 32, 64, 100]) for _ in range(n)]
        chunks = [rng.choice([1, 2, 3, 9, 11, 33, 187, 544, 1056]) for _ in range(n)]
        check(cus, slabs, tiles, chunks)


def test_exhaustive_search_beats_or_ties_every_partition_of_three():
    tiles, chunks = [16, 8, 4], [300, 120, 77]
    _, _, _, _, total, singles = check(256, 576, tiles, chunks)
    assert total <= singles
    # {pair} + {third}: the planner's own cost of the pair (itself the better of merged / apart) plus the third alone
    for pair in itertools.combinations(range(3), 2):
        (third,) = [i for i in range(3) if i not in pair]
        pair_cost = plan(256, 576, [tiles[i] for i in pair], [chunks[i] for i in pair])[4]
        alone = plan(256, 576, [tiles[third]], [chunks[third]])[4]
        assert total <= pair_cost + alone + 1e-9


def test_without_slabs_launches_are_atomics_only_and_unconstrained():
    # 2-chunk problems beside a long one: with no workspace nothing limits the workgroups of a launch to the slab count
    launches, launch, splits, cps, total, singles = check(256, 0, [4, 1, 1], [187, 2, 2])
    assert launches == 1 and splits == [94, 1, 1] and cps == [2, 2, 2]


def test_the_plan_the_gpu_test_relies_on():
    launches, launch, splits, cps, total, singles = check(256, 576, [4, 1, 1], [187, 2, 2])
    assert launches == 1 and splits == [94, 1, 1] and cps == [2, 2, 2]


def test_bad_arguments_are_refused():
    lib = _lib.load()
    arr = ctypes.c_int * 13
    out = [arr() for _ in range(3)]
    ones = arr(*([1] * 13))
    assert lib.mr_tn_taps_plan(256, 576, 13, ones, ones, *out, None) < 0
    assert lib.mr_tn_taps_plan(256, 576, 0, ones, ones, *out, None) < 0
    assert lib.mr_tn_taps_plan(0, 576, 2, ones, ones, *out, None) < 0
    zeros = arr()
    assert lib.mr_tn_taps_plan(256, 576, 2, zeros, ones, *out, None) < 0
