"""The sub-sequence JPEG decoder without a GPU: the restatement (tests/_jpeg_split_ref.py) against the serial restatement
(tests/_jpeg_ref.py, which tests/test_jpeg_decode_cpu.py holds against PIL), the host split plan (mr_jpeg_plan_split) against
the restatement's table, and the coverage the fixtures of tests/golden/jpeg_split/ are chosen for."""
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _jpeg_ref as ref  # noqa: E402
import _jpeg_split_ref as sref  # noqa: E402
from megreader_amd.data import jpeg_decode as jd  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_split")
NAMES = ["c420_300x200_q75", "c444_101x33_q95", "c422_120x48_q50_opt", "gray_256x64_q30_opt", "c420_300x200_q75_rst5rows",
         "c444_1x1"]
SIZES = [16, 32, 128, 1024]


def blob_of(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def serial():
    """{name: (blob, parsed, _jpeg_ref's BGR pixels)}: computed once, never modified."""
    out = {}
    for name in NAMES:
        blob = blob_of(name)
        pixels = ref.decode(blob)
        pixels.setflags(write=False)
        out[name] = (blob, ref.parse(blob), pixels)
    return out


def test_the_fixture_files_are_the_documented_ones():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "*.jpg"))) == sorted(
        n + ".jpg" for n in NAMES + ["pad640_c420_q75", "pad640_c444_q50", "reader_scene0", "reader_scene1", "reader_scene2"])
    p = ref.parse(blob_of("c420_300x200_q75_rst5rows"))
    assert len(p.items) > 1 and all(length > 1024 for _, _, _, length in p.items)
    for name in NAMES:
        if "rst" not in name:
            assert len(ref.parse(blob_of(name)).items) == 1, name


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_serial_decoder(serial, name, S):
    blob, p, pixels = serial[name]
    samp = [(p.hs, p.vs)] + [(1, 1)] * (p.ncomp - 1)
    got = [np.zeros((p.mcu_h * sv, p.mcu_w * sh, 64), dtype=np.int64) for sh, sv in samp]
    want = [np.zeros_like(c) for c in got]
    for mcu0, nmcu, off, length in p.items:
        data = blob[off:off + length]
        st = sref.Stream(p, data, nmcu, S)
        ins, exits, counts, _, _ = st.synchronise()
        states, blocks = st.serial_states()
        assert ins == states                                              # the repaired entry states are the serial walk's
        assert counts == blocks and exits[:-1] == states[1:]
        assert sref.item_coefficients(p, data, mcu0, nmcu, S, got) == ref.OK
        assert ref._decode_item(data, p, mcu0, nmcu, want) == ref.OK
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    out, status = sref.decode_status(blob, S)
    assert status == ref.OK and np.array_equal(out, pixels)
    assert np.array_equal(sref.decode_status(blob, S, rgb=True)[0], pixels[:, :, ::-1])


def test_the_fixtures_cover_what_they_are_chosen_for(serial):
    blob, p, _ = serial["c420_300x200_q75"]
    (_, nmcu, off, length), = p.items
    st = sref.Stream(p, blob[off:off + length], nmcu, 16)
    assert st.n_sub > 2 * sref.WG                                         # more than two workgroups' worth
    states, _ = st.serial_states()
    assert any(states[g * sref.WG] != st.guess(g * sref.WG) for g in range(1, -(-st.n_sub // sref.WG)))   # a wrong boundary guess
    dist = [st.sync_distance(i, states) for i in range(st.n_sub)]
    assert max(d for d in dist if d is not None) > 3
    assert any(d is None for d in dist)                                   # a sub-sequence that never synchronises
    _, _, _, rounds, redone = st.synchronise()
    assert max(rounds) > 3 and sum(redone) >= 1                           # the device schedule needs its rounds and its passes
    # the 4:4:4 q95 file still has a never-synchronising sub-sequence at 128 bytes
    blob, p, _ = serial["c444_101x33_q95"]
    (_, nmcu, off, length), = p.items
    st = sref.Stream(p, blob[off:off + length], nmcu, 128)
    states, _ = st.serial_states()
    assert any(st.sync_distance(i, states) is None for i in range(st.n_sub))


def host_plan(blobs, split_above, S):
    plan = jd.make_plan(blobs)
    before = (bytes(plan.images), bytes(plan.items), plan.workspace_bytes)
    plan.split(split_above, S)
    return plan, before


@pytest.mark.parametrize("S", SIZES)
def test_host_split_plan_equals_the_restatement(serial, S):
    blobs = [serial[n][0] for n in NAMES] + [b"not a jpeg"]
    for split_above in (0, 1024, 6000):
        plan, before = host_plan(blobs, split_above, S)
        table, total = sref.split_table([ref.parse(b) for b in blobs], split_above, S)
        assert plan.n_splits == len(table) and plan.workspace_bytes == total
        assert total >= before[2]
        for got, want in zip(plan.split_table(), table):
            for field, _ in jd.JpegSplit._fields_:
                assert getattr(got, field) == want[field], (field, want['item'])
            assert plan.items[got.item].reserved == 1 + table.index(want)
            # every region lies inside the grown workspace, 16-byte aligned and behind the planes
            regions = [(got.meta_off, 16), (got.raw_off, got.raw_bytes), (got.in_off, 8 * got.n_sub), (got.exit_off, 8 * got.n_sub),
                       (got.wg_exit_off, 16 * got.n_wg), (got.block_off, 4 * got.n_sub), (got.coef_off, got.coef_bytes)]
            for off, size in regions:
                assert off % 16 == 0 and before[2] <= off and off + size <= plan.workspace_bytes
            assert all(a + s <= b for (a, s), (b, _) in zip(regions, regions[1:]))
        split_items = {e['item'] for e in table}
        assert [i for i in range(plan.n_items) if plan.items[i].reserved] == sorted(split_items)
    if S == 16:
        assert any(e['n_wg'] >= 3 for e in table) or split_above != 0


def test_a_threshold_above_every_item_changes_nothing(serial):
    blobs = [serial[n][0] for n in NAMES]
    plan, before = host_plan(blobs, 1 << 20, 128)
    assert plan.n_splits == 0 and plan.sections()[3:] == []
    assert (bytes(plan.images), bytes(plan.items), plan.workspace_bytes) == before


def test_split_plan_refuses_bad_sizes(serial):
    plan = jd.make_plan([serial[NAMES[0]][0]])
    for S in (0, 12, 18, 1028):
        with pytest.raises(RuntimeError, match="subseq_bytes"):
            jd.make_plan([serial[NAMES[0]][0]]).split(0, S)
    with pytest.raises(ValueError):
        jd.JpegDecoder(device="cpu", split_above=0, subseq_bytes=18)
    assert plan.n_splits == 0


def flipped(blob, p, count=20, seed=77):
    """`count` copies of the file with one byte in the middle half of its entropy-coded segment inverted (never into or out
    of FF, so that the marker structure stays)."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        at = p.scan_off + p.scan_len // 4 + int(rng.randint(p.scan_len // 2))
        new = blob[at] ^ 0xFF
        if blob[at] == 0xFF or new == 0xFF or blob[at - 1] == 0xFF:
            continue
        out.append(blob[:at] + bytes([new]) + blob[at + 1:])
    return out


def damaged(blob, p):
    """{name: blob}: cut in half, 200 bytes of AA in front of the EOI, and the 20 byte flips."""
    end = p.scan_off + p.scan_len
    cases = {"truncated": blob[:p.scan_off + p.scan_len // 2], "padded": blob[:end] + b"\xAA" * 200 + blob[end:]}
    cases.update(("flip%02d" % i, b) for i, b in enumerate(flipped(blob, p)))
    return cases


@pytest.mark.parametrize("S", [16, 128])
def test_status_equals_the_serial_decoder_on_damaged_streams(serial, S):
    blob, p, _ = serial["c420_300x200_q75"]
    cases = damaged(blob, p)
    assert ref.decode_status(cases["truncated"])[1] == ref.CORRUPT
    seen = set()
    for name, bad in cases.items():
        want_px, want = ref.decode_status(bad)
        got_px, got = sref.decode_status(bad, S)
        assert got == want, name
        seen.add(want)
        if want == ref.OK:
            assert np.array_equal(got_px, want_px), name
    assert sref.decode_status(cases["truncated"], S)[1] == ref.CORRUPT
    assert seen == {ref.OK, ref.CORRUPT}                                  # the flips exercise both outcomes
