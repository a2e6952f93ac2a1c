"""The restatement of CTC prefix beam search (tests/_ctc_beam_ref.py) against enumeration of every path, its lower-bound property
on pruned runs, the host-only workspace query of the library and the argument checks of `ctc_beam_search_decode`.  No GPU."""
import numpy as np
import pytest
import torch

import _ctc_beam_ref as B
from megreader_amd import _lib
from megreader_amd.ops.decode import ctc_beam_search_decode

# (C, T, unknown, distinct labelings): every string over the symbols that fits T columns (a repeat needs a blank between)
ENUMERATION_SHAPES = [(3, 5, -1, 25), (3, 6, -1, 41), (4, 3, -1, 25), (4, 4, -1, 61), (5, 3, -1, 57), (4, 4, 1, None)]


@pytest.mark.parametrize("C,T,unknown,labelings", ENUMERATION_SHAPES)
def test_float64_restatement_equals_enumeration_of_all_paths(C, T, unknown, labelings):
    rng = np.random.RandomState(10 * C + T)
    for y in B.posterior(rng, 4, T, C, sharp=1.5):
        want = B.enumerate_strings(y, blank=0, unknown=unknown)
        if labelings is not None:
            assert len(want) == labelings
        assert len(want) <= 64
        got = B.beam_search(B.log_probs(y, np.float64), 64, 64, C, blank=0, unknown=unknown, dtype=np.float64)
        assert len(got['hyps']) == len(want)
        assert {p for p, _ in got['hyps']} == set(want)
        scores = [s for _, s in got['hyps']]
        assert scores == sorted(scores, reverse=True)
        for p, s in got['hyps']:
            assert abs(s - want[p]) <= 1e-12, (p, s, want[p])
        # on the f32 table of logs that the device reads, the rounding of the logs is all that differs
        for p, s in B.beam_search(B.logs(y), 64, 64, C, blank=0, unknown=unknown, dtype=np.float64)['hyps']:
            assert abs(s - want[p]) <= 1e-6, (p, s, want[p])


def test_unknown_mass_is_lost_and_never_emitted():
    y = B.posterior(np.random.RandomState(3), 1, 4, 4, sharp=1.0)[0]
    got = B.beam_search(B.logs(y), 64, 64, 4, blank=0, unknown=1)
    assert all(1 not in p for p, _ in got['hyps'])
    assert np.exp([s for _, s in got['hyps']]).sum() < 1.0 - y[:, 1].min()


@pytest.mark.parametrize("beam,top", [(1, 1), (2, 3), (4, 2), (8, 4)])
def test_pruned_scores_are_lower_bounds(beam, top):
    rng = np.random.RandomState(beam * 7 + top)
    for y in B.posterior(rng, 8, 10, 7, sharp=1.5):
        lp = B.logs(y)
        got = B.beam_search(lp, beam, beam, top, blank=0, unknown=1)
        assert 1 <= len(got['hyps']) <= beam
        assert len({p for p, _ in got['hyps']}) == len(got['hyps'])       # merged by content: no string twice
        for p, s in got['hyps']:
            assert s <= B.true_score(lp, p, 0, 1) + 1e-12, (p, s)


def test_the_most_probable_string_is_not_the_best_path():
    y = np.array([[0.6, 0.0, 0.4], [0.6, 0.0, 0.4]], dtype=np.float32)      # blank, unknown, A
    got = B.beam_search(B.logs(y), 8, 8, 16)
    assert [p for p, _ in got['hyps']] == [(2,), ()]
    assert abs(np.exp(got['hyps'][0][1]) - 0.64) < 1e-7 and abs(np.exp(got['hyps'][1][1]) - 0.36) < 1e-7
    assert y.argmax(axis=1).tolist() == [0, 0]                            # the best path spells ""
    # beam 1 keeps "A" after the first column?  No: "" (0.6) beats "A" (0.4) there, and "" + A in column 2 is 0.24 against 0.36
    assert B.beam_search(B.logs(y), 1, 1, 16)['hyps'][0][0] == ()


def test_reentry_beside_a_live_child_happens_at_the_shapes_the_device_test_uses():
    y = B.posterior(np.random.RandomState(0), 200, 12, 5, sharp=1.0)
    events = sum(r['reentries'] > 0 for r in B.decode(B.logs(y), 4, 4, 3))
    assert events >= 1


def test_workspace_query_is_positive_monotone_and_refuses_what_the_entry_point_refuses():
    ws = _lib.load().mr_ctc_beam_ws_bytes
    assert ws.restype is _lib.ctypes.c_int
    base = ws(4, 32, 8, 16)
    assert base > 0
    assert ws(5, 32, 8, 16) > base and ws(4, 33, 8, 16) > base and ws(4, 32, 9, 16) > base and ws(4, 32, 8, 17) > base
    assert ws(1, 1, 1, 1) > 0 and ws(8, 4096, 64, 64) > 0
    cap = _lib._DEFINES["MR_SEQ_MEASURE_MAX"]
    assert (_lib._DEFINES["MR_CTC_BEAM_MAX"], _lib._DEFINES["MR_CTC_BEAM_TOP_MAX"]) == (64, 64)
    for bad in ((0, 32, 8, 16), (-1, 32, 8, 16), (4, 0, 8, 16), (4, cap + 1, 8, 16), (4, 32, 0, 16), (4, 32, 65, 16),
                (4, 32, 8, 0), (4, 32, 8, 65), (1 << 20, 4096, 64, 64)):          # the last: above 2 GiB
        assert ws(*bad) == 0, bad
    with pytest.raises(TypeError):
        _lib.call("mr_ctc_beam_ws_bytes", 4, 32, 8, 16)                            # host only: no stream


def test_python_argument_errors_come_before_any_launch():
    ok = torch.full((2, 5, 1, 7), 0.2)
    for kwargs in (dict(beam=0), dict(beam=65), dict(nbest=0), dict(beam=4, nbest=5), dict(top_classes=0), dict(top_classes=65),
                   dict(blank=5), dict(blank=-1)):
        with pytest.raises(ValueError):
            ctc_beam_search_decode(ok, **kwargs)
    with pytest.raises(RuntimeError):
        ctc_beam_search_decode(torch.zeros(2, 5, 2, 7))
    with pytest.raises(RuntimeError):
        ctc_beam_search_decode(torch.zeros(5, 7))
    with pytest.raises(ValueError):
        ctc_beam_search_decode(torch.zeros(2, 5, 0))
    with pytest.raises(ValueError):
        ctc_beam_search_decode(torch.zeros(2, 1, 7))
    with pytest.raises(NotImplementedError):                                       # well-formed, but not on a GPU: no CPU fallback
        ctc_beam_search_decode(ok)


def test_text_reader_argument_errors():
    from megreader_amd.reader import TextReader
    with pytest.raises(ValueError, match="needs decode='ctc'"):
        TextReader(None, None, None, decode='beam', lexicon=[], lexicon_rule='likelihood')
    with pytest.raises(ValueError, match="decode must be"):
        TextReader(None, None, None, decode='beams')
    with pytest.raises(ValueError, match="beam_width"):
        TextReader(None, None, None, decode='beam', beam_width=4, nbest=5)
