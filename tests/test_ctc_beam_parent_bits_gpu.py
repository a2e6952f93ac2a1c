"""mr_ctc_beam_search and mr_ctc_beam_search_lm (csrc/ctc_beam.hip) bit for bit against tests/golden/ctc_beam_parent_bits.npz: the
outputs of the library as it was when the two entry points still had a row kernel each (the commit is named in the file), on the
smallest cases that reach every branch the one row kernel now shares.  tools/make_ctc_beam_fixture.py wrote the file with the
CASES and `decode` below; the inputs are stored in it, nothing is drawn again here.  The model is not stored: `CharNgramLM.train`
builds it from WORDS.

Every case runs without a model, with the order-3 model at (alpha, beta, end) = (0.8, 0.5, 1) and with it at (0, 0, 0); the int32
views of ids, lengths, scores, count -- with a model ctc_scores and lm_scores too -- must be equal."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd.charsets import Charset  # noqa: E402
from megreader_amd.ops.decode import ctc_beam_search_decode  # noqa: E402
from megreader_amd.ops.language_model import CharNgramLM  # noqa: E402

DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_beam_parent_bits.npz")
CHARSET = Charset("abcdefghij", case_sensitive=True)                                    # blank, unknown, a .. j: 12 classes
WORDS = ["bad", "badge", "bead", "beige", "cab", "cabbage", "dice", "each", "face", "fade", "fig", "hid", "hide", "high", "idea",
         "jade", "jab", "add", "age", "ice", "if", "he", "be", "a", "i"]
# name: (stored input [N, T, C], how it is passed, log_probs, beam, nbest, top_classes).  'bf16': the stored int16 are the bits
CASES = {
    "pruned": ("pruned", 'f32', False, 8, 3, 6),
    "pruned_bf16": ("pruned_bf16", 'bf16', False, 8, 3, 6),
    "pruned_logs": ("pruned_logs", 'f32', True, 8, 3, 6),
    "full": ("full", 'f32', False, 64, 64, 64),                                         # all 64 + 4 096 candidate keys
    "smallest": ("smallest", 'f32', False, 1, 1, 1),
    "dead_row": ("dead_row", 'f32', False, 8, 3, 6),                                    # row DEAD has a column on `unknown`
}
DEAD = 2
MODES = {"plain": None, "lm": (0.8, 0.5, 1), "lm_zero": (0.0, 0.0, 0)}
PLAIN = ('ids', 'lengths', 'scores', 'count')
FUSED = PLAIN + ('ctc_scores', 'lm_scores')


def model():
    return CharNgramLM.train(WORDS, CHARSET, order=3)


def decode(stored, case, mode, lm):
    """One call of one case: {output name: numpy array}."""
    key, how, log_probs, beam, nbest, top = CASES[case]
    y = torch.from_numpy(stored[key])                                                    # [N, T, C]
    if how == 'bf16':
        y = y.view(torch.bfloat16)
    pred = y.to(DEV).permute(0, 2, 1).contiguous().unsqueeze(2)                          # the eval layout [N, C, 1, T]
    kw = dict(beam=beam, nbest=nbest, top_classes=top, blank=0, unknown=1, log_probs=log_probs)
    if MODES[mode] is not None:
        alpha, beta, end = MODES[mode]
        kw.update(lm=lm, lm_weight=alpha, lm_bonus=beta, lm_end=end)
    out = ctc_beam_search_decode(pred, **kw)
    return {k: out[k].cpu().numpy() for k in (PLAIN if MODES[mode] is None else FUSED)}


@pytest.fixture(scope="module")
def stored():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def lm():
    return model()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_outputs_are_the_parent_commits_bits(stored, lm, case, mode):
    assert len(str(stored['parent_commit'])) == 40
    got = decode(stored, case, mode, lm)
    for key, value in got.items():
        want = stored["%s.%s.%s" % (case, mode, key)]
        assert value.dtype == want.dtype and value.shape == want.shape, (key, value.dtype, value.shape)
        assert np.array_equal(value.view(np.int32), want.view(np.int32)), (case, mode, key)
    if case == "dead_row":
        assert got['count'][DEAD] == 0 and np.all(got['lengths'][DEAD] == 0) and np.all(got['ids'][DEAD] == 0)
        for key in got:
            if key.endswith('scores'):
                assert np.all(got[key][DEAD] == -np.inf), key
        assert np.all(np.delete(got['count'], DEAD) > 0)
