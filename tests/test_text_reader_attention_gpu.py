"""TextReader(decode='attention'): text, score, alternatives and character boxes from an attention recogniser.  The detector and
the photos are the recipe of tests/test_text_reader_scores_gpu.py, restated (dark photos with bright rectangles, a detector that
turns brightness into a probability); the recogniser is the analytically known decoder of tests/test_attention_eval_gpu.py
(next word = pi(last word), every step's probability 1 to float32) behind a stub backbone, with an attention that is made one-hot
at column s for character s."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import megreader_amd as mr  # noqa: E402
from megreader_amd import TextReader  # noqa: E402
from megreader_amd.decoders import AttentionDecoder  # noqa: E402
from megreader_amd.nn import functional as Fn  # noqa: E402

DEV = "cuda"
H = 512
A, B = 60.0, 20.0
DET_SIZE = (240, 320)
REC_SIZE = (16, 64)                       # the decoder's encoder takes 16 x 64 features down to 1 x 32
SCENES = [((120, 160), [((50.0, 30.0), 0.0, 135), ((100.0, 85.0), 20.0, 255)]),
          ((150, 200), [((60.0, 110.0), 0.0, 215), ((140.0, 40.0), 0.0, 175)]),
          ((90, 120), [])]                                   # a photo without boxes
CYCLE = [0, 5, 9, 3, 20, 11, 37]          # pi^7(blank) = blank: six characters, then the blank
L, V = 8.0, 200.0


@pytest.fixture(autouse=True)
def _reset():
    yield
    mr.set_compute_dtype(torch.bfloat16)
    Fn.LSTM_STATUS = None


def paint(shape, rects):
    photo = np.zeros(shape + (3,), dtype=np.uint8)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    for (cx, cy), angle, level in rects:
        t = math.radians(angle)
        along = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
        across = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
        photo[(np.abs(along) <= A / 2) & (np.abs(across) <= B / 2)] = level
    return photo


def photos():
    return [paint(shape, rects) for shape, rects in SCENES]


def detector(x):
    """Pixels brighter than the mean are text, the surer the brighter (0.86 .. 1)."""
    v = x[:, :1]
    return {'binary': torch.where(v > 0, (0.85 + 0.3 * v).clamp(max=1.0), torch.zeros_like(v))}


def known_decoder():
    """The permutation decoder, and an attention that looks at column s in step s.  The state entering step s >= 1 is the +-1
    pattern tanh(4) P[c_s] of the word fed one step earlier (c_1 = blank, c_2 = the first character, ..), so a hidden projection
    W with W (tanh(4) P[c_s]) = D[s] exists (38 patterns in 512 dimensions): D[s][h] = 0 at h = s and -2 L at the other h < 32, and
    -3 L at h = 32.  eproj of column t is +L at h = t and at h = 32 +L for t = 0, -L else; v = V on those 33 units.  Then in step
    s >= 1 unit h contributes V tanh(L) at h = s = t, V tanh(-L) at h = t != s and V tanh(0) at h = s != t: column s leads by V.
    In step 0 the state is 0, every column gets V tanh(L) from its own unit, and unit 32 puts column 0 ahead by 2 V."""
    torch.manual_seed(3)
    dec = AttentionDecoder(in_channels=256)
    cell = dec.decoder
    C = len(dec.charset)
    pi = list(range(C))
    for a, b in zip(CYCLE, CYCLE[1:] + CYCLE[:1]):
        pi[a] = b
    g = torch.Generator().manual_seed(8)
    P = (torch.randint(0, 2, (C, H), generator=g) * 2 - 1).float()
    S = dec.max_size
    with torch.no_grad():
        cell.word_linear.weight.copy_(P.t())
        cell.word_linear.bias.zero_()
        cell.rnn.weight_ih.zero_()
        cell.rnn.weight_ih[2 * H:, :H] = 4 * torch.eye(H)
        cell.rnn.weight_hh.zero_()
        cell.rnn.bias_hh.zero_()
        cell.rnn.bias_ih.zero_()
        cell.rnn.bias_ih[H:2 * H] = -30
        cell.out.weight.copy_(P[torch.argsort(torch.tensor(pi))])
        cell.out.bias.zero_()
        # the attention
        D = torch.zeros(C, H, dtype=torch.float64)
        fed = [0] + CYCLE[1:]                                   # c_s for s = 1, 2, ..: blank, then the characters
        for s, c in enumerate(fed, start=1):
            D[c, :S] = -2 * L
            D[c, s] = 0.0
            D[c, S] = -3 * L
        Pd = P.double() * math.tanh(4.0)
        W = D.t() @ torch.linalg.solve(Pd @ Pd.t(), Pd)          # W Pd[c] = D[c]
        cell.attn.attn.weight.zero_()
        cell.attn.attn.bias.zero_()
        cell.attn.attn.weight[:, :H] = W.float()
        x0 = H + 512 + dec.height                               # the one-hot x position of the encoder sequence
        for t in range(S):
            cell.attn.attn.weight[t, x0 + t] = L
            cell.attn.attn.weight[S, x0 + t] = L if t == 0 else -L
        cell.attn.v.zero_()
        cell.attn.v[:S + 1] = V
    return dec.to(DEV).eval()


class Model(torch.nn.Module):
    """A recogniser with .backbone and .decoder, as tests/_cases.py:fpn_attention_n32_hip builds it."""

    class Backbone(torch.nn.Module):
        def forward(self, crops):
            return crops[:, :1].expand(-1, 256, -1, -1).contiguous()

    def __init__(self, decoder):
        super().__init__()
        self.backbone = Model.Backbone()
        self.decoder = decoder

    def forward(self, crops):
        return self.decoder(self.backbone(crops), train=False)


_MODEL = {}


def model():
    if "m" not in _MODEL:
        _MODEL["m"] = Model(known_decoder())
    return _MODEL["m"]


def reader(**kw):
    m = model()
    return TextReader(detector, m, m.decoder.charset, det_size=DET_SIZE, rec_size=REC_SIZE, **kw)


def known_text():
    return model().decoder.charset.label_to_string(CYCLE[1:])


def test_text_score_and_alternatives():
    text = known_text()
    assert len(text) == 6
    for kw in (dict(), dict(beam_width=4, nbest=3)):
        results = reader(decode='attention', **kw).read(photos())
        assert [len(found) for found in results] == [2, 2, 0]
        for item in (item for found in results for item in found):
            assert set(item) == {'quad', 'text', 'text_score'} | ({'alternatives'} if kw else set())
            assert item['text'] == text and abs(item['text_score']) < 1e-3
            if kw:
                alts = item['alternatives']
                assert len(alts) == 3 and alts[0] == (text, item['text_score'])
                assert all(a[1] >= b[1] for a, b in zip(alts, alts[1:])) and all(math.isfinite(a[1]) for a in alts)
                assert len({a[0] for a in alts}) == 3


def test_lexicon_word_of_the_decoded_string_and_boxes_of_the_raw_string():
    text = known_text()
    word = text[:5] + ("A" if text[5] != "A" else "B")
    results = reader(decode='attention', lexicon=[word, "ZZ"], chars=True).read(photos())
    for item in (item for found in results for item in found):
        assert (item['text'], item['raw_text'], item['lexicon_distance']) == (word, text, 1)
        assert "".join(c['char'] for c in item['chars']) == text                  # the boxes stay those of what was read
    with pytest.raises(ValueError, match="needs decode='ctc'"):
        reader(decode='attention', lexicon=[word], lexicon_rule='likelihood')


@pytest.mark.parametrize("beam", [1, 4])
def test_character_boxes_are_the_attended_columns(beam):
    rd = reader(decode='attention', beam_width=beam, chars=True)
    imgs = photos()
    results = rd.read(imgs)
    # the crop plans, as `read` makes them
    batch, on_device = rd._upload(imgs)
    boxes, _ = rd.representer.represent({'image': batch['image'], 'shape': [im.shape[:2] for im in imgs]}, detector(batch['image']))
    staged, layout = rd.cropper.pack(on_device, boxes)
    index = staged.numpy()[layout.index_off:layout.index_off + 4 * layout.M].view(np.int32).tolist()
    assert layout.M == 4
    text = known_text()
    seen = [0] * len(imgs)
    for i, plan in zip(index, layout.plans):
        item = results[i][seen[i]]
        seen[i] += 1
        Hc, Wc = plan.canvas
        assert (Hc, Wc) == REC_SIZE and len(item['chars']) == 6
        for s, ch in enumerate(item['chars']):
            u0, u1 = s * Wc / 32.0, (s + 1) * Wc / 32.0
            want = plan.canvas_to_photo([[u0, 0.0], [u1, 0.0], [u1, float(Hc)], [u0, float(Hc)]])
            assert ch['char'] == text[s] and abs(ch['score'] - 1.0) < 1e-3
            assert float(np.abs(np.asarray(ch['quad']) - want).max()) < 1e-3, (s, ch['quad'], want.tolist())
    # a wider extent changes nothing while the maps have no spread; the least box is half a cell either side of the mean
    again = reader(decode='attention', beam_width=beam, chars=True, attention_extent=4.0).read(imgs)
    assert again == results


class Reads(torch.nn.Module):
    """A recogniser with its own `read`: every crop spells 5, unknown, 9 and ends; the maps sit on the cells 2, 7 and 11 of a
    1 x 32 grid, the last one spread by one cell."""
    height, max_size = 1, 32

    def read(self, crops, beam=1, nbest=1):
        M, S = crops.shape[0], self.max_size
        ids = torch.zeros((M, 1, S), dtype=torch.int32, device=crops.device)
        ids[:, 0, :3] = torch.tensor([5, 1, 9], dtype=torch.int32)
        sym_lp = torch.full((M, S), -50.0, device=crops.device)
        sym_lp[:, :3] = torch.log(torch.tensor([0.5, 0.25, 0.125]))
        moments = torch.zeros((M, S, 4), device=crops.device)
        moments[:, :3, 0] = torch.tensor([2.5, 7.5, 11.5])
        moments[:, :, 1] = 0.5
        moments[:, 2, 2] = 1.0
        return dict(ids=ids, lengths=torch.full((M, 1), 3, dtype=torch.int32, device=crops.device),
                    scores=torch.full((M, 1), -1.0, device=crops.device),
                    count=torch.ones((M,), dtype=torch.int32, device=crops.device), sym_lp=sym_lp, moments=moments)


def test_a_recogniser_with_its_own_read_and_an_unknown_step():
    charset = model().decoder.charset
    assert int(charset.unknown) == 1
    rd = TextReader(detector, Reads(), charset, det_size=DET_SIZE, rec_size=REC_SIZE, decode='attention', chars=True)
    imgs = photos()
    results = rd.read(imgs)
    batch, on_device = rd._upload(imgs)
    boxes, _ = rd.representer.represent({'image': batch['image'], 'shape': [im.shape[:2] for im in imgs]}, detector(batch['image']))
    staged, layout = rd.cropper.pack(on_device, boxes)
    index = staged.numpy()[layout.index_off:layout.index_off + 4 * layout.M].view(np.int32).tolist()
    text = charset.label_to_string([5, 9])
    seen = [0] * len(imgs)
    for i, plan in zip(index, layout.plans):
        item = results[i][seen[i]]
        seen[i] += 1
        assert item['text'] == text and item['text_score'] == -1.0
        assert [c['char'] for c in item['chars']] == list(text)                       # the unknown step has no entry
        assert [round(c['score'], 6) for c in item['chars']] == [0.5, 0.125]
        Hc, Wc = plan.canvas
        # half a cell either side of 2.5; 1.5 standard deviations of one cell either side of 11.5; 2 pixels a cell
        for ch, (c0, c1) in zip(item['chars'], [(2.0, 3.0), (10.0, 13.0)]):
            u0, u1 = c0 * Wc / 32.0, c1 * Wc / 32.0
            want = plan.canvas_to_photo([[u0, 0.0], [u1, 0.0], [u1, float(Hc)], [u0, float(Hc)]])
            assert float(np.abs(np.asarray(ch['quad']) - want).max()) < 1e-3


def test_the_other_modes_are_unchanged():
    plain = reader(decode='ids').read(photos())
    read = reader(decode='attention').read(photos())
    assert all(set(item) == {'quad', 'text'} for found in plain for item in found)
    assert [[(item['quad'], item['text']) for item in found] for found in read] == \
        [[(item['quad'], item['text']) for item in found] for found in plain]
    assert reader(decode='ids').beam_width == 8 and reader(decode='attention').beam_width == 1
