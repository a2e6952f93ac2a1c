"""TextReader (megreader_amd/reader.py) end to end: photos -> detector -> SegDetectorRepresenter -> QuadCropper -> recogniser ->
strings.  The plumbing is checked with stub models whose answers are known -- the detector marks every bright pixel, the recogniser
spells a string chosen by the crop's mean brightness -- and then with a real (randomly initialised) CRNN against the same steps
done by hand.

What the boxes must be.  `SegDetectorRepresenter` treats a region as DB's SHRUNK text kernel and unclips it: an a x b rectangle
comes back grown by d = 1.5 a b / (2 (a + b)) on every side (structure/db_geometry.py `unclip`; 11.25 px for 60 x 20).  So a
painted rectangle is expected back as that rectangle grown by d, within 3 px, after both are put in the order top-left,
top-right, bottom-right, bottom-left."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd import QuadCropper, TextReader  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.ops.decode import ctc_greedy_decode  # noqa: E402
from megreader_amd.structure.db_geometry import mini_box  # noqa: E402

A, B = 60.0, 20.0                                   # every painted rectangle: the crops then hold the same share of bright pixels
GROW = 1.5 * A * B / (2.0 * (A + B))                # the representer's unclip distance
SHARE = A * B / ((A + 2 * GROW) * (B + 2 * GROW))   # bright share of an unclipped box
LEVELS = {135: "AB12", 175: "HELLO", 215: "X9", 255: "TEXT"}
# (photo shape, [(centre, angle in degrees, grey level)]); both photos are 3 : 4 like the detector's input, so the detector's
# resize is isotropic and the unclip distance is the same in photo pixels
SCENES = [((120, 160), [((50.0, 30.0), 0.0, 135), ((100.0, 85.0), 20.0, 255)]),
          ((150, 200), [((60.0, 110.0), 0.0, 215), ((140.0, 40.0), 0.0, 175)]),
          ((90, 120), [])]
DET_SIZE = (240, 320)


def rectangle(a, b, centre, angle):
    t = math.radians(angle)
    c, s = math.cos(t), math.sin(t)
    base = np.array([[-a / 2, -b / 2], [a / 2, -b / 2], [a / 2, b / 2], [-a / 2, b / 2]], dtype=np.float64)
    return base @ np.array([[c, s], [-s, c]]) + np.asarray(centre, dtype=np.float64)


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
    return {'binary': (x[:, :1] > 0).float()}


class SpellByBrightness(torch.nn.Module):
    """[M, C, 1, T] scores that spell LEVELS[g], g the grey level nearest to (mean of channel 0 in grey levels) / SHARE, with a
    blank between the symbols.  Counts its calls."""

    def __init__(self, charset, T=16):
        super().__init__()
        self.charset, self.T, self.batches = charset, T, []

    def forward(self, crops):
        self.batches.append(crops.shape[0])
        grey = (crops[:, 0] * 255.0 + RGB_MEAN[0]).mean(dim=(1, 2)).cpu().numpy() / SHARE
        out = torch.zeros((crops.shape[0], len(self.charset), 1, self.T), dtype=torch.float32)
        for m, g in enumerate(grey):
            text = LEVELS[min(LEVELS, key=lambda level: abs(level - g))]
            ids = [0] * self.T
            ids[1:2 * len(text):2] = [self.charset.index(ch) for ch in text]
            out[m, ids, 0, torch.arange(self.T)] = 1.0
        return out.to(crops.device)


def ordered(quad):
    return np.array(mini_box([tuple(p) for p in quad])[0], dtype=np.float64)


def check(results):
    assert len(results) == len(SCENES)
    for found, (shape, rects) in zip(results, SCENES):
        assert len(found) == len(rects)
        left = list(rects)
        for item in found:
            got = ordered(item['quad'])
            dist = [np.abs(got - ordered(rectangle(A + 2 * GROW, B + 2 * GROW, centre, angle))).max() for centre, angle, _ in left]
            k = int(np.argmin(dist))
            print("box at %s: %.2f px from the painted rectangle grown by %.2f" % (left[k][0], dist[k], GROW))
            assert dist[k] < 3.0
            assert item['text'] == LEVELS[left[k][2]]               # the text of ITS box
            del left[k]
    assert results[2] == []


def test_plumbing_with_stubs():
    charset = EnglishCharset()
    recognizer = SpellByBrightness(charset)
    reader = TextReader(detector, recognizer, charset, det_size=DET_SIZE)
    results = reader.read(photos())
    check(results)
    assert recognizer.batches == [4]
    chunked = SpellByBrightness(charset)
    again = TextReader(detector, chunked, charset, det_size=DET_SIZE, max_crops=2).read(photos())
    assert chunked.batches == [2, 2]
    assert again == results
    assert TextReader(detector, recognizer, charset, det_size=DET_SIZE).read([photos()[2]]) == [[]]
    assert reader.read([]) == []


def test_real_recogniser_reads_what_the_steps_by_hand_read():
    from megreader_amd.backbones import crnn_backbone
    from megreader_amd.decoders import CRNNDecoder

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = crnn_backbone()
            self.decoder = CRNNDecoder(in_channels=512)

        def forward(self, x):
            return self.decoder(self.backbone(x))

    torch.manual_seed(0)
    model = Model().cuda().eval()
    charset = EnglishCharset()
    results = TextReader(detector, model, charset, det_size=DET_SIZE, rec_size=(32, 128)).read(photos())
    assert [len(found) for found in results] == [2, 2, 0]
    quads = [[item['quad'] for item in found] for found in results]
    crops = QuadCropper(image_size=(32, 128)).crop(photos(), quads)
    assert crops['index'].cpu().tolist() == [0, 0, 1, 1]
    with torch.no_grad():
        pred = model(crops['image'])
    assert pred.shape[:3] == (4, len(charset), 1)
    ids, lengths = ctc_greedy_decode(pred)
    by_hand = [charset.label_to_string(row[:int(k)]) for row, k in zip(ids.cpu().numpy(), lengths.cpu().numpy())]
    assert [item['text'] for found in results for item in found] == by_hand


class SoftSpell(SpellByBrightness):
    """The stub's spelling with a quarter of every column's mass spread over all classes: no probability is 0 or 1, so the scores
    of the beam, of the lexicon and of the characters are numbers that can differ."""

    def forward(self, crops):
        hard = super().forward(crops)
        return hard * 0.75 + 0.25 / hard.shape[1]


def item_keys(decode, rule, chars, scores):
    """An item's keys in the order `TextReader.read` documents."""
    return (['quad', 'text'] + (['raw_text', 'lexicon_distance'] if rule else []) + (['lexicon_score'] if rule == 'likelihood' else [])
            + (['text_score', 'alternatives'] if decode == 'beam' else []) + (['chars'] if chars else []) + (['score'] if scores else []))


def test_items_of_every_mode_are_what_the_ops_give_by_hand():
    from megreader_amd.data.quad_crop import plan_crop
    from megreader_amd.ops.decode import ctc_beam_search_decode, ctc_forced_align
    from megreader_amd.ops.lexicon import Lexicon
    charset = EnglishCharset()
    blank, unknown = charset.blank, charset.unknown
    words, delta, rec_size = ["AB12", "HELL0", "TEXTS"], 1, (32, 128)       # AB12 is there, HELLO and TEXT are one edit away, X9 far
    lexicon = Lexicon(words, charset)
    pictures = photos()
    shapes = [p.shape for p in pictures for _ in range(2)][:4]

    def string(row, k):
        return charset.label_to_string(row[:int(k)])

    # the same crops, the posterior and every op, once, by hand
    plain = TextReader(detector, SoftSpell(charset), charset, det_size=DET_SIZE).read(pictures)
    quads = [[item['quad'] for item in found] for found in plain]
    crops = QuadCropper(image_size=rec_size).crop(pictures, quads)
    assert crops['index'].cpu().tolist() == [0, 0, 1, 1]
    post = SoftSpell(charset)(crops['image'])
    T = post.shape[3]
    decoded = {}
    ids, lengths = ctc_greedy_decode(post, blank=blank, unknown=unknown)
    decoded['ctc'] = (ids, lengths, [string(r, k) for r, k in zip(ids.cpu().numpy(), lengths.cpu().numpy())], None)
    beam = ctc_beam_search_decode(post, beam=8, nbest=2, top_classes=16, blank=blank, unknown=unknown)
    b_ids, b_len, b_scores, b_count = (beam[k].cpu().numpy() for k in ('ids', 'lengths', 'scores', 'count'))
    extras = [{'text_score': float(s[0]) if n > 0 else float('-inf'),
               'alternatives': [(string(r[j], k[j]), float(s[j])) for j in range(int(n))]}
              for r, k, s, n in zip(b_ids, b_len, b_scores, b_count)]
    decoded['beam'] = (beam['ids'][:, 0], beam['lengths'][:, 0], [string(r[0], k[0]) for r, k in zip(b_ids, b_len)], extras)
    assert sorted(decoded['ctc'][2]) == sorted(LEVELS.values()) and decoded['beam'][2] == decoded['ctc'][2]
    assert all(len(e['alternatives']) == 2 and e['alternatives'][0][1] > e['alternatives'][1][1] > -math.inf for e in extras)

    def by_hand(decode, rule, chars):
        ids, lengths, raw, extras = decoded[decode]
        rows = ids.to(torch.int32).masked_fill(torch.arange(ids.shape[1], device=ids.device)[None, :] >= lengths[:, None], blank)
        final = [r[:int(k)].tolist() for r, k in zip(rows.cpu().numpy(), lengths.cpu().numpy())]
        items = [{'text': t} for t in raw]
        took = [False] * len(raw)
        if rule:
            found = lexicon.nearest(rows) if rule == 'nearest' else lexicon.transcribe(post, max_distance=delta)
            index, distance = found['index'].cpu().tolist(), found['distance'].cpu().tolist()
            took = [i >= 0 and (rule == 'likelihood' or d <= delta) for i, d in zip(index, distance)]
            for m, item in enumerate(items):
                item.update(raw_text=raw[m], lexicon_distance=distance[m])
                if took[m]:
                    item['text'] = words[index[m]]
                    final[m] = lexicon.sym[lexicon.off[index[m]]:lexicon.off[index[m] + 1]].tolist()
                if rule == 'likelihood':
                    item['lexicon_score'] = found['score'].cpu().tolist()[m]
        if extras is not None:
            for item, extra in zip(items, extras):
                item.update(extra)
        if chars:
            S = max(len(f) for f in final)
            targets = torch.tensor([f + [blank] * (S - len(f)) for f in final], dtype=torch.int32, device="cuda")
            lens = torch.tensor([len(f) for f in final], dtype=torch.int32, device="cuda")
            out = {k: v.cpu().numpy() for k, v in ctc_forced_align(post, targets, lens, blank=blank, unknown=unknown).items()}
            if lexicon.fold is not None:                        # a lexicon word is aligned to the folded posterior
                fold = torch.tensor(lexicon.fold, dtype=torch.int32, device="cuda")
                folded = ctc_forced_align(lexicon._folded(post.select(2, 0), fold, False), targets, lens, blank=blank, unknown=unknown)
                out = {k: np.where(np.asarray(took).reshape((-1,) + (1,) * (v.ndim - 1)), folded[k].cpu().numpy(), v)
                       for k, v in out.items()}
            for m, item in enumerate(items):
                assert math.isfinite(float(out['score'][m]))
                plan = plan_crop(shapes[m], np.asarray(plain_flat[m]['quad'], dtype=np.float64), rec_size, 'resize', 'min_area_rect')
                item['chars'] = []
                for k, ch in enumerate(item['text']):
                    b, e = int(out['begin'][m][k]), int(out['end'][m][k])
                    u0, u1 = (min(max(v * (rec_size[1] / float(T)), 0.0), float(plan.dst_w)) for v in (b, e))
                    quad = plan.canvas_to_photo([[u0, 0.0], [u1, 0.0], [u1, float(rec_size[0])], [u0, float(rec_size[0])]])
                    item['chars'].append({'char': ch, 'quad': quad.tolist(), 'score': math.exp(float(out['sym_lp'][m][k]) / (e - b))})
        return items

    plain_flat = [item for found in plain for item in found]
    seen = set()
    for decode, rule in (('ctc', None), ('ctc', 'nearest'), ('ctc', 'likelihood'), ('beam', None), ('beam', 'nearest')):
        for chars in (False, True):
            want = by_hand(decode, rule, chars)
            for scores in (False, True):
                recognizer = SoftSpell(charset)
                kw = dict(lexicon=lexicon, lexicon_rule=rule, lexicon_max_distance=delta) if rule else {}
                reader = TextReader(detector, recognizer, charset, det_size=DET_SIZE, rec_size=rec_size, decode=decode, nbest=2,
                                    max_crops=3, chars=chars, scores=scores, **kw)
                results = reader.read(pictures)
                assert recognizer.batches == [3, 1] and [len(found) for found in results] == [2, 2, 0]
                got = [item for found in results for item in found]
                for item, ref, base in zip(got, want, plain_flat):
                    mode = (decode, rule, chars, scores)
                    assert list(item) == item_keys(decode, rule, chars, scores), mode
                    assert item['quad'] == base['quad']
                    if scores:
                        assert isinstance(item.pop('score'), float)
                    quads_got = [ch.pop('quad') for ch in item.get('chars', [])]
                    quads_ref = [ch.pop('quad') for ch in [dict(c) for c in ref.get('chars', [])]]
                    assert len(quads_got) == len(quads_ref) and np.allclose(np.asarray(quads_got).reshape(-1, 4, 2),
                                                                            np.asarray(quads_ref).reshape(-1, 4, 2), atol=1e-9), mode
                    ref = dict(ref, quad=base['quad'])
                    if chars:
                        ref['chars'] = [{k: v for k, v in ch.items() if k != 'quad'} for ch in ref['chars']]
                    assert item == ref, (mode, item, ref)                   # strings, ints and floats (-inf included) bit for bit
                    seen.add((item['text'], item.get('raw_text'), item.get('lexicon_distance')))
    # the lexicon did all three things: confirmed a string, replaced one, and left one alone (nearest: too far; likelihood: nothing)
    assert {("AB12", "AB12", 0), ("HELL0", "HELLO", 1), ("TEXTS", "TEXT", 1), ("X9", "X9", -1)} <= seen
    assert any(t == "X9" and d is not None and d > delta for t, _, d in seen)
