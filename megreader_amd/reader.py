"""Read text end to end: photos in, per photo a list of {'quad', 'text'} out (with `scores=True` also 'score', the detector's
confidence in the box; with `lexicon=` also 'raw_text' and 'lexicon_distance', and 'text' is the nearest lexicon word, or with
`lexicon_rule='likelihood'` the word with the greatest CTC probability, its log-probability in 'lexicon_score'; with
`decode='beam'` 'text' is the most probable string of the CTC posterior, its log-probability in 'text_score', and with
`nbest > 1` the other readings in 'alternatives'; with `chars=True` also 'chars': where every character of 'text' lies in the photo
and how sure the recogniser is of it, by forced alignment of the final string to the CTC posterior).

The reference has the pieces in separate programs -- the DB detector with `SegDetectorRepresenter`
(structure/representers/seg_detector_representer.py), `ImageCropper` (data/crop_file_dataset.py:85-124) and the recognisers --
and joins them through files of cropped images.  Here the photo is uploaded once and never leaves the device between the two
models:

    reader = TextReader(detector, recognizer, charset)
    for found in reader.read(photos):               # photos: uint8 HWC numpy arrays (cv2.imread(..., IMREAD_COLOR))
        for item in found:
            item['quad'], item['text']

  1. `DevicePipeline(det_size, 'resize')` stages and uploads the photos and makes the detector's input from them
     (`det_size` = the validate `Resize` of experiments/seg_detector/community-base.yaml: 1024 x 576);
  2. `detector(image)` in eval mode under no_grad, `representer.represent` with the photos' own shapes (boxes in photo pixels);
  3. `QuadCropper.crop` samples the recognition batch out of the photos still resident in the pipeline's device buffer;
  4. `recognizer` in chunks of `max_crops`, greedy decoding (or prefix beam search), `charset.label_to_string`.
Only the boxes (a few hundred points) and the decoded ids (with the beam: ids, lengths and scores; with `chars=True` the first and
last column and the summed log-probability of every character) cross to the host.

A recogniser whose eval output is the pair (classify [M, C, H, W], mask [M, 1, H, W]) with H > 1 is a 2D-CTC head
(decoders/ctc_decoder2d.py).  Its posterior is `ctc2d_marginal(classify, mask)`, computed once per chunk: the string probabilities
of the 2-D head are the 1-D CTC probabilities of that marginal, so the beam, the lexicon and the alignment read it unchanged.
`decode='ctc'` is `ctc2d_greedy_decode`, the rule `CTCRepresenter2D` scores.  With `chars=True` `ctc2d_char_rows` also gives every
character the band of heights it lies on, and its quad spans that band instead of the whole height of the crop (per chunk the
lowest and the highest height of every character cross to the host as well).

An attention recogniser (a backbone and an `AttentionDecoder`) has no posterior to read; `decode='attention'` goes through
`AttentionDecoder.read` instead: the probability of the string and of every character under the decoder, n-best strings by beam
search, and character boxes from the mean and spread of each step's attention map (per chunk the words' log-probabilities
and four moments per character cross to the host).

`det_scales` (None: step 1 and 2 as above, one `det_size` canvas per photo whatever its size) reads large photos at their own
scale: `det_size` becomes the size of a TILE, every photo is resized to one canvas per entry of `det_scales` ('fit': `det_size`
itself; a float s: the photo times s, rounded to multiples of `det_align`), the canvases are covered by tiles that overlap by
twice `det_halo`, the detector runs on the tiles in chunks of `det_batch`, and the tiles' maps of all levels are fused
(`det_fuse`: 'max' or 'mean') into ONE map per photo, on which the representer runs once with the photo's own shape
(data/detection_tiles.py: `DetectionTiler`; a word cut by a tile border comes back as one box).  The tiles are sampled from the
photos the pipeline uploaded, decoded ones with `encoded=True`; everything behind the boxes is as above.

`curved=True` reads words that follow a curve.  The representer's `represent_ribbons` returns beside every box the RIBBON its
component follows (structure/ribbon.py; `mr_db_ribbons` with `ribbon_slabs` slabs), or None where the word is short or straight
enough for its box, and every crop goes through `StripCropper` (data/strip_crop.py, one launch of mr_strip_crop) -- a box without
a ribbon as `Ribbon.from_box`, which is the quad crop's map.  Every item gains 'polygon', the ribbon's outline (top forward, bottom
backward) or the box's four corners; 'quad' stays the box; character quads go through `StripPlan.canvas_to_photo` and follow the
curve.  The representer scores a box by the mean of the map over the RECTANGLE, of which a curved word fills only a part: give the
representer a lower `box_thresh` than the 0.7 that suits straight words."""
import math

import numpy as np
import torch

from .data.detection_tiles import DetectionTiler
from .data.device_pipeline import DevicePipeline, EncodedDevicePipeline
from .data.jpeg_decode import SPLIT_ABOVE
from .data.quad_crop import DegenerateQuad, QuadCropper
from .data.strip_crop import StripCropper, plan_strip
from .ops.decode import (ctc2d_char_rows, ctc2d_greedy_decode, ctc2d_marginal, ctc_beam_search_decode, ctc_forced_align,
                         ctc_greedy_decode)
from .ops.lexicon import Lexicon
from ._lib import _DEFINES
from .structure.ribbon import Ribbon
from .structure.seg_detector_representer import SegDetectorRepresenter


class TextReader(object):
    def __init__(self, detector, recognizer, charset, representer=None, det_size=(576, 1024), rec_size=(32, 128),
                 rec_mode='resize', rectify='min_area_rect', decode='ctc', max_crops=256, scores=False, lexicon=None,
                 lexicon_max_distance=None, lexicon_rule='nearest', beam_width=None, nbest=1, beam_top_classes=16, chars=False,
                 column_geometry=None, row_geometry=None, attention_extent=1.5, encoded=False, lm=None, lm_weight=1.0,
                 lm_bonus=0.0, det_scales=None, det_halo=(64, 64), det_fuse='max', det_batch=8, det_align=32, curved=False,
                 ribbon_slabs=8):
        self.det_tiler = None
        if det_scales is not None:      # tiles of `det_size` at the photo's own scale, fused per photo (data/detection_tiles.py)
            if int(det_batch) < 1:
                raise ValueError("det_batch must be at least 1, got %r" % (det_batch,))
            self.det_tiler = DetectionTiler(tile=det_size, halo=det_halo, scales=det_scales, fuse=det_fuse, align=det_align)
        self.det_batch = int(det_batch)
        if lexicon_rule not in ('nearest', 'likelihood'):
            raise ValueError("lexicon_rule must be 'nearest' or 'likelihood', got %r" % (lexicon_rule,))
        if lexicon_rule == 'likelihood' and decode != 'ctc':
            raise ValueError("lexicon_rule='likelihood' scores CTC posteriors: it needs decode='ctc', got %r" % (decode,))
        if not (decode in ('ctc', 'ids', 'beam', 'attention') or callable(decode)):
            raise ValueError("decode must be 'ctc', 'beam', 'ids', 'attention' or a callable pred -> (ids, lengths), got %r"
                             % (decode,))
        if beam_width is None:                              # the CTC beam's default is 8 prefixes, the attention reader's greedy
            beam_width = 1 if decode == 'attention' else 8
        if decode == 'beam' and not (1 <= int(nbest) <= int(beam_width) <= 64 and 1 <= int(beam_top_classes) <= 64):
            raise ValueError("decode='beam' needs 1 <= nbest <= beam_width <= 64 and 1 <= beam_top_classes <= 64, got nbest=%r "
                             "beam_width=%r beam_top_classes=%r" % (nbest, beam_width, beam_top_classes))
        if lm is not None and decode != 'beam':
            raise ValueError("lm is fused into the CTC prefix beam search: it needs decode='beam', got %r" % (decode,))
        if int(max_crops) < 1:
            raise ValueError("max_crops must be at least 1, got %r" % (max_crops,))
        if decode == 'attention':
            if not 1 <= int(nbest) <= int(beam_width) <= 64:
                raise ValueError("decode='attention' needs 1 <= nbest <= beam_width <= 64, got nbest=%r beam_width=%r"
                                 % (nbest, beam_width))
            if not (callable(getattr(recognizer, 'read', None))
                    or (hasattr(recognizer, 'backbone') and callable(getattr(getattr(recognizer, 'decoder', None), 'read', None)))):
                raise ValueError("decode='attention' needs a recogniser with read(crops, beam=, nbest=), or with .backbone and "
                                 ".decoder (an AttentionDecoder), got %r" % (type(recognizer).__name__,))
            if not (math.isfinite(float(attention_extent)) and float(attention_extent) >= 0.0):
                raise ValueError("attention_extent must be a finite number of standard deviations >= 0, got %r"
                                 % (attention_extent,))
        if chars and decode not in ('ctc', 'beam', 'attention'):
            raise ValueError("chars=True aligns the text to a CTC posterior or reads an attention decoder's maps: it needs "
                             "decode='ctc', 'beam' or 'attention', got %r" % (decode,))
        if column_geometry is not None:
            stride, offset = (float(v) for v in column_geometry)
            if not (stride > 0.0 and math.isfinite(stride) and math.isfinite(offset)):
                raise ValueError("column_geometry must be (stride > 0, offset) in canvas pixels, got %r" % (column_geometry,))
            column_geometry = (stride, offset)
        if row_geometry is not None:
            stride, offset = (float(v) for v in row_geometry)
            if not (stride > 0.0 and math.isfinite(stride) and math.isfinite(offset)):
                raise ValueError("row_geometry must be (stride > 0, offset) in canvas pixels, got %r" % (row_geometry,))
            row_geometry = (stride, offset)
        self.detector = detector
        self.recognizer = recognizer
        self.charset = charset
        self.blank, self.unknown = getattr(charset, 'blank', 0), getattr(charset, 'unknown', 1)
        self.representer = representer if representer is not None else SegDetectorRepresenter(resize=True)
        self.decode = decode
        self.beam_width, self.nbest, self.beam_top_classes = int(beam_width), int(nbest), int(beam_top_classes)
        self.lm, self.lm_weight, self.lm_bonus = lm, float(lm_weight), float(lm_bonus)
        self.max_crops = int(max_crops)
        self.scores = bool(scores)
        self.chars = bool(chars)
        self.column_geometry = column_geometry
        self.row_geometry = row_geometry
        self.attention_extent = float(attention_extent)
        if lexicon is not None and not isinstance(lexicon, Lexicon):
            lexicon = Lexicon(lexicon, charset)
        self.lexicon = lexicon
        self.lexicon_max_distance = None if lexicon_max_distance is None else int(lexicon_max_distance)
        self.lexicon_rule = lexicon_rule
        self.encoded = bool(encoded)
        if self.encoded:    # `read` takes the photos as encoded files; the device decodes them (data/jpeg_decode.py), whole photos
            self.det_pipeline = EncodedDevicePipeline(image_size=det_size, mode='resize', charset=charset,    # by many lanes each
                                                      split_above=SPLIT_ABOVE)
        else:
            self.det_pipeline = DevicePipeline(image_size=det_size, mode='resize', charset=charset)
        self.cropper = QuadCropper(image_size=rec_size, mode=rec_mode, rectify=rectify)
        self.curved = bool(curved)
        self.ribbon_slabs = int(ribbon_slabs)
        if self.curved:         # every crop through mr_strip_crop: a ribbon where the representer found one, else the box's
            if not callable(getattr(self.representer, 'represent_ribbons', None)):
                raise ValueError("curved=True needs a representer with represent_ribbons(batch, pred, slabs=) -> (boxes, scores, "
                                 "ribbons), got %r" % (type(self.representer).__name__,))
            if rectify != 'min_area_rect':
                raise ValueError("curved=True crops boxes as `Ribbon.from_box` does: it needs rectify='min_area_rect', got %r"
                                 % (rectify,))
            if not 3 <= self.ribbon_slabs <= _DEFINES["MR_RIBBON_MAX_SLABS"]:
                raise ValueError("ribbon_slabs must be in [3, %d], got %r" % (_DEFINES["MR_RIBBON_MAX_SLABS"], ribbon_slabs))
            self.strip_cropper = StripCropper(image_size=rec_size, mode=rec_mode)

    def _upload(self, images):
        """The detector's input batch and the photos as uint8 HWC views of the device buffer the pipeline uploaded."""
        staged, layout = self.det_pipeline.pack(images, [''] * len(images))
        batch = self.det_pipeline.upload(staged, layout)
        return batch, self.det_pipeline.photos(batch, layout)

    def _detect_tiled(self, photos):
        """With `det_scales`: the detector on tiles of the resident photos at their own scale (`DetectionTiler.detect_maps`), every
        map the representer reads -- 'binary', and `representer.dest` when it differs -- fused per photo, and the representer
        once per photo on the fused map with the photo's own shape: (boxes per photo, scores per photo or None, with `curved`
        ribbons per photo or None)."""
        keys = ('binary',) + ((self.representer.dest,) if getattr(self.representer, 'dest', 'binary') != 'binary' else ())
        fused = self.det_tiler.detect_maps(self.detector, photos, batch=self.det_batch, keys=keys)
        boxes, box_scores = [], ([] if self.scores else None)
        ribbons = [] if self.curved else None
        for i, photo in enumerate(photos):
            det_batch = {'image': None, 'shape': [tuple(photo.shape[:2])]}
            pred = {key: fused[key][i] for key in keys}
            if self.curved:
                found, scored, curves = self.representer.represent_ribbons(det_batch, pred, slabs=self.ribbon_slabs)
                ribbons.extend(curves)
                if self.scores:
                    box_scores.extend(scored)
            elif self.scores:
                found, scored, _ = self.representer.represent_scored(det_batch, pred)
                box_scores.extend(scored)
            else:
                found, _ = self.representer.represent(det_batch, pred)
            boxes.extend(found)
        return boxes, box_scores, ribbons

    def _pack_strips(self, photos, boxes, ribbons):
        """With `curved`: every box as a strip -- its ribbon, or `Ribbon.from_box` of the box where there is none -- planned and
        staged by the `StripCropper`: (staged, layout, per crop its photo, its box and its outline).  A box with a zero side is
        dropped, as the `QuadCropper` drops it."""
        plans, index, quads, outlines, dropped = [], [], [], [], []
        for i, (found, curves) in enumerate(zip(boxes, ribbons)):
            for k, (box, ribbon) in enumerate(zip(found, curves)):
                outline = box
                try:
                    if ribbon is not None:
                        try:
                            plan, outline = plan_strip(photos[i].shape, ribbon, self.strip_cropper.image_size,
                                                       self.strip_cropper.mode), ribbon.polygon().tolist()
                        except DegenerateQuad:
                            ribbon = None
                    if ribbon is None:
                        plan = plan_strip(photos[i].shape, Ribbon.from_box(box), self.strip_cropper.image_size,
                                          self.strip_cropper.mode)
                except DegenerateQuad:
                    dropped.append((i, k))
                    continue
                plans.append((i, plan))
                index.append(i)
                quads.append([[float(x), float(y)] for x, y in box])
                outlines.append(outline)
        staged, layout = self.strip_cropper.pack(photos, None, plans=plans)
        return staged, layout._replace(dropped=dropped), index, quads, outlines

    @staticmethod
    def _head2d(pred):
        """(classify [M, C, H, W], mask [M, 1, H, W]) when `pred` is the eval output of a 2D-CTC head -- a pair whose first member
        has four dimensions and more than one height -- else None."""
        if isinstance(pred, (tuple, list)) and len(pred) == 2 and torch.is_tensor(pred[0]) and torch.is_tensor(pred[1]) \
                and pred[0].dim() == 4 and pred[0].shape[2] > 1:
            return pred[0], pred[1]
        return None

    def _decode(self, pred, post, head2d=None):
        """The decode step of one chunk (pred: the recogniser's output, post: its CTC posterior, head2d: `_head2d(pred)`): (ids
        [M, S] and lengths [M] or None, on the device; None or, with decode='beam', per crop the dict of the keys the beam adds
        to an item).  The greedy string of a 2-D head is `ctc2d_greedy_decode`'s, the rule `CTCRepresenter2D` scores."""
        if self.decode == 'beam':
            return self._beam(post)
        if callable(self.decode):
            return tuple(self.decode(pred)) + (None,)
        if self.decode == 'ids':
            return pred, None, None
        if head2d is not None:
            return ctc2d_greedy_decode(head2d[0], head2d[1], blank=self.blank, unknown=self.unknown) + (None,)
        return ctc_greedy_decode(post, blank=self.blank, unknown=self.unknown) + (None,)

    @staticmethod
    def _eval(module, x, call=None):
        """module(x) -- or call(x), which runs `module` -- under no_grad, in eval mode for the call (a module that was training is
        put back)."""
        was_training = bool(getattr(module, 'training', False))
        if was_training:
            module.eval()
        try:
            with torch.no_grad():
                return module(x) if call is None else call(x)
        finally:
            if was_training:
                module.train()

    def _beam(self, pred):
        """One chunk by prefix beam search: (top-1 ids [M, T] and lengths [M] on the device, per crop {'text_score'} and, with
        nbest > 1, {'alternatives'}).  The ids, lengths and scores of the hypotheses are all that crosses to the host."""
        out = ctc_beam_search_decode(pred, beam=self.beam_width, nbest=self.nbest, top_classes=self.beam_top_classes,
                                     blank=self.blank, unknown=self.unknown, lm=self.lm, lm_weight=self.lm_weight,
                                     lm_bonus=self.lm_bonus)
        return out['ids'][:, 0], out['lengths'][:, 0], self._hypotheses(out)

    def _align(self, pred, ids, lengths, found, head2d=None):
        """One chunk's FINAL strings aligned to its posterior (`ctc_forced_align`): (begin, end, sym_lp) as numpy [M, S], the
        number of columns T and None or, for a 2-D head, (row_lo, row_hi as numpy [M, S], the number of heights H).  The final
        ids are the decoded ones (greedy, or the beam's first hypothesis), or `Lexicon.ids` of the
        word where one was taken; a lexicon word is aligned to the posterior over the folded alphabet (`Lexicon._folded`), the
        rows that kept their raw string to the posterior as it is: two calls per chunk at most, each with length -1 (unalignable,
        no work) for the other call's rows.  Each alignment of a 2-D head (pred: its sum-marginal, head2d: classify and mask)
        goes on through `ctc2d_char_rows`, a lexicon word's over classify folded as the posterior was.  Only the arrays returned
        cross to the host."""
        if pred.dim() == 4:
            pred = pred.select(2, 0)
        dev = pred.device
        # (a string of more symbols than mr_ctc_align takes keeps its length and is unalignable)
        targets = ids[:, :_DEFINES["MR_CTC_ALIGN_MAX_SYMBOLS"]].to(device=dev, dtype=torch.int32)
        lens = lengths.to(device=dev, dtype=torch.int32)
        took = fold = None
        if found is not None:
            took = self._takes_word(found['index'], found['distance'])
            words, word_lens = self.lexicon.ids(torch.where(took, found['index'], torch.full_like(found['index'], -1)))
            S = max(targets.shape[1], words.shape[1])
            targets = torch.nn.functional.pad(targets, (0, S - targets.shape[1]), value=self.blank)
            words = torch.nn.functional.pad(words, (0, S - words.shape[1]), value=self.blank)
            targets = torch.where(took[:, None], words, targets)
            lens = torch.where(took, word_lens, lens)
            fold = self.lexicon._tensors(dev)[2]

        def align(post, heads, lens):
            out = ctc_forced_align(post, targets, lens, blank=self.blank, unknown=self.unknown)
            if heads is not None:
                out.update(ctc2d_char_rows(heads[0], heads[1], targets, lens, out, blank=self.blank))
            return out

        keys = ('begin', 'end', 'sym_lp') + (('row_lo', 'row_hi') if head2d is not None else ())
        if fold is None:                                        # one posterior for every row
            out = align(pred, head2d, lens)
        else:
            none = torch.full_like(lens, -1)
            raw = align(pred, head2d, torch.where(took, none, lens))
            heads = None if head2d is None else (self.lexicon._folded(head2d[0], fold, False), head2d[1].float())
            folded = align(self.lexicon._folded(pred, fold, False), heads, torch.where(took, lens, none))
            out = {k: torch.where(took[:, None], folded[k], raw[k]) for k in keys}
        begin, end, sym_lp = (out[k].cpu().numpy() for k in keys[:3])
        bands = None if head2d is None else (out['row_lo'].cpu().numpy(), out['row_hi'].cpu().numpy(), int(head2d[0].shape[2]))
        return begin, end, sym_lp, int(pred.shape[2]), bands

    def _spans(self, symbols, begin, end, sym_lp, T, bands=None):
        """What `read` makes one crop's 'chars' of: [(character, first column, one past the last, summed log-probability, lowest
        height, highest height)], T and H, or None when the string could not be aligned (the slots of its symbols are then
        empty).  `bands`: this crop's row_lo, row_hi and H for a 2-D head; None gives None for the heights and for H."""
        n = int((begin >= 0).sum())
        if n != len(symbols):
            return None
        lo, hi, H = bands if bands is not None else (None, None, None)
        return [(ch, int(begin[k]), int(end[k]), float(sym_lp[k])) + ((None, None) if H is None else (int(lo[k]), int(hi[k])))
                for k, ch in enumerate(symbols)], T, H

    def recognize(self, crops):
        """crops: f32 [M, 3, H, W] on the device -> M strings (with a lexicon: the nearest words, see `read`)."""
        return [rec['text'] for rec in self._recognize(crops)]

    def _takes_word(self, index, distance):
        """Whether the lexicon word `index` at edit distance `distance` replaces the raw string: the one statement of the rule, on
        device tensors (`_align`) and on the host's integers (`_to_host`) alike."""
        took = index >= 0
        if self.lexicon_rule == 'nearest' and self.lexicon_max_distance is not None:
            took = took & (distance <= self.lexicon_max_distance)
        return took

    def _lexicon(self, pred, ids, lengths):
        """The lexicon step of one chunk, on the device: None, or what `Lexicon.transcribe` finds in the posterior (likelihood
        rule) or `Lexicon.nearest` for the decoded ids, before they are copied."""
        if self.lexicon is None:
            return None
        if self.lexicon_rule == 'likelihood':
            return self.lexicon.transcribe(pred, max_distance=self.lexicon_max_distance)
        rows = ids.to(torch.int32)
        if lengths is not None:
            beyond = torch.arange(rows.shape[1], device=rows.device)[None, :] >= lengths.to(rows.device)[:, None]
            rows = rows.masked_fill(beyond, self.blank)
        return self.lexicon.nearest(rows)

    def _to_host(self, ids, lengths, extras, found, aligned):
        """One chunk's records (`_recognize`): copies the ids, lengths and what the lexicon found; `aligned` is on the host."""
        ids = ids.cpu().numpy()
        lengths = np.full(len(ids), ids.shape[1]) if lengths is None else lengths.cpu().numpy()
        records = [{'text': self.charset.label_to_string(row[:int(k)]), 'word': False} for row, k in zip(ids, lengths)]
        for rec, extra in zip(records, extras or ()):
            rec['extras'] = extra
        if found is not None:
            index, distance = torch.stack([found['index'], found['distance']]).cpu().tolist()
            for rec, i, d in zip(records, index, distance):
                rec.update(raw_text=rec['text'], lexicon_distance=d, word=bool(self._takes_word(i, d)))
                if rec['word']:
                    rec['text'] = self.lexicon.words[i]
            if self.lexicon_rule == 'likelihood':
                for rec, score in zip(records, found['score'].cpu().tolist()):
                    rec['lexicon_score'] = score
        if aligned is not None:
            begin, end, sym_lp, T, bands = aligned
            for m, (rec, row, k) in enumerate(zip(records, ids, lengths)):
                own = [self.charset.label_to_string(row[j:j + 1]) for j in range(int(k))]      # the raw string: its own ids
                rec['spans'] = self._spans(list(rec['text']) if rec['word'] else own, begin[m], end[m], sym_lp[m], T,
                                           None if bands is None else (bands[0][m], bands[1][m], bands[2]))
        return records

    def _recognize(self, crops):
        """One record (a dict) per crop, of the fields its mode produces and no others:
          'text', 'word'      the final string, and whether it is a lexicon word that was taken for the decoded one;
          'raw_text', 'lexicon_distance'   with a lexicon: the decoded string, and the distance of the word found (taken or not);
          'lexicon_score'     with the likelihood rule: log p(word | posterior);
          'extras'            with decode='beam': the dict of the keys the beam adds to an item;
          'spans'             with chars=True: what `_spans` returns for the final text (None: it could not be aligned);
          'marks'             with decode='attention' and chars=True: per character of the decoded string (character, sym_lp, cx,
                              cy, sx, sy), and the decoder's grid (height, max_size).
        Per chunk of `max_crops`: (the marginal of a 2-D head,) decode, lexicon and align on the device, then one step that copies
        to the host."""
        records = []
        if self.decode == 'attention':
            for lo in range(0, crops.shape[0], self.max_crops):
                records.extend(self._read_attention(crops[lo:lo + self.max_crops]))
            return records
        for lo in range(0, crops.shape[0], self.max_crops):
            pred = self._eval(self.recognizer, crops[lo:lo + self.max_crops])
            head2d = self._head2d(pred)
            if head2d is not None:                                          # (of a 2D-CTC recogniser: once per chunk)
                post = ctc2d_marginal(head2d[0], head2d[1])
            else:
                post = pred[0] if isinstance(pred, (tuple, list)) else pred     # (of a CTC recogniser)
            ids, lengths, extras = self._decode(pred, post, head2d)
            found = self._lexicon(post, ids, lengths)
            aligned = self._align(post, ids, lengths, found, head2d) if self.chars else None
            records.extend(self._to_host(ids, lengths, extras, found, aligned))
        return records

    def _hypotheses(self, out):
        """What a beam's n-best adds to the items of one chunk (out: ids, lengths, scores and count on the device): per crop
        {'text_score'} and, with nbest > 1, {'alternatives'}.  The ids, lengths and scores are all that crosses to the host."""
        scores, count = out['scores'].cpu().tolist(), out['count'].cpu().tolist()
        extras = [{'text_score': float(row[0]) if k > 0 else float('-inf')} for row, k in zip(scores, count)]
        parts = [out[key].cpu().tolist() for key in ('lm_scores', 'ctc_scores') if key in out]       # with a language model
        if parts:
            for m, extra in enumerate(extras):
                extra['lm_score'], extra['ctc_score'] = (float(part[m][0]) for part in parts)    # (-inf past count: a dead beam)
        if self.nbest > 1:
            ids, lengths = out['ids'].cpu().numpy(), out['lengths'].cpu().numpy()
            for m, (extra, rows, lens, row_scores, k) in enumerate(zip(extras, ids, lengths, scores, count)):
                extra['alternatives'] = [(self.charset.label_to_string(rows[j][:int(lens[j])]), float(row_scores[j]))
                                         + tuple(float(part[m][j]) for part in parts) for j in range(k)]
        return extras

    def _read_attention(self, crops):
        """One chunk's records with decode='attention': the recogniser's `read` (or its decoder's, behind the backbone), the
        nearest lexicon word of the decoded string, and with chars=True the 'marks' of the decoded string -- per chunk sym_lp
        and moments up to the chunk's longest string cross to the host besides the ids, lengths and scores.  A step that
        emitted `unknown` spells nothing in 'text' (`label_to_string` drops it) and gets no mark either."""
        rec = self.recognizer
        kw = dict(beam=self.beam_width, nbest=self.nbest)
        if callable(getattr(rec, 'read', None)):
            decoder, out = rec, self._eval(rec, crops, lambda x: rec.read(x, **kw))
        else:
            decoder, out = rec.decoder, self._eval(rec, crops, lambda x: rec.decoder.read(rec.backbone(x), **kw))
        ids, lengths = out['ids'][:, 0], out['lengths'][:, 0]
        found = self._lexicon(None, ids, lengths)
        ids, lengths = ids.cpu(), lengths.cpu()                               # (the one copy: `_to_host` and the marks read it)
        records = self._to_host(ids, lengths, self._hypotheses(out), found, None)
        if self.chars:
            grid = (int(decoder.height), int(decoder.max_size))
            rows, lens = ids.numpy(), lengths.numpy()
            longest = int(lens.max()) if len(lens) else 0
            sym_lp, moments = out['sym_lp'][:, :longest].cpu().numpy(), out['moments'][:, :longest].cpu().numpy()
            for m, rec_ in enumerate(records):
                spelt = [(self.charset.label_to_string(rows[m][j:j + 1]), float(sym_lp[m][j]))
                         + tuple(float(x) for x in moments[m][j]) for j in range(int(lens[m]))]
                rec_['marks'] = ([mark for mark in spelt if mark[0]], grid)
        return records

    def _attention_chars(self, plan, marks):
        """One item's 'chars' from its crop's plan and the decoder's marks: the rectangle around the mean of each character's
        attention map (`read`), on the canvas, clamped to it, carried to the photo."""
        marks, (height, width) = marks
        H, W = plan.canvas
        cell_w, cell_h = float(W) / width, float(H) / height
        chars = []
        for ch, lp, cx, cy, sx, sy in marks:
            hx, hy = max(self.attention_extent * sx, 0.5), max(self.attention_extent * sy, 0.5)
            u0 = min(max((cx - hx) * cell_w, 0.0), float(plan.dst_w))
            u1 = min(max((cx + hx) * cell_w, 0.0), float(plan.dst_w))
            v0 = min(max((cy - hy) * cell_h, 0.0), float(H))
            v1 = min(max((cy + hy) * cell_h, 0.0), float(H))
            quad = plan.canvas_to_photo([[u0, v0], [u1, v0], [u1, v1], [u0, v1]])
            chars.append({'char': ch, 'quad': quad.tolist(), 'score': math.exp(lp)})
        return chars

    def _chars(self, plan, spans):
        """One item's 'chars' from its crop's plan and aligned spans: the canvas rectangle of each character's columns (of a 2-D
        head: and of its band of heights), clamped to the valid canvas, carried to the photo by `CropPlan.canvas_to_photo`."""
        if spans is None:
            return None
        spans, T, rows = spans
        H, W = plan.canvas
        stride, offset = self.column_geometry if self.column_geometry is not None else (float(W) / T, 0.0)
        if rows is not None:                                                   # a 2-D head: the band of heights too
            row_stride, row_offset = self.row_geometry if self.row_geometry is not None else (float(H) / rows, 0.0)
        chars = []
        for ch, begin, end, lp, lo, hi in spans:
            u0 = min(max(offset + begin * stride, 0.0), float(plan.dst_w))
            u1 = min(max(offset + end * stride, 0.0), float(plan.dst_w))
            v0, v1 = 0.0, float(H)
            if rows is not None:
                v0 = min(max(row_offset + lo * row_stride, 0.0), float(H))
                v1 = min(max(row_offset + (hi + 1) * row_stride, 0.0), float(H))
            quad = plan.canvas_to_photo([[u0, v0], [u1, v0], [u1, v1], [u0, v1]])
            chars.append({'char': ch, 'quad': quad.tolist(), 'score': math.exp(lp / (end - begin))})
        return chars

    def read(self, images):
        """images: a list of uint8 HWC numpy arrays -- with `encoded=True` a list of `bytes`, the encoded files (JPEG decoded on the
        device, what it does not decode on the host; a file whose header is corrupt raises ValueError).  Returns, per image, a list of {'quad': [[x, y] * 4], 'text': str} in the
        representer's box order; [] for an image without boxes.  With `scores=True` every item also has 'score': the mean of the
        detector's probability map inside the box (`SegDetectorRepresenter.represent_scored`).  With a lexicon (a `Lexicon` or a
        list of words, encoded with the reader's charset) 'text' is the lexicon word nearest to the greedy string when its edit
        distance is at most `lexicon_max_distance` (None: always), and every item also has 'raw_text', the greedy string, and
        'lexicon_distance' (-1 for an empty lexicon).  With `lexicon_rule='likelihood'` (CTC recognisers, `decode='ctc'`) 'text' is
        instead the word with the greatest CTC probability under the recogniser's posterior among the words within
        `lexicon_max_distance` edits of the greedy string (None: the whole lexicon), 'lexicon_distance' that word's distance, and
        every item also has 'lexicon_score', log p(word | posterior); where no word is possible the greedy string is kept with
        -1 and -inf.  With `decode='beam'` (CTC recognisers) the string is the most probable one found by prefix beam search with
        `beam_width` hypotheses over the `beam_top_classes` best symbols of each column instead of the greedy one -- as 'text', or
        with a lexicon and the `nearest` rule as 'raw_text' and as what the nearest word is searched for -- and every item also
        has 'text_score', a float: its log-probability under the posterior (a lower bound: pruned alignments are missing); with
        `nbest > 1` also 'alternatives', the list of (text, score) of all hypotheses returned, the first one included, in
        descending order.  A crop whose beam died (no string has a non-zero probability) gets '', -inf and [].  With `lm`, a
        `CharNgramLM` over the reader's charset (`decode='beam'` only), the beam ranks its strings by log p_ctc + lm_weight *
        log p_lm + lm_bonus * (symbols) (`ctc_beam_search_decode(lm=...)`): 'text_score' is that fused value, every item also
        has 'lm_score' and 'ctc_score', its two parts (the latter the log-probability under the posterior), and the
        'alternatives' are (text, score, lm_score, ctc_score).  With `chars=True`
        (`decode='ctc'` or `'beam'`) every item also has 'chars', one {'char', 'quad', 'score'} per character of 'text': the final
        string -- the greedy ids, the beam's first hypothesis, or the lexicon word where one was taken -- is aligned to the crop's
        posterior by `ctc_forced_align` (a lexicon word to the posterior over the folded alphabet), 'score' is the geometric mean
        probability of the character over the columns of its span, exp(sym_lp / (end - begin)), and 'quad' the photo quadrilateral
        [[x, y] * 4] (TL, TR, BR, BL of the canvas rectangle) of the canvas columns U in [offset + begin * stride, offset + end *
        stride], clamped to the valid canvas, over the whole height, carried to the photo by `CropPlan.canvas_to_photo` -- a
        vertical crop gives boxes stacked along the photo's vertical axis.  `column_geometry` is (stride, offset) in canvas pixels;
        None means (W / T, 0): the posterior's columns partition the canvas evenly.  A model whose columns are not spread evenly
        (the CRNN's 33 columns over 128 pixels) should pass its own.  A text that cannot be aligned (a lexicon word of more
        symbols than columns, or one reachable only through zero probabilities) gets 'chars': None.  A 2D-CTC recogniser (eval
        output (classify [M, C, H, W], mask [M, 1, H, W]), H > 1) is read through `ctc2d_marginal(classify, mask)`, the 1-D
        posterior with the 2-D head's string probabilities: every mode above works on it as on a 1-D head's, `decode='ctc'` being
        `ctc2d_greedy_decode`.  With `chars=True` a character's quad is then the canvas rectangle of its columns and of the rows
        V in [row_offset + row_lo * row_stride, row_offset + (row_hi + 1) * row_stride], clamped to the canvas, row_lo and row_hi
        the lowest and highest of the most probable heights of its columns (`ctc2d_char_rows`; a lexicon word's over the folded
        alphabet); `row_geometry` is (row_stride, row_offset) in canvas pixels, None means (H_canvas / H, 0).  'score' stays
        exp(sym_lp / (end - begin)) on the marginal.
        With `decode='attention'` the recogniser is an attention decoder: a module with `read(crops, beam=, nbest=)`, or one with
        `.backbone` and `.decoder` (an `AttentionDecoder`), read through `AttentionDecoder.read` with `beam_width` (None: 1,
        greedy) hypotheses.  'text' is the first hypothesis up to its first blank and every item also has 'text_score', the
        log-probability of that string with its terminating blank under the decoder (no length normalisation); with `nbest > 1`
        also 'alternatives' as above.  With a lexicon (the `nearest` rule only) the nearest word is searched for the decoded
        string as for `decode='beam'`.  With `chars=True` every item also has 'chars', one {'char', 'quad', 'score'} per
        character of the DECODED string -- with a lexicon the boxes stay those of 'raw_text', also where a word was taken: the
        decoder has attended to what it read, not to the word; a step that emitted `unknown` spells nothing and has no entry -- where 'score' is the probability of the character at its step,
        exp(sym_lp), and 'quad' comes from the step's attention map over the decoder's height x max_size feature grid: with
        (cx, cy) its mean and (sx, sy) its standard deviation in cells, the rectangle cx +- max(attention_extent * sx, 0.5) by
        cy +- max(attention_extent * sy, 0.5) cells, scaled by W_canvas / max_size and H_canvas / height, clamped to the valid
        canvas and carried to the photo by `CropPlan.canvas_to_photo`.  An attention map says where the decoder looked, which is
        not a segmentation: `attention_extent` (1.5 standard deviations) is a choice, and half a cell the least box.
        With `curved=True` every item also has 'polygon' ([[x, y], ...]: the outline of the word's ribbon, or the four corners of
        'quad' where the box stands) and the crops, and with them every character quad, follow the ribbon (module docstring)."""
        images = list(images)
        results = [[] for _ in images]
        if not images:
            return results
        batch, photos = self._upload(images)
        ribbons = None
        if self.det_tiler is not None:          # (the pipeline's one-canvas batch is not looked at: the tiles read the photos)
            boxes, box_scores, ribbons = self._detect_tiled(photos)
        else:
            pred = self._eval(self.detector, batch['image'])
            if not isinstance(pred, dict):
                pred = {'binary': pred}
            det_batch = {'image': batch['image'], 'shape': [tuple(p.shape[:2]) for p in photos]}
            if self.curved:
                boxes, box_scores, ribbons = self.representer.represent_ribbons(det_batch, pred, slabs=self.ribbon_slabs)
            elif self.scores:
                boxes, box_scores, _ = self.representer.represent_scored(det_batch, pred)
            else:
                boxes, _ = self.representer.represent(det_batch, pred)
        outlines = None
        if self.curved:
            staged, layout, index, quads, outlines = self._pack_strips(photos, boxes, ribbons)
        else:
            staged, layout = self.cropper.pack(photos, boxes)
        if layout.M == 0:
            return results
        crops = (self.strip_cropper if self.curved else self.cropper).upload(staged, layout)
        records = self._recognize(crops['image'])
        if not self.curved:
            host = staged.numpy()
            index = host[layout.index_off:layout.index_off + 4 * layout.M].view(np.int32).tolist()
            quads = host[layout.quad_off:layout.quad_off + 64 * layout.M].view(np.float64).reshape(layout.M, 4, 2).tolist()
        # (boxes with a zero side were dropped by the cropper)
        for m, (i, quad, plan, rec) in enumerate(zip(index, quads, layout.plans, records)):
            item = {'quad': quad, 'text': rec['text']}
            if outlines is not None:
                item['polygon'] = outlines[m]
            item.update((key, rec[key]) for key in ('raw_text', 'lexicon_distance', 'lexicon_score') if key in rec)
            item.update(rec.get('extras', ()))
            if 'spans' in rec:
                item['chars'] = self._chars(plan, rec['spans'])
            if 'marks' in rec:
                item['chars'] = self._attention_chars(plan, rec['marks'])
            results[i].append(item)
        if self.scores:                                                        # ... and so are their scores
            dropped = set(layout.dropped)
            for i, found in enumerate(results):
                kept = [s for k, s in enumerate(box_scores[i]) if (i, k) not in dropped]
                for item, s in zip(found, kept):
                    item['score'] = s
        return results
