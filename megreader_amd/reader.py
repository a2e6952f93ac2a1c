"""Read text end to end: photos in, per photo a list of {'quad', 'text'} out (with `scores=True` also 'score', the detector's
confidence in the box; with `lexicon=` also 'raw_text' and 'lexicon_distance', and 'text' is the nearest lexicon word, or with
`lexicon_rule='likelihood'` the word with the greatest CTC probability, its log-probability in 'lexicon_score'; with
`decode='beam'` 'text' is the most probable string of the CTC posterior, its log-probability in 'text_score', and with
`nbest > 1` the other readings in 'alternatives').

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
Only the boxes (a few hundred points) and the decoded ids (with the beam: ids, lengths and scores) cross to the host."""
import numpy as np
import torch

from .data.device_pipeline import DevicePipeline
from .data.quad_crop import QuadCropper
from .ops.decode import ctc_beam_search_decode, ctc_greedy_decode
from .ops.lexicon import Lexicon
from .structure.seg_detector_representer import SegDetectorRepresenter


class TextReader(object):
    def __init__(self, detector, recognizer, charset, representer=None, det_size=(576, 1024), rec_size=(32, 128),
                 rec_mode='resize', rectify='min_area_rect', decode='ctc', max_crops=256, scores=False, lexicon=None,
                 lexicon_max_distance=None, lexicon_rule='nearest', beam_width=8, nbest=1, beam_top_classes=16):
        if lexicon_rule not in ('nearest', 'likelihood'):
            raise ValueError("lexicon_rule must be 'nearest' or 'likelihood', got %r" % (lexicon_rule,))
        if lexicon_rule == 'likelihood' and decode != 'ctc':
            raise ValueError("lexicon_rule='likelihood' scores CTC posteriors: it needs decode='ctc', got %r" % (decode,))
        if not (decode in ('ctc', 'ids', 'beam') or callable(decode)):
            raise ValueError("decode must be 'ctc', 'beam', 'ids' or a callable pred -> (ids, lengths), got %r" % (decode,))
        if decode == 'beam' and not (1 <= int(nbest) <= int(beam_width) <= 64 and 1 <= int(beam_top_classes) <= 64):
            raise ValueError("decode='beam' needs 1 <= nbest <= beam_width <= 64 and 1 <= beam_top_classes <= 64, got nbest=%r "
                             "beam_width=%r beam_top_classes=%r" % (nbest, beam_width, beam_top_classes))
        if int(max_crops) < 1:
            raise ValueError("max_crops must be at least 1, got %r" % (max_crops,))
        self.detector = detector
        self.recognizer = recognizer
        self.charset = charset
        self.representer = representer if representer is not None else SegDetectorRepresenter(resize=True)
        self.decode = decode
        self.beam_width, self.nbest, self.beam_top_classes = int(beam_width), int(nbest), int(beam_top_classes)
        self.max_crops = int(max_crops)
        self.scores = bool(scores)
        if lexicon is not None and not isinstance(lexicon, Lexicon):
            lexicon = Lexicon(lexicon, charset)
        self.lexicon = lexicon
        self.lexicon_max_distance = None if lexicon_max_distance is None else int(lexicon_max_distance)
        self.lexicon_rule = lexicon_rule
        self.det_pipeline = DevicePipeline(image_size=det_size, mode='resize', charset=charset)
        self.cropper = QuadCropper(image_size=rec_size, mode=rec_mode, rectify=rectify)

    def _upload(self, images):
        """The detector's input batch and the photos as uint8 HWC views of the device buffer the pipeline uploaded."""
        staged, layout = self.det_pipeline.pack(images, [''] * len(images))
        batch = self.det_pipeline.upload(staged, layout)
        return batch, self.det_pipeline.photos(batch, layout)

    def _ids(self, pred):
        """(ids [M, S], lengths [M] or None) of one chunk's prediction."""
        if callable(self.decode):
            return self.decode(pred)
        if self.decode == 'ids':
            return pred, None
        if isinstance(pred, (tuple, list)):
            pred = pred[0]
        return ctc_greedy_decode(pred, blank=getattr(self.charset, 'blank', 0), unknown=getattr(self.charset, 'unknown', 1))

    @staticmethod
    def _eval(module, x):
        """module(x) under no_grad, in eval mode for the call (a module that was training is put back)."""
        was_training = bool(getattr(module, 'training', False))
        if was_training:
            module.eval()
        try:
            with torch.no_grad():
                return module(x)
        finally:
            if was_training:
                module.train()

    def _beam(self, pred):
        """One chunk by prefix beam search: (top-1 ids [M, T] and lengths [M] on the device, per crop {'text_score'} and, with
        nbest > 1, {'alternatives'}).  The ids, lengths and scores of the hypotheses are all that crosses to the host."""
        if isinstance(pred, (tuple, list)):
            pred = pred[0]
        out = ctc_beam_search_decode(pred, beam=self.beam_width, nbest=self.nbest, top_classes=self.beam_top_classes,
                                     blank=getattr(self.charset, 'blank', 0), unknown=getattr(self.charset, 'unknown', 1))
        scores, count = out['scores'].cpu().tolist(), out['count'].cpu().tolist()
        extras = [{'text_score': float(row[0]) if k > 0 else float('-inf')} for row, k in zip(scores, count)]
        if self.nbest > 1:
            ids, lengths = out['ids'].cpu().numpy(), out['lengths'].cpu().numpy()
            for extra, rows, lens, row_scores, k in zip(extras, ids, lengths, scores, count):
                extra['alternatives'] = [(self.charset.label_to_string(rows[j][:int(lens[j])]), float(row_scores[j]))
                                         for j in range(k)]
        return out['ids'][:, 0], out['lengths'][:, 0], extras

    def recognize(self, crops):
        """crops: f32 [M, 3, H, W] on the device -> M strings (with a lexicon: the nearest words, see `read`)."""
        texts = self._recognize(crops)[0]
        return texts if self.lexicon is None else [t[0] for t in texts]

    def _recognize(self, crops):
        """(texts, extras).  texts: M strings; with a lexicon M (text, raw text, distance) triples, the text the nearest lexicon
        word where its distance is within `lexicon_max_distance`; with the likelihood rule (text, raw text, distance, score), the
        text the most probable word among those within `lexicon_max_distance` of the greedy string.  extras: None, or with
        decode='beam' M dicts of the keys the beam adds to an item."""
        texts = []
        extras = [] if self.decode == 'beam' else None
        likelihood = self.lexicon is not None and self.lexicon_rule == 'likelihood'
        for lo in range(0, crops.shape[0], self.max_crops):
            pred = self._eval(self.recognizer, crops[lo:lo + self.max_crops])
            if extras is None:
                ids, lengths = self._ids(pred)
            else:
                ids, lengths, more = self._beam(pred)
                extras.extend(more)
            found = None
            if likelihood:                                      # on the device posterior
                found = self.lexicon.transcribe(pred[0] if isinstance(pred, (tuple, list)) else pred,
                                                max_distance=self.lexicon_max_distance)
            elif self.lexicon is not None:                      # on the device ids, before they are copied
                rows = ids.to(torch.int32)
                if lengths is not None:
                    beyond = torch.arange(rows.shape[1], device=rows.device)[None, :] >= lengths.to(rows.device)[:, None]
                    rows = rows.masked_fill(beyond, getattr(self.charset, 'blank', 0))
                found = self.lexicon.nearest(rows)
            ids = ids.cpu().numpy()
            lengths = np.full(len(ids), ids.shape[1]) if lengths is None else lengths.cpu().numpy()
            raw = [self.charset.label_to_string(row[:int(k)]) for row, k in zip(ids, lengths)]
            if found is None:
                texts.extend(raw)
                continue
            if likelihood:
                index, distance = torch.stack([found['index'], found['distance']]).cpu().tolist()
                for text, i, d, score in zip(raw, index, distance, found['score'].cpu().tolist()):
                    texts.append((self.lexicon.words[i] if i >= 0 else text, text, d, score))
                continue
            index, distance = torch.stack([found['index'], found['distance']]).cpu().tolist()
            for text, i, d in zip(raw, index, distance):
                near = i >= 0 and (self.lexicon_max_distance is None or d <= self.lexicon_max_distance)
                texts.append((self.lexicon.words[i] if near else text, text, d))
        return texts, extras

    def read(self, images):
        """images: a list of uint8 HWC numpy arrays.  Returns, per image, a list of {'quad': [[x, y] * 4], 'text': str} in the
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
        descending order.  A crop whose beam died (no string has a non-zero probability) gets '', -inf and []."""
        images = list(images)
        results = [[] for _ in images]
        if not images:
            return results
        batch, photos = self._upload(images)
        pred = self._eval(self.detector, batch['image'])
        if not isinstance(pred, dict):
            pred = {'binary': pred}
        det_batch = {'image': batch['image'], 'shape': [im.shape[:2] for im in images]}
        if self.scores:
            boxes, box_scores, _ = self.representer.represent_scored(det_batch, pred)
        else:
            boxes, _ = self.representer.represent(det_batch, pred)
        staged, layout = self.cropper.pack(photos, boxes)
        if layout.M == 0:
            return results
        crops = self.cropper.upload(staged, layout)
        texts, extras = self._recognize(crops['image'])
        host = staged.numpy()
        index = host[layout.index_off:layout.index_off + 4 * layout.M].view(np.int32)
        quads = host[layout.quad_off:layout.quad_off + 64 * layout.M].view(np.float64).reshape(layout.M, 4, 2)
        # (boxes with a zero side were dropped by the cropper)
        for m, (i, quad, text) in enumerate(zip(index.tolist(), quads.tolist(), texts)):
            if self.lexicon is None:
                results[i].append({'quad': quad, 'text': text})
            else:
                results[i].append({'quad': quad, 'text': text[0], 'raw_text': text[1], 'lexicon_distance': text[2]})
                if len(text) > 3:
                    results[i][-1]['lexicon_score'] = text[3]
            if extras is not None:
                results[i][-1].update(extras[m])
        if self.scores:                                                        # ... and so are their scores
            dropped = set(layout.dropped)
            for i, found in enumerate(results):
                kept = [s for k, s in enumerate(box_scores[i]) if (i, k) not in dropped]
                for item, s in zip(found, kept):
                    item['score'] = s
        return results
