"""Mirror of structure/measurers/sequence_recognition_measurer.py:11-112 (`measure` / `validate_measure` /
`gather_measure` contract) scoring the id sequences on the GPU (mr_seq_measure): accuracy = upper-cased strings equal,
edit_distance = 1 - min(len, levenshtein) / len (0 for an empty label).

With a lexicon (`nori_lexicon_path`, the reference's state, or `lexicon`) the reference's split is reported as well: `measure`
adds `in_lexicon` per sample and `gather_measure` returns total / in-lexicon / out-of-lexicon meters for each of accuracy and edit
distance (reference lines 28-49, 59-64, 74-100).  Membership is tested on the device from the label ids (mr_lexicon_nearest,
distance 0).  `correct=True` is ours, not the reference's: `lexicon_accuracy` per sample, the label equal to the lexicon word
nearest to the prediction -- the figure the papers call accuracy "with lexicon"."""
import numpy as np
import torch

from ..charsets import upper_fold_table
from ..ops.decode import sequence_measure


class AverageMeter(object):
    """concern/average_meter.py semantics (val / avg / sum / count).  An update with numpy operands and a count of zero leaves a
    `nan` average until a later update, as there (no exception)."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        return self


class SequenceRecognitionMeasurer(object):
    def __init__(self, charset=None, blank=0, unknown=1, cmd=None, nori_lexicon_path=None, lexicon=None, correct=False,
                 **kwargs):
        from . import member_from_config
        charset = member_from_config(charset, cmd)
        self.blank, self.unknown = blank, unknown
        self.fold = None
        fold = upper_fold_table(charset)          # `.upper()` of the strings: ids whose characters upper-case alike compare equal
        if fold is not None:
            self.fold = torch.tensor(fold, dtype=torch.int32)
        self.nori_lexicon_path = nori_lexicon_path
        self.correct = bool(correct)
        self.lexicon = None
        self.members = 0
        words = None
        if lexicon is not None:
            words = list(lexicon.words) if hasattr(lexicon, 'words') else list(lexicon)
        elif nori_lexicon_path:
            with open(nori_lexicon_path) as f:
                words = sorted(set(f.read().split()))
        if words:                                 # (an empty lexicon is no lexicon: the reference tests `if self.nori_lexicon`)
            from ..ops.lexicon import Lexicon
            # The reference tests `label_string.upper() in self.nori_lexicon` against the entries verbatim, so an entry that is not
            # its own .upper() can never be a member.  Members first: a label's candidates are the words [0, members), the
            # candidates of a correction all of them.
            member = [w for w in words if w == w.upper()]
            self.members = len(member)
            self.lexicon = Lexicon(member + [w for w in words if w != w.upper()], charset)
            self.lexicon.blank, self.lexicon.unknown = blank, unknown

    def _lexicon_measure(self, label, pred):
        """(in_lexicon, lexicon_accuracy or None) as lists of bool: one mr_lexicon_nearest call, one copy back."""
        N, L = label.shape[0], len(self.lexicon)
        S = max(label.shape[1], pred.shape[1]) if self.correct else label.shape[1]

        def rows(t):
            t = t.to(torch.int32)
            return t if t.shape[1] == S else torch.nn.functional.pad(t, (0, S - t.shape[1]), value=self.blank)
        parts, spans = [rows(label)], [(0, self.members)]
        if self.correct:
            if self.members != L:
                parts.append(rows(label))
                spans.append((0, L))
            parts.append(rows(pred))
            spans.append((0, L))
        span = torch.tensor([s for s in spans for _ in range(N)], dtype=torch.int32).reshape(-1, 2)
        found = self.lexicon.nearest(torch.cat(parts), span)
        host = torch.stack([found['index'], found['distance']]).cpu().numpy().reshape(2, len(parts), N)
        index, distance = host[0], host[1]
        in_lexicon = (distance[0] == 0).tolist()
        if not self.correct:
            return in_lexicon, None
        # the label IS the word nearest to the prediction: it is a word (distance 0 over all words) and the lowest index that
        # spells it is the lowest index nearest to the prediction (words that spell alike are equally far from anything)
        hit = (distance[-2] == 0) & (index[-2] == index[-1])
        return in_lexicon, hit.tolist()

    def measure(self, batch, output):
        pred = torch.stack([o['pred_ids'] for o in output])
        label = torch.stack([o['label_ids'] for o in output]).to(pred.device)
        m = sequence_measure(label, pred, self.blank, self.unknown, self.fold)
        result = dict(accuracy=m['accuracy'].cpu().tolist(), edit_distance=m['edit_distance'].cpu().tolist())
        if self.lexicon is not None:
            result['in_lexicon'], hit = self._lexicon_measure(label, pred)
            if hit is not None:
                result['lexicon_accuracy'] = hit
        return result

    def validate_measure(self, batch, output):
        return self.measure(batch, output), []

    evaluate_measure = validate_measure

    def gather_measure(self, raw_metrics, logger=None):
        def gather(key):
            meter = AverageMeter()
            for m in raw_metrics:
                v = m[key]
                meter.update(np.array(v).sum() / len(v), len(v))
            return meter
        if self.lexicon is None:
            return dict(accuracy=gather('accuracy'), edit_distance=gather('edit_distance'))

        def split(key):                           # reference lines 83-100
            meter, inside, outside = AverageMeter(), AverageMeter(), AverageMeter()
            with np.errstate(invalid='ignore', divide='ignore'):        # a meter whose count is still 0 averages to nan, quietly
                for m in raw_metrics:
                    raw, in_lexicon = np.array(m[key]), np.array(m['in_lexicon'])
                    total = len(raw)
                    meter.update(raw.sum() / total, total)
                    for part, sel in ((inside, raw[in_lexicon == True]), (outside, raw[in_lexicon == False])):  # noqa: E712
                        part.update(sel.sum() / max(len(sel), 1), len(sel))
            return meter, inside, outside
        total_ed, in_ed, out_ed = split('edit_distance')
        total_acc, in_acc, out_acc = split('accuracy')
        result = dict(total_edit_distance=total_ed, in_lexicon_edit_distance=in_ed, out_lexicon_edit_distance=out_ed,
                      total_accuracy=total_acc, in_lexicon_accuracy=in_acc, out_lexicon_accuracy=out_acc)
        if self.correct and all('lexicon_accuracy' in m for m in raw_metrics):
            result['lexicon_accuracy'] = gather('lexicon_accuracy')
        return result
