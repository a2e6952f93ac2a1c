"""A character n-gram language model for the CTC prefix beam search (mr_ctc_beam_search_lm, include/megreader_hip.h): what lets
a reader without a closed lexicon prefer "the" over "tbe".

    lm = CharNgramLM.train(words, charset, order=3)          # or CharNgramLM.from_arpa(text_or_path, charset)
    lm.log_prob(ids)                                          # float64, on the host
    ctc_beam_search_decode(pred, lm=lm, lm_weight=0.8)        # fused on the device (ops/decode.py)

The model is ARPA's backoff model over the class ids of a charset, natural logs in float64:
    g(c | ctx) = lp(ctx, c)                       if the n-gram ctx + c is listed,
                 bow(ctx) + g(c | ctx[1:])        otherwise (bow of a context that is not listed: 0),
and the empty context lists every eligible class (neither blank nor `unknown`): one the source lacks takes the `<unk>` value if
the source has one, else the smallest listed unigram value (that of `<s>` aside).  `<s>` and `</s>` frame a string: scoring starts
in the context `<s>` when the model lists it, and with end=True the string pays g(</s> | its last context).

On the device the model is a finite automaton (the header's "Model"): one state per listed context shorter than the order, the
n-grams as arcs in an open-addressing table keyed by (state, symbol), per state the backoff weight, the backoff state and
g(</s> | state).  `image(C)` builds it with numpy, needs no GPU and checks every invariant the kernel relies on."""
import math
import os

import numpy as np
import torch

from .._lib import _DEFINES
from ..charsets import DefaultCharset

ORDER_MAX = _DEFINES["MR_NGRAM_ORDER_MAX"]
BOS, EOS = -1, -2              # <s> and </s> as tokens of an n-gram; a class id is its own token
_LN10 = math.log(10.0)
_SPECIAL = {"<s>": BOS, "</s>": EOS}


def arc_hash(state, sym, slots):
    """The first slot of the probe sequence of (state, sym): the header's rule, in 32-bit unsigned arithmetic."""
    h = ((state * 0x9E3779B1) & 0xffffffff) ^ (((sym + 1) * 0x85EBCA6B) & 0xffffffff)
    return (h ^ (h >> 15)) % slots


class CharNgramLM(object):
    def __init__(self, ngrams, charset=None, order=None, unk=None, skipped=0):
        """ngrams: {tuple of tokens: (lp, bow)}, natural logs, bow 0.0 where the source gives none; tokens are class ids, BOS and
        EOS.  unk: the source's `<unk>` value or None.  Use `from_arpa` or `train`."""
        self.charset = charset if charset is not None else DefaultCharset()
        self.blank = getattr(self.charset, 'blank', 0)
        self.unknown = getattr(self.charset, 'unknown', 1)
        self.classes = len(self.charset)
        self.skipped = int(skipped)
        self.ngrams = {tuple(k): (float(v[0]), float(v[1])) for k, v in ngrams.items()}
        self.order = int(order) if order is not None else max([len(k) for k in self.ngrams] + [1])
        if not 1 <= self.order <= ORDER_MAX:
            raise ValueError("CharNgramLM: order %d, 1..MR_NGRAM_ORDER_MAX=%d are taken" % (self.order, ORDER_MAX))
        for gram, (lp, bow) in self.ngrams.items():
            if not 1 <= len(gram) <= self.order:
                raise ValueError("CharNgramLM: n-gram %r in a model of order %d" % (gram, self.order))
            if any(t not in (BOS, EOS) and (t == self.blank or t == self.unknown or not 0 <= t < self.classes) for t in gram):
                raise ValueError("CharNgramLM: n-gram %r holds blank, unknown or no class of the charset" % (gram,))
            if len(gram) > 1 and gram[:-1] not in self.ngrams:
                raise ValueError("CharNgramLM: n-gram %r is listed, its context %r is not" % (gram, gram[:-1]))
            if math.isnan(lp) or math.isnan(bow) or lp == math.inf or bow == math.inf:
                raise ValueError("CharNgramLM: n-gram %r has the values (%r, %r)" % (gram, lp, bow))
        listed = [v[0] for k, v in self.ngrams.items() if len(k) == 1 and k[0] != BOS and v[0] > -math.inf]
        if unk is None and not listed:
            raise ValueError("CharNgramLM: the model lists no unigram with a finite value")
        self.floor = float(unk) if unk is not None else min(listed)
        self.has_end = (EOS,) in self.ngrams
        # the automaton: one state per listed context that can be reached (no </s> inside) and is shorter than the order
        contexts = sorted((k for k in self.ngrams if len(k) < self.order and EOS not in k and BOS not in k[1:]),
                          key=lambda k: (len(k), k))
        self.contexts = [()] + contexts
        self.state_of = {ctx: i for i, ctx in enumerate(self.contexts)}
        self.states = len(self.contexts)
        self.start_state = self.state_of.get((BOS,), 0)
        self.bow = [0.0] + [self.ngrams[ctx][1] for ctx in contexts]
        self.backoff = [-1] + [self._suffix_state(ctx[1:]) for ctx in contexts]
        # arcs: (state, class) -> (lp, next state); next = the longest suffix of context + class that is a state
        self.arcs = {}
        for gram, (lp, _) in self.ngrams.items():
            if gram[-1] >= 0 and gram[:-1] in self.state_of:
                self.arcs[(self.state_of[gram[:-1]], gram[-1])] = (lp, self._suffix_state(gram[-(self.order - 1):]
                                                                                          if self.order > 1 else ()))
        self.end_lp = [self._backed_off(s, EOS)[0] if self.has_end else 0.0 for s in range(self.states)]
        self._resident = {}                         # (device, C) -> the device image, uploaded on first use

    def eligible(self, C=None):
        """The class ids a string may hold, below C (None: the charset's classes)."""
        return [c for c in range(self.classes if C is None else int(C)) if c != self.blank and c != self.unknown]

    def _suffix_state(self, ctx):
        """The state of the longest suffix of `ctx` that is a state."""
        ctx = tuple(ctx)
        while ctx not in self.state_of:
            ctx = ctx[1:]
        return self.state_of[ctx]

    def _backed_off(self, state, token):
        """(g(token | state), next state) in float64: the bows of the states backed off through, added first, then the value."""
        acc = 0.0
        while True:
            if token == EOS:
                hit = self.ngrams.get(self.contexts[state] + (EOS,))
                hit = None if hit is None else (hit[0], 0)
            else:
                hit = self.arcs.get((state, token))
                if hit is None and state == 0 and token >= 0 and token != self.blank and token != self.unknown:
                    hit = (self.floor, 0)           # the empty context lists every eligible class
            if hit is not None:
                return acc + hit[0], hit[1]
            if state == 0:
                return -math.inf, 0
            acc += self.bow[state]
            state = self.backoff[state]

    def step(self, state, c):
        """(g(c | state), the state of the string's context after c), float64 on the host."""
        return self._backed_off(state, int(c))

    def log_prob(self, ids, end=True):
        """The float64 log-probability of a string of class ids: from `start_state`, the sum of g, with end=True also
        g(</s> | the last state) when the model has `</s>`.  A string that holds blank or `unknown` scores -inf."""
        state, total = self.start_state, 0.0
        for c in ids:
            g, state = self.step(state, c)
            total += g
        return total + (self.end_lp[state] if end else 0.0)

    # ---- sources

    @classmethod
    def from_arpa(cls, text_or_path, charset=None):
        """An ARPA file (its text, or a path to it): `\\data\\` with the `ngram N=count` lines, the `\\N-grams:` sections of
        `log10 w1 .. wN [log10 bow]` lines, `\\end\\`.  Tokens are single characters, mapped through `charset.index`; `<space>` is
        ' '; `<s>`, `</s>` and `<unk>` keep their meaning.  An n-gram with a character outside the charset (or `<unk>` in an order
        above 1) is dropped and counted in `.skipped`.  ValueError: malformed text, an order above MR_NGRAM_ORDER_MAX, a count
        that disagrees with its section, the same n-gram twice, an n-gram whose context is not listed."""
        charset = charset if charset is not None else DefaultCharset()
        text = text_or_path
        if "\n" not in text and not text.lstrip().startswith("\\data\\"):
            if not os.path.exists(text):
                raise ValueError("CharNgramLM.from_arpa: neither ARPA text nor a file: %r" % (text,))
            with open(text, encoding="utf-8") as f:
                text = f.read()
        blank, unknown = getattr(charset, 'blank', 0), getattr(charset, 'unknown', 1)
        counts, found, ngrams, unk, skipped = {}, {}, {}, None, 0
        section, ended = None, False
        for number, line in enumerate(text.splitlines(), 1):
            line = line.strip()
            where = "CharNgramLM.from_arpa: line %d %r" % (number, line)
            if not line:
                continue
            if ended:
                raise ValueError("%s: text after \\end\\" % where)
            if line == "\\data\\":
                if section is not None:
                    raise ValueError("%s: a second \\data\\" % where)
                section = 0
            elif section is None:
                raise ValueError("%s: before \\data\\" % where)
            elif line == "\\end\\":
                ended = True
            elif line.startswith("\\"):
                if not (line.endswith("-grams:") and line[1:-7].isdigit()):
                    raise ValueError("%s: not a section" % where)
                section = int(line[1:-7])
                if section != len(found) + 1 or section not in counts:
                    raise ValueError("%s: the sections are 1, 2, .. as \\data\\ counts them" % where)
                found[section] = 0
            elif section == 0:
                head, _, value = line.partition("=")
                if not (head.split()[:1] == ["ngram"] and len(head.split()) == 2 and head.split()[1].isdigit()
                        and value.strip().isdigit()):
                    raise ValueError("%s: not `ngram N=count`" % where)
                n = int(head.split()[1])
                if n != len(counts) + 1:
                    raise ValueError("%s: the orders are 1, 2, .." % where)
                if n > ORDER_MAX:
                    raise ValueError("%s: order %d, MR_NGRAM_ORDER_MAX=%d are taken" % (where, n, ORDER_MAX))
                counts[n] = int(value)
            else:
                fields = line.split()
                if len(fields) not in (section + 1, section + 2):
                    raise ValueError("%s: a %d-gram line has a value, %d tokens and at most a backoff weight"
                                     % (where, section, section))
                try:
                    lp = float(fields[0]) * _LN10
                    bow = float(fields[section + 1]) * _LN10 if len(fields) == section + 2 else 0.0
                except ValueError:
                    raise ValueError("%s: not a number" % where)
                found[section] += 1
                gram, drop = [], False
                for token in fields[1:section + 1]:
                    if token in _SPECIAL:
                        gram.append(_SPECIAL[token])
                    elif token == "<unk>":
                        drop = True
                    else:
                        ch = ' ' if token == "<space>" else token
                        if len(ch) != 1:
                            raise ValueError("%s: token %r is not one character" % (where, token))
                        c = charset.index(ch)
                        drop = drop or c == unknown or c == blank
                        gram.append(c)
                if fields[1:section + 1] == ["<unk>"]:
                    unk = lp
                elif drop:
                    skipped += 1
                elif tuple(gram) in ngrams:
                    raise ValueError("%s: the n-gram is listed twice (after the charset's folding)" % where)
                else:
                    ngrams[tuple(gram)] = (lp, bow)
        if not ended or not counts:
            raise ValueError("CharNgramLM.from_arpa: no \\data\\ counts, or no \\end\\")
        for n, count in counts.items():
            if found.get(n) != count:
                raise ValueError("CharNgramLM.from_arpa: \\data\\ counts %d %d-grams, the section has %r" % (count, n, found.get(n)))
        return cls(ngrams, charset, order=len(counts), unk=unk, skipped=skipped)

    @classmethod
    def train(cls, words, charset=None, order=3, discount=0.75):
        """Interpolated absolute discounting over `words` (strings), each framed by `<s>` / `</s>`, stored in backoff form:
            p(c | ctx) = max(count(ctx, c) - D, 0) / count(ctx, .) + gamma(ctx) * p(c | ctx[1:]),
            gamma(ctx) = D * (distinct successors of ctx) / count(ctx, .),     bow(ctx) = log gamma(ctx),
        unigrams add-one over the eligible classes and `</s>`.  Every seen n-gram is listed with p; an unseen one backs off to
        gamma(ctx) * p(c | ctx[1:]), which is the same formula.  A word with a character outside the charset is left out and
        counted in `.skipped`."""
        charset = charset if charset is not None else DefaultCharset()
        order, D = int(order), float(discount)
        if not 1 <= order <= ORDER_MAX:
            raise ValueError("CharNgramLM.train: order %d, 1..MR_NGRAM_ORDER_MAX=%d are taken" % (order, ORDER_MAX))
        if not 0.0 < D < 1.0:
            raise ValueError("CharNgramLM.train: discount must be in (0, 1), got %r" % (discount,))
        blank, unknown = getattr(charset, 'blank', 0), getattr(charset, 'unknown', 1)
        vocab = [c for c in range(len(charset)) if c != blank and c != unknown] + [EOS]
        count, skipped = {}, 0                          # n-gram -> occurrences, the last token a predicted one
        for word in words:
            ids = [charset.index(ch) for ch in word]
            if any(c == unknown or c == blank for c in ids):
                skipped += 1
                continue
            seq = [BOS] + ids + [EOS]
            for i in range(1, len(seq)):
                for n in range(1, min(order, i + 1) + 1):
                    gram = tuple(seq[i - n + 1:i + 1])
                    count[gram] = count.get(gram, 0) + 1
        total, successors = {}, {}                      # context -> count(ctx, .), distinct successors
        for gram, k in count.items():
            total[gram[:-1]] = total.get(gram[:-1], 0) + k
            successors[gram[:-1]] = successors.get(gram[:-1], 0) + 1
        prob = {(w,): (count.get((w,), 0) + 1.0) / (total.get((), 0) + len(vocab)) for w in vocab}

        def lower(gram):                                # p(gram[-1] | gram[:-1]) of a gram that need not be listed
            while gram not in prob:
                ctx = gram[:-1]
                if ctx in total:
                    return D * successors[ctx] / total[ctx] * lower(gram[1:])
                gram = gram[1:]
            return prob[gram]
        for gram in sorted((g for g in count if len(g) > 1), key=len):
            ctx = gram[:-1]
            prob[gram] = (count[gram] - D) / total[ctx] + D * successors[ctx] / total[ctx] * lower(gram[1:])
        ngrams = {gram: (math.log(p), 0.0) for gram, p in prob.items()}
        ngrams[(BOS,)] = (-99.0 * _LN10, 0.0)
        for ctx in total:
            if ctx and len(ctx) < order:
                ngrams[ctx] = (ngrams[ctx][0], math.log(D * successors[ctx] / total[ctx]))
        return cls(ngrams, charset, order=order, skipped=skipped)

    def to_arpa(self):
        """The model as ARPA text (log10, nine significant digits): `from_arpa` of it gives the same model."""
        def name(token):
            if token == BOS:
                return "<s>"
            if token == EOS:
                return "</s>"
            return "<space>" if self.charset[token] == ' ' else self.charset[token]
        by_order = [sorted(k for k in self.ngrams if len(k) == n) for n in range(1, self.order + 1)]
        lines = ["\\data\\"] + ["ngram %d=%d" % (n + 1, len(grams)) for n, grams in enumerate(by_order)]
        for n, grams in enumerate(by_order):
            lines += ["", "\\%d-grams:" % (n + 1)]
            for gram in grams:
                lp, bow = self.ngrams[gram]
                line = "%.9g\t%s" % (lp / _LN10, " ".join(name(t) for t in gram))
                lines.append(line + ("\t%.9g" % (bow / _LN10) if bow != 0.0 else ""))
        return "\n".join(lines + ["", "\\end\\", ""])

    # ---- the device image

    def image(self, C=None):
        """The automaton as the header lays it out, for a posterior of C classes (None: the charset's), as a dict of numpy arrays
        and ints: keys u64 [slots], arc_lp f32 [slots], arc_next i32 [slots], bow f32 [states], backoff i32 [states], end_lp f32
        [states], states, slots, max_probe, start_state, order.  State 0 lists every eligible class below C (a class past the
        charset's takes the floor as well).  Raises ValueError where an invariant of the kernel does not hold."""
        C = self.classes if C is None else int(C)
        if C < self.classes:
            raise ValueError("CharNgramLM: the model is over %d classes, the posterior has C=%d" % (self.classes, C))
        arcs = dict(self.arcs)
        for c in self.eligible(C):
            arcs.setdefault((0, c), (self.floor, 0))
        slots = max(2 * len(arcs), 2)
        if self.states >= 2 ** 31 or slots >= 2 ** 31:
            raise ValueError("CharNgramLM: %d states and %d arcs do not fit the device image" % (self.states, len(arcs)))
        keys = np.zeros(slots, dtype=np.uint64)
        arc_lp = np.zeros(slots, dtype=np.float32)
        arc_next = np.zeros(slots, dtype=np.int32)
        max_probe = 1
        for (state, sym), (lp, nxt) in sorted(arcs.items()):
            h, probes = arc_hash(state, sym, slots), 1
            while keys[h] != 0:
                h, probes = (h + 1) % slots, probes + 1
            keys[h] = (state << 32) | (sym + 1)
            arc_lp[h], arc_next[h] = lp, nxt
            max_probe = max(max_probe, probes)
        img = dict(keys=keys, arc_lp=arc_lp, arc_next=arc_next, bow=np.asarray(self.bow, dtype=np.float32),
                   backoff=np.asarray(self.backoff, dtype=np.int32), end_lp=np.asarray(self.end_lp, dtype=np.float32),
                   states=self.states, slots=slots, max_probe=max_probe, start_state=self.start_state, order=self.order)
        self._check(img, arcs, C)
        return img

    def _check(self, img, arcs, C):
        """What the kernel relies on: states in range, backoff chains that strictly shorten and end in state 0 within `order`
        steps, finite values, a table at most half full, state 0 complete."""
        S, lengths = img['states'], [len(ctx) for ctx in self.contexts]
        used = img['keys'] != 0
        ok = (S >= 1 and 0 <= img['start_state'] < S and int(used.sum()) == len(arcs) and 2 * len(arcs) <= img['slots']
              and img['backoff'][0] == -1 and lengths[0] == 0 and max(lengths) < self.order
              and np.all((img['arc_next'][used] >= 0) & (img['arc_next'][used] < S))
              and all(0 <= b < S and lengths[b] < lengths[s] for s, b in enumerate(self.backoff) if s > 0)
              and np.all(np.isfinite(img['arc_lp'][used])) and np.all(np.isfinite(img['bow']))
              and np.all(np.isfinite(img['end_lp'])) and all((0, c) in arcs for c in self.eligible(C)))
        if not ok:
            raise ValueError("CharNgramLM: the automaton breaks an invariant of mr_ctc_beam_search_lm (values that are not "
                             "finite in float32, or a context table that is not closed)")

    def _tensors(self, device, C):
        device = torch.device(device)
        got = self._resident.get((device, C))
        if got is None:
            img = self.image(C)
            got = dict(img)
            got['keys'] = torch.from_numpy(img['keys'].view(np.int64)).to(device)
            for name in ('arc_lp', 'arc_next', 'bow', 'backoff', 'end_lp'):
                got[name] = torch.from_numpy(img[name]).to(device)
            self._resident[(device, C)] = got
        return got
