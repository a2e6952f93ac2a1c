"""A backoff n-gram model as a dict of n-grams, scored straight from the ARPA definition -- no automaton, no states, nothing of
megreader_amd/ops/language_model.py:
    g(c | ctx) = lp(ctx + c) if that n-gram is listed, else bow(ctx) (0 for a context that is not listed) + g(c | ctx[1:]),
with the context cut to its last order - 1 tokens first; the empty context gives an eligible class that is not listed the floor
(the `<unk>` value, else the smallest unigram value, `<s>` aside).  Natural logs, float64.  Tokens are class ids, BOS for `<s>`
and EOS for `</s>`."""
import math

BOS, EOS = -1, -2
LN10 = math.log(10.0)


def parse_arpa(text, index):
    """({n-gram tuple: (lp, bow)}, order, the <unk> value or None) of ARPA text; `index` maps a character to its class id.  The
    reader of a test: it trusts the text (n-grams with <unk> above order 1 are left out)."""
    ngrams, n, unk = {}, 0, None
    for line in text.splitlines():
        line = line.strip()
        if line.endswith("-grams:"):
            n = int(line[1:-7])
        elif n and line and not line.startswith("\\"):
            fields = line.split()
            tokens = fields[1:n + 1]
            lp = float(fields[0]) * LN10
            bow = float(fields[n + 1]) * LN10 if len(fields) > n + 1 else 0.0
            if tokens == ["<unk>"]:
                unk = lp
            elif "<unk>" not in tokens:
                gram = tuple(BOS if t == "<s>" else EOS if t == "</s>" else index(' ' if t == "<space>" else t) for t in tokens)
                ngrams[gram] = (lp, bow)
    return ngrams, n, unk


class DictLM(object):
    """The scorer.  A "state" is the history itself, cut to its last order - 1 tokens."""

    def __init__(self, ngrams, order, eligible, unk=None):
        self.ngrams, self.order, self.eligible = dict(ngrams), order, set(eligible)
        self.floor = unk if unk is not None else min(v[0] for k, v in ngrams.items() if len(k) == 1 and k[0] != BOS)
        self.start = (BOS,) if (BOS,) in ngrams and order > 1 else ()
        self.has_end = (EOS,) in ngrams

    def cut(self, ctx):
        return tuple(ctx)[len(ctx) - (self.order - 1):] if len(ctx) > self.order - 1 else tuple(ctx)

    def terms(self, ctx, c):
        """([the backoff weights in the order they are met], the value of the n-gram found or None, the next history)."""
        ctx, bows = self.cut(ctx), []
        nxt = self.cut(ctx + (c,))
        while True:
            hit = self.ngrams.get(ctx + (c,))
            if hit is not None:
                return bows, hit[0], nxt
            if not ctx:
                return bows, (self.floor if c in self.eligible else None), nxt
            if ctx in self.ngrams:
                bows.append(self.ngrams[ctx][1])
            ctx = ctx[1:]

    def g(self, ctx, c):
        bows, value, _ = self.terms(ctx, c)
        return -math.inf if value is None else sum(bows) + value

    def end(self, ctx):
        return self.g(ctx, EOS) if self.has_end else 0.0

    def log_prob(self, ids, end=True):
        ctx, total = self.start, 0.0
        for c in ids:
            total += self.g(ctx, c)
            ctx = self.cut(ctx + (c,))
        return total + (self.end(ctx) if end else 0.0)
