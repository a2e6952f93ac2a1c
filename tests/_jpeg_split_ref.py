"""Numpy/Python restatement of the split JPEG decoder of csrc/jpeg_split.hip (self-synchronising sub-sequence decoding), on top
of tests/_jpeg_ref.py, which it imports and does not change.

THE CUT.  A work item's bytes are UNSTUFFED first (the byte after every FF is dropped); sub-sequence i covers unstuffed bytes
[i * S, (i + 1) * S), i.e. bits [i * S * 8, end_i) with end_i = min((i + 1) * S, U) * 8 and U the number of unstuffed bytes.  The
NUMBER of sub-sequences comes from the stuffed length, n_sub = ceil(len / S) (the host plan does not unstuff), so the last ones can
be empty.

THE STATE RULE.  Between two symbols the serial decoder is in state (p, b, k): bit position, block slot in the MCU (0 .. B - 1,
B = hs * vs + 2 for colour, 1 for gray), zigzag index (0: a DC size comes next).  `Stream.step` is the serial rule as a total
function: an invalid code takes 16 bits and yields symbol 0, the DC size is masked to 4 bits, a run past 63 ends the block, bits
past the end are zeros.  F_i(state) = step while p < end_i.

THE REPAIR.  Exact entry states: in[0] = (0, 0, 0), in[i + 1] = F_i(in[i]) (`serial_states`).  `synchronise` finds them the way
the device does: every sub-sequence starts from the guess (i * S * 8, 0, 0) and is decoded again whenever the state it was last
decoded from differs from the state its predecessor produced -- rounds inside workgroups of 256 sub-sequences, and one pass per
workgroup boundary that hands workgroup g the exit of g - 1 from the pass before.

`decode_status` = entry states -> block offsets (prefix sum of completed blocks) -> coefficients with DC differences -> DC prefix
sums -> the IDCT and colour code of _jpeg_ref.  Status as the device raises it: CORRUPT for an invalid code, a DC size above 11
or a run past 63 inside one of the item's n_blocks blocks, for fewer than n_blocks completed blocks, and for a last wanted block
that ends past the item's bits; blocks beyond n_blocks are dropped silently.
"""
import numpy as np

import _jpeg_ref as ref

OK, UNSUPPORTED, CORRUPT = ref.OK, ref.UNSUPPORTED, ref.CORRUPT
WG = 256                    # sub-sequences per workgroup
SPLIT_MAX_LEN = 1 << 27


def align16(v):
    return (v + 15) // 16 * 16


def unstuff(data):
    raw = bytearray()
    i = 0
    while i < len(data):
        raw.append(data[i])
        if data[i] == 0xFF:
            i += 1
            while i < len(data) and data[i] == 0xFF:
                i += 1
        i += 1
    return bytes(raw)


class Stream(object):
    """One work item: its unstuffed bytes, the tables of its image, and the step rule."""

    def __init__(self, p, data, nmcu, S):
        self.raw = unstuff(data)
        self.nbits = len(self.raw) * 8
        self.pad = self.raw + b'\0' * 8
        self.S = S
        self.n_sub = -(-len(data) // S)
        self.B = p.hs * p.vs + 2 if p.ncomp == 3 else 1
        self.ny = self.B - 2 if p.ncomp == 3 else 1
        self.n_blocks = nmcu * self.B
        self.huff = p.huff
        self.td, self.ta = p.comp_td, p.comp_ta
        self._memo = {}

    def end(self, i):
        return min((i + 1) * self.S * 8, self.nbits)

    def peek(self, pos, n):
        """n <= 16 bits from bit `pos` (zeros past the end)."""
        q = pos >> 3
        if q >= len(self.raw):
            return 0
        w = int.from_bytes(self.pad[q:q + 4], 'big')
        return (w >> (32 - n - (pos & 7))) & ((1 << n) - 1) if n else 0

    def step(self, pos, b, k):
        """One symbol from (pos, b, k): (pos', b', k', done, at, value, error).  `at`: zigzag index the value belongs to (0: a
        DC difference, -1: none); `done`: the step completed a block."""
        c = 0 if b < self.ny else b - self.ny + 1
        maxcode, valoff, syms = self.huff[self.td[c] if k == 0 else 2 + self.ta[c]]
        w = self.peek(pos, 16)
        sym, err = 0, True
        use = 16
        for l in range(1, 17):
            if (w >> (16 - l)) <= maxcode[l]:
                sym, err, use = syms[(w >> (16 - l)) + valoff[l]], False, l
                break
        pos += use
        done, at, val = False, -1, 0
        if k == 0:
            if sym > 11:
                err = True
            s = sym & 15
            v = self.peek(pos, s)
            val = v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v
            pos += s
            at, k = 0, 1
        else:
            r, s = sym >> 4, sym & 15
            if s == 0:
                if r != 15:
                    done = True
                else:
                    k += 16
                    done = k >= 64
            else:
                k += r
                if k > 63:
                    err = done = True
                else:
                    v = self.peek(pos, s)
                    val = v - (1 << s) + 1 if v < (1 << (s - 1)) else v
                    pos += s
                    at = k
                    k += 1
                    done = k == 64
        if done:
            k, b = 0, (b + 1) % self.B
        return pos, b, k, done, at, val, err

    def F(self, i, state):
        """(exit state, blocks completed) of sub-sequence i decoded from `state`."""
        key = (i,) + state
        hit = self._memo.get(key)
        if hit is None:
            pos, b, k = state
            end, n = self.end(i), 0
            while pos < end:
                pos, b, k, done = self.step(pos, b, k)[:4]
                n += done
            hit = self._memo[key] = ((pos, b, k), n)
        return hit

    def guess(self, i):
        return (i * self.S * 8, 0, 0)

    def serial_states(self):
        """The entry state of every sub-sequence by the serial walk, and the blocks completed inside each."""
        states, counts = [(0, 0, 0)], []
        for i in range(self.n_sub):
            out, n = self.F(i, states[-1])
            states.append(out)
            counts.append(n)
        return states[:-1], counts

    def synchronise(self):
        """The device's schedule.  Returns (in states, exit states, blocks per sub-sequence, rounds of each workgroup in pass 0,
        workgroups re-decoded per later pass)."""
        n, n_wg = self.n_sub, -(-self.n_sub // WG)
        ins = [self.guess(i) for i in range(n)]
        outs = [self.F(i, ins[i]) for i in range(n)]
        wg_exit = [[None] * n_wg, [None] * n_wg]
        rounds, redone = [], []

        def repair(g):
            lo, hi = g * WG, min(n, (g + 1) * WG)
            used = 0
            for r in range(hi - lo):
                changed = [i for i in range(lo + 1, hi) if outs[i - 1][0] != ins[i]]
                if not changed:
                    break
                used += 1
                new = [(i, outs[i - 1][0]) for i in changed]        # all lanes read before any lane writes
                for i, s in new:
                    ins[i] = s
                for i, s in new:
                    outs[i] = self.F(i, s)
            return used, outs[hi - 1][0]

        for g in range(n_wg):
            used, ex = repair(g)
            rounds.append(used)
            wg_exit[0][g] = ex
        for q in range(1, n_wg):
            cur, prev = wg_exit[q & 1], wg_exit[(q & 1) ^ 1]
            count = 0
            for g in range(q, n_wg):
                if prev[g - 1] == ins[g * WG]:
                    cur[g] = prev[g]
                    continue
                count += 1
                ins[g * WG] = prev[g - 1]
                outs[g * WG] = self.F(g * WG, ins[g * WG])
                cur[g] = repair(g)[1]
            redone.append(count)
        assert ins[0] == (0, 0, 0) and all(ins[i] == outs[i - 1][0] for i in range(1, n))   # the chain condition
        return ins, [o[0] for o in outs], [o[1] for o in outs], rounds, redone

    def sync_distance(self, i, states):
        """How many sub-sequences a decoder started from the guess of sub-sequence i needs until its state equals the serial
        decoder's (0: the guess is right); None if it never does before the item ends."""
        s = self.guess(i)
        for j in range(i, self.n_sub):
            if s == states[j]:
                return j - i
            s = self.F(j, s)[0]
        return None

    def coefficients(self, ins, counts):
        """(block offsets, dc [n_blocks] differences, coef [n_blocks][64] in zigzag order (index 0 unused), status)."""
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        dc = np.zeros(self.n_blocks, dtype=np.int64)
        coef = np.zeros((self.n_blocks, 64), dtype=np.int64)
        status = OK if offs[-1] >= self.n_blocks else CORRUPT
        for i in range(self.n_sub):
            (pos, b, k), blk, end = ins[i], int(offs[i]), self.end(i)
            while pos < end and blk < self.n_blocks:
                pos, b, k, done, at, val, err = self.step(pos, b, k)
                if at == 0:
                    dc[blk] = val
                elif at > 0:
                    coef[blk, at] = val
                if err or (done and blk == self.n_blocks - 1 and pos > self.nbits):
                    status = CORRUPT
                blk += done
        return offs[:-1], dc, coef, status


def streams(blob, S, split_above=0, parsed=None):
    """[(item index in the image, Stream)] of the items of `blob` longer than split_above."""
    p = ref.parse(blob) if parsed is None else parsed
    return [(j, Stream(p, bytes(blob)[off:off + length], nmcu, S)) for j, (mcu0, nmcu, off, length) in enumerate(p.items)
            if split_above < length < SPLIT_MAX_LEN]


def workspace_planes(p):
    """The unsplit plan's workspace bytes of one OK image (csrc/jpeg_plan.h: plan)."""
    total = 0
    for c in range(p.ncomp):
        total = align16(total + p.mcu_w * 8 * (p.hs if c == 0 else 1) * p.mcu_h * 8 * (p.vs if c == 0 else 1))
    return total


def split_table(parsed, split_above, S):
    """mr_jpeg_plan_split over a batch of `Parsed`: ([one dict per split item, named as mr_jpeg_split], the workspace total)."""
    ws = sum(workspace_planes(p) for p in parsed if p.status == OK)
    table, item = [], 0

    def take(nbytes):
        nonlocal ws
        at = ws
        ws = align16(ws + nbytes)
        return at

    for image, p in enumerate(parsed):
        if p.status != OK:
            continue
        for mcu0, nmcu, off, length in p.items:
            if split_above < length < SPLIT_MAX_LEN:
                e = dict(item=item, image=image, subseq_bytes=S, n_sub=-(-length // S))
                e['n_wg'] = -(-e['n_sub'] // WG)
                e['blocks_per_mcu'] = p.hs * p.vs + 2 if p.ncomp == 3 else 1
                e['n_blocks'] = nmcu * e['blocks_per_mcu']
                e['reserved'] = 0
                e['meta_off'] = take(16)
                e['raw_bytes'] = align16(e['n_sub'] * S) + 16
                e['raw_off'] = take(e['raw_bytes'])
                e['in_off'] = take(8 * e['n_sub'])
                e['exit_off'] = take(8 * e['n_sub'])
                e['wg_exit_off'] = take(16 * e['n_wg'])
                e['block_off'] = take(4 * e['n_sub'])
                e['coef_bytes'] = align16(4 * e['n_blocks']) + 128 * e['n_blocks']
                e['coef_off'] = take(e['coef_bytes'])
                table.append(e)
            item += 1
    return table, ws


def item_coefficients(p, data, mcu0, nmcu, S, coef):
    """Like _jpeg_ref._decode_item, through the split decoder: fills coef[c][block row][block col][64] (dequantised, natural
    order) and returns the status."""
    st = Stream(p, data, nmcu, S)
    ins, _, counts, _, _ = st.synchronise()
    _, dc, zz, status = st.coefficients(ins, counts)
    samp = [(p.hs, p.vs)] + [(1, 1)] * (p.ncomp - 1)
    pred = [0] * p.ncomp
    for j in range(st.n_blocks):
        m, slot = mcu0 + j // st.B, j % st.B
        c = 0 if slot < st.ny else slot - st.ny + 1
        sub = slot if c == 0 else 0
        by, bx = divmod(sub, samp[c][0])
        my, mx = divmod(m, p.mcu_w)
        q = p.quant[p.comp_tq[c]]
        pred[c] += int(dc[j])
        blk = coef[c][my * samp[c][1] + by, mx * samp[c][0] + bx]
        blk[ref.ZIGZAG[1:]] = zz[j, 1:] * q[1:]
        blk[0] = pred[c] * q[0]
    return status


def decode_status(blob, S, split_above=0, rgb=False):
    """(uint8 [h, w, 3] or None, status): items longer than split_above through the split decoder, the others through
    _jpeg_ref._decode_item; IDCT, upsampling and colour conversion are _jpeg_ref's."""
    p = ref.parse(blob)
    if p.status != OK:
        return None, p.status
    samp = [(p.hs, p.vs)] + [(1, 1)] * (p.ncomp - 1)
    coef = [np.zeros((p.mcu_h * sv, p.mcu_w * sh, 64), dtype=np.int64) for sh, sv in samp]
    status = OK
    for mcu0, nmcu, off, length in p.items:
        data = bytes(blob)[off:off + length]
        if split_above < length < SPLIT_MAX_LEN:
            status = max(status, item_coefficients(p, data, mcu0, nmcu, S, coef))
        else:
            status = max(status, ref._decode_item(data, p, mcu0, nmcu, coef))
    return pixels_of(p, coef, rgb), status


def pixels_of(p, coef, rgb=False):
    """The tail of _jpeg_ref.decode_status: coefficient arrays -> uint8 [h, w, 3]."""
    planes = [ref.idct_blocks(c).swapaxes(1, 2).reshape(c.shape[0] * 8, c.shape[1] * 8) for c in coef]
    h, w = p.h, p.w
    y = planes[0][:h, :w].astype(np.int64)
    if p.ncomp == 1:
        out = np.stack([y, y, y], axis=-1)
    else:
        ch, cw = -(-h // p.vs), -(-w // p.hs)
        chroma = []
        for c in planes[1:]:
            c = c[:ch, :cw]
            chroma.append(c.astype(np.int64) if p.hs == 1 else ref._h2v1(c, w) if p.vs == 1 else ref._h2v2(c, h, w))
        cb, cr = chroma[0] - 128, chroma[1] - 128
        r = y + ((91881 * cr + 32768) >> 16)
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
        out = np.stack([r, g, b] if rgb else [b, g, r], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)
