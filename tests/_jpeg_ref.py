"""Numpy restatement of the baseline JPEG decoder of csrc/jpeg.hip, blob -> uint8 HWC (BGR by default).

Written from the JPEG standard (ITU-T T.81: marker syntax B.2, Huffman table generation C.2 / F.2.2.3, EXTEND F.2.2.1, zigzag
order A.3.6, restart intervals E.2.4) and from a description of the default decode of the common JPEG libraries, which is what
PIL returns:

* dequantise, then the "slow integer" 8x8 inverse DCT: 13-bit fixed-point constants FIX(x) = round(x * 2**13), a column pass
  that keeps 2 extra bits (descale by 11) and a row pass that removes them with the factor 8 (descale by 18), + 128;
* the result indexes a range-limit table with its low 10 bits: as a signed 10-bit number s, the table holds clamp(s + 128);
* chroma planes of real size ceil(w / 2) [x ceil(h / 2)] are brought to full size by triangle ("fancy") filters when they are more
  than 2 samples wide, by plain replication otherwise:
    h2v1: out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2, first and last output = the edge sample
    h2v2: s[i] = 3 near[i] + far[i] with `far` the row above (even output rows) or below (odd), the edge ROW OF THE REAL PLANE
          replicated; out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, first output
          (4 s[0] + 8) >> 4, last output (4 s[last] + 7) >> 4;
* YCbCr -> RGB in 16-bit fixed point: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16) with cb, cr centred on 128 (both chroma terms summed before the shift), clamped.

`parse` mirrors the host plan (csrc/jpeg_plan.h: the same supported set, the same statuses, the same work items); the CPU tests
compare the two field by field, and this file against PIL bit for bit.  No PIL, no project import: it runs wherever numpy does.
"""
import numpy as np

OK, UNSUPPORTED, CORRUPT = 0, 1, 2

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])            # natural (row-major) index of the k-th coefficient in zigzag order


class Parsed(object):
    """What the plan holds for one image (status != OK: only `status` is meaningful)."""

    def __init__(self, status):
        self.status = status


def _huffman(counts):
    """Canonical table (T.81 C.2): maxcode[l] (-1: no code of length l), valoff[l] = index of the first symbol of length l minus
    its code, for l = 1..16 (index 0 unused).  None if a code does not fit its length."""
    maxcode, valoff = [-1] * 17, [0] * 17
    code = k = 0
    for l in range(1, 17):
        if counts[l - 1]:
            valoff[l] = k - code
            code += counts[l - 1]
            k += counts[l - 1]
            if code > (1 << l):
                return None
            maxcode[l] = code - 1
        code <<= 1
    return maxcode, valoff


def parse(blob):
    blob = bytes(blob)
    n = len(blob)
    if n < 2 or blob[0] != 0xFF or blob[1] != 0xD8:
        return Parsed(UNSUPPORTED)
    pos = 2
    quant, huff = {}, {}                                # tq -> 64 bytes (zigzag order); table 0..3 (DC0 DC1 AC0 AC1) -> ...
    frame = None
    restart = 0
    jfif = adobe = False
    transform = -1
    while True:
        if pos >= n or blob[pos] != 0xFF:
            return Parsed(CORRUPT)
        while pos < n and blob[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return Parsed(CORRUPT)
        m = blob[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if m == 0xD9 or m == 0x00:
            return Parsed(CORRUPT)
        if pos + 2 > n:
            return Parsed(CORRUPT)
        L = blob[pos] << 8 | blob[pos + 1]
        if L < 2 or pos + L > n:
            return Parsed(CORRUPT)
        seg = blob[pos + 2:pos + L]
        if m == 0xC0:
            if frame is not None or len(seg) < 6:
                return Parsed(CORRUPT)
            prec, h, w, nc = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if prec != 8:
                return Parsed(UNSUPPORTED)
            if nc not in (1, 3):
                return Parsed(UNSUPPORTED)
            if len(seg) != 6 + 3 * nc or h == 0 or w == 0:
                return Parsed(CORRUPT)
            comps = []
            for c in range(nc):
                cid, hv, tq = seg[6 + 3 * c:9 + 3 * c]
                if tq > 3:
                    return Parsed(CORRUPT)
                comps.append((cid, hv >> 4, hv & 15, tq))
            frame = (h, w, comps)
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            return Parsed(UNSUPPORTED)                  # progressive, lossless, arithmetic, extended: not on the device
        elif m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0:
                    return Parsed(UNSUPPORTED if pq == 1 else CORRUPT)
                if tq > 3 or i + 65 > len(seg):
                    return Parsed(CORRUPT)
                quant[tq] = seg[i + 1:i + 65]
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                if tc > 1 or th > 3 or i + 17 > len(seg):
                    return Parsed(CORRUPT)
                if th > 1:
                    return Parsed(UNSUPPORTED)
                counts = list(seg[i + 1:i + 17])
                total = sum(counts)
                if total > 256 or i + 17 + total > len(seg):
                    return Parsed(CORRUPT)
                canon = _huffman(counts)
                if canon is None:
                    return Parsed(CORRUPT)
                huff[tc * 2 + th] = (canon[0], canon[1], seg[i + 17:i + 17 + total])
                i += 17 + total
        elif m == 0xDD:
            if L != 4:
                return Parsed(CORRUPT)
            restart = seg[0] << 8 | seg[1]
        elif m == 0xE0:
            if len(seg) >= 5 and seg[:5] == b'JFIF\0':
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                adobe, transform = True, seg[11]
        elif m == 0xDA:
            if frame is None or len(seg) < 1:
                return Parsed(CORRUPT)
            h, w, comps = frame
            ns = seg[0]
            if ns < 1 or ns > 4 or len(seg) != 4 + 2 * ns:
                return Parsed(CORRUPT)
            if ns != len(comps):
                return Parsed(UNSUPPORTED)              # one scan per component (or a subset): multi-scan
            sel = []
            for c in range(ns):
                cid, t = seg[1 + 2 * c], seg[2 + 2 * c]
                if cid != comps[c][0]:
                    return Parsed(UNSUPPORTED)
                if (t >> 4) > 1 or (t & 15) > 1:
                    return Parsed(UNSUPPORTED)
                sel.append((t >> 4, t & 15))
            if seg[1 + 2 * ns] != 0 or seg[2 + 2 * ns] != 63 or seg[3 + 2 * ns] != 0:
                return Parsed(UNSUPPORTED)
            for c in range(ns):
                if comps[c][3] not in quant or sel[c][0] not in huff or 2 + sel[c][1] not in huff:
                    return Parsed(CORRUPT)
            pos += L
            break
        pos += L
    if len(comps) == 3:
        if jfif:
            pass
        elif adobe:
            if transform == 0:
                return Parsed(UNSUPPORTED)              # RGB stored as is
        elif [c[0] for c in comps] == [82, 71, 66]:
            return Parsed(UNSUPPORTED)                  # components named 'R', 'G', 'B'
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
            return Parsed(UNSUPPORTED)
    else:
        hs = vs = 1                                     # a single-component scan is not interleaved: its sampling is moot
    p = Parsed(OK)
    p.h, p.w, p.ncomp, p.hs, p.vs, p.restart = h, w, len(comps), hs, vs, restart
    p.mcu_w, p.mcu_h = -(-w // (8 * hs)), -(-h // (8 * vs))
    p.comp_tq = [c[3] for c in comps]
    p.comp_td = [s[0] for s in sel]
    p.comp_ta = [s[1] for s in sel]
    p.quant = {t: np.frombuffer(q, dtype=np.uint8).astype(np.int64) for t, q in quant.items()}
    p.huff = huff
    # the entropy-coded segment: up to the first marker that is neither a stuffed FF 00 nor RSTn (or the end of the blob)
    p.scan_off = pos
    starts, rst = [pos], []
    i = pos
    end = n
    while i < n:
        if blob[i] != 0xFF:
            i += 1
            continue
        j = i + 1
        while j < n and blob[j] == 0xFF:
            j += 1                                      # fill bytes in front of a marker
        if j >= n:
            end = i
            break
        if blob[j] == 0:
            i = j + 1
            continue
        if 0xD0 <= blob[j] <= 0xD7:
            rst.append((i, blob[j] - 0xD0))
            starts.append(j + 1)
            i = j + 1
            continue
        end = i
        break
    p.scan_len = end - pos
    total = p.mcu_w * p.mcu_h
    if restart == 0:
        if rst:
            return Parsed(CORRUPT)
        p.items = [(0, total, pos, end - pos)]
    else:
        want = -(-total // restart)
        if len(rst) != want - 1:
            return Parsed(CORRUPT)
        if any(k != i % 8 for i, (_, k) in enumerate(rst)):
            return Parsed(CORRUPT)
        ends = [r[0] for r in rst] + [end]
        p.items = [(i * restart, min(restart, total - i * restart), starts[i], ends[i] - starts[i]) for i in range(want)]
    return p


def _decode_item(data, p, mcu0, nmcu, coef):
    """Huffman-decode MCUs mcu0 .. mcu0+nmcu-1 from the stuffed bytes `data` into coef[c][block row][block col][64] (dequantised,
    natural order).  Returns OK or CORRUPT; bits past the end of `data` read as zeros."""
    raw = bytearray()
    i = 0
    while i < len(data):
        raw.append(data[i])
        if data[i] == 0xFF:
            i += 1                                      # the plan leaves only FF 00 (and fill FF) inside an item
            while i < len(data) and data[i] == 0xFF:
                i += 1
        i += 1
    nbits = len(raw) * 8
    bits = np.unpackbits(np.frombuffer(bytes(raw) + b'\0' * 8, dtype=np.uint8)).tolist()
    pos = 0
    status = OK

    def get(k):
        nonlocal pos
        v = 0
        for b in bits[pos:pos + k]:
            v = v << 1 | b
        v <<= k - len(bits[pos:pos + k])
        pos += k
        return v

    def symbol(table):
        nonlocal pos, status
        maxcode, valoff, syms = p.huff[table]
        code = 0
        for l in range(1, 17):
            code = code << 1 | (bits[pos + l - 1] if pos + l - 1 < len(bits) else 0)
            if code <= maxcode[l]:
                pos += l
                return syms[code + valoff[l]]
        status = CORRUPT
        pos += 16
        return 0

    def extend(v, s):
        return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v

    pred = [0] * p.ncomp
    samp = [(p.hs, p.vs)] + [(1, 1)] * (p.ncomp - 1)
    for m in range(mcu0, mcu0 + nmcu):
        my, mx = divmod(m, p.mcu_w)
        for c in range(p.ncomp):
            q = p.quant[p.comp_tq[c]]
            for by in range(samp[c][1]):
                for bx in range(samp[c][0]):
                    blk = coef[c][my * samp[c][1] + by, mx * samp[c][0] + bx]
                    s = symbol(p.comp_td[c])
                    if s > 11:
                        status = CORRUPT
                        s &= 15
                    pred[c] += extend(get(s), s)
                    blk[0] = pred[c] * q[0]
                    k = 1
                    while k < 64:
                        rs = symbol(2 + p.comp_ta[c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            status = CORRUPT
                            break
                        blk[ZIGZAG[k]] = extend(get(s), s) * q[k]
                        k += 1
                    if pos > len(bits):
                        pos = len(bits)
    if pos > nbits:
        status = CORRUPT
    return status


def _fix(x):
    return int(x * 8192 + 0.5)


def _idct_1d(v, shift):
    """One pass of the slow-integer inverse DCT along the last axis (8 values, int64): even part from v0 v2 v4 v6, odd part
    from v1 v3 v5 v7, outputs descaled by `shift` with rounding."""
    z2, z3 = v[..., 2], v[..., 6]
    z1 = (z2 + z3) * _fix(0.541196100)
    t2 = z1 - z3 * _fix(1.847759065)
    t3 = z1 + z2 * _fix(0.765366865)
    t0 = (v[..., 0] + v[..., 4]) << 13
    t1 = (v[..., 0] - v[..., 4]) << 13
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * _fix(1.175875602)
    o0 = o0 * _fix(0.298631336)
    o1 = o1 * _fix(2.053119869)
    o2 = o2 * _fix(3.072711026)
    o3 = o3 * _fix(1.501321110)
    z1 = -z1 * _fix(0.899976223)
    z2 = -z2 * _fix(2.562915447)
    z3 = -z3 * _fix(1.961570560) + z5
    z4 = -z4 * _fix(0.390180644) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef):
    """coef [..., 64] dequantised, natural order -> uint8 [..., 8, 8]."""
    b = coef.astype(np.int64).reshape(coef.shape[:-1] + (8, 8))
    ws = _idct_1d(b.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # columns first
    x = _idct_1d(ws, 18) & 1023
    s = (x ^ 512) - 512                                             # the table index as a signed 10-bit number
    return np.clip(s + 128, 0, 255).astype(np.uint8)


def _h2v1(c, w):
    c = c.astype(np.int64)
    if c.shape[1] <= 2:
        return np.repeat(c, 2, axis=1)[:, :w]
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out[:, :w]


def _h2v2(c, h, w):
    c = c.astype(np.int64)
    if c.shape[1] <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]
    up = np.concatenate([c[:1], c[:-1]], axis=0)
    down = np.concatenate([c[1:], c[-1:]], axis=0)
    s = np.empty((2 * c.shape[0], c.shape[1]), dtype=np.int64)
    s[0::2] = 3 * c + up
    s[1::2] = 3 * c + down
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    out[:, 0] = (4 * s[:, 0] + 8) >> 4
    out[:, -1] = (4 * s[:, -1] + 7) >> 4
    return out[:h, :w]


def decode_status(blob, rgb=False, parsed=None):
    """(uint8 [h, w, 3] or None, status)."""
    p = parse(blob) if parsed is None else parsed
    if p.status != OK:
        return None, p.status
    samp = [(p.hs, p.vs)] + [(1, 1)] * (p.ncomp - 1)
    coef = [np.zeros((p.mcu_h * sv, p.mcu_w * sh, 64), dtype=np.int64) for sh, sv in samp]
    status = OK
    for mcu0, nmcu, off, length in p.items:
        status = max(status, _decode_item(bytes(blob)[off:off + length], p, mcu0, nmcu, coef))
    planes = [idct_blocks(c).swapaxes(1, 2).reshape(c.shape[0] * 8, c.shape[1] * 8) for c in coef]
    h, w = p.h, p.w
    y = planes[0][:h, :w].astype(np.int64)
    if p.ncomp == 1:
        out = np.stack([y, y, y], axis=-1)
    else:
        ch, cw = -(-h * 1 // p.vs), -(-w * 1 // p.hs)
        chroma = []
        for c in planes[1:]:
            c = c[:ch, :cw]
            chroma.append(c.astype(np.int64) if p.hs == 1 else _h2v1(c, w) if p.vs == 1 else _h2v2(c, h, w))
        cb, cr = chroma[0] - 128, chroma[1] - 128
        r = y + ((91881 * cr + 32768) >> 16)
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
        out = np.stack([r, g, b] if rgb else [b, g, r], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8), status


def decode(blob, rgb=False):
    out, status = decode_status(blob, rgb)
    if status != OK:
        raise ValueError("not a decodable baseline JPEG (status %d)" % status)
    return out
