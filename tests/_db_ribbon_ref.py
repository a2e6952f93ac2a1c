"""`mr_db_ribbons` (csrc/db_post.hip) restated in pure Python, operation for operation after the rule written out in
include/megreader_hip.h.  TEST INFRASTRUCTURE ONLY.

Python floats are float64 and never fused, which is what `#pragma clang fp contract(off)` makes of the kernel; the slab sums are
Python integers (exact, as the kernel's 64-bit ones).  `ribbon_of` is the rule for one candidate, `db_ribbons` the entry point
behind `_db_boxes_ref.db_boxes`: the compacted order, the zeros behind the used knots and behind the last box."""
import math

import numpy as np

import _db_boxes_ref as B

MAX_SLABS, MAX_KNOTS = 16, 18
RIBBON, SHORT, EMPTY, STEEP, FOLDED = 0, 1, 2, 3, 4


def _len(x, y):
    return math.sqrt(x * x + y * y)


def axis_of(cand):
    """Step 1: (o, e, L) of the ordered rectangle `cand` [[x, y] * 4]."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(float(x), float(y)) for x, y in cand]
    ax, ay, bx, by = x1 - x0, y1 - y0, x3 - x0, y3 - y0
    a, b = _len(ax, ay), _len(bx, by)
    if float(max(int(b), 1)) > 1.5 * float(max(int(a), 1)):
        return (x1, y1), ((x2 - x1) / b, (y2 - y1) / b), b
    if a == 0.0:
        return (x0, y0), (float('nan'), float('nan')), a
    return (x0, y0), (ax / a, ay / a), a


def outline(top, bot):
    return list(top) + list(bot)[::-1]


def unclip_distance(top, bot, ratio):
    """Step 7's d: shoelace area and perimeter of T_0 .. T_last, B_last .. B_0, summed in that order."""
    q = outline(top, bot)
    a2, per = 0.0, 0.0
    for i in range(len(q)):
        (px, py), (qx, qy) = q[i], q[(i + 1) % len(q)]
        a2 = a2 + (px * qy - qx * py)
        dx, dy = qx - px, qy - py
        per = per + math.sqrt(dx * dx + dy * dy)
    return abs(a2) / 2.0 * ratio / per


def cells_convex(top, bot):
    """Step 8: every cell (T_i, T_i+1, B_i+1, B_i) strictly convex, y down."""
    for i in range(len(top) - 1):
        q = [top[i], top[i + 1], bot[i + 1], bot[i]]
        for j in range(4):
            (ax, ay), (bx, by), (cx, cy) = q[j], q[(j + 1) % 4], q[(j + 2) % 4]
            if not (bx - ax) * (cy - by) - (by - ay) * (cx - bx) > 0.0:
                return False
    return True


def rulings(c, t, h):
    top = [(cx - (-ty) * hh, cy - tx * hh) for (cx, cy), (tx, ty), hh in zip(c, t, h)]
    bot = [(cx + (-ty) * hh, cy + tx * hh) for (cx, cy), (tx, ty), hh in zip(c, t, h)]
    return top, bot


def finish(c, t, h, ratio):
    """Steps 7 and 8 on centres, unit tangents and half thicknesses of the knots: (why, top, bot, d)."""
    top, bot = rulings(c, t, h)
    d = unclip_distance(top, bot, ratio)
    c = list(c)
    c[0] = (c[0][0] - d * t[0][0], c[0][1] - d * t[0][1])
    c[-1] = (c[-1][0] + d * t[-1][0], c[-1][1] + d * t[-1][1])
    top, bot = rulings(c, t, [hh + d for hh in h])
    return (RIBBON if cells_convex(top, bot) else FOLDED), top, bot, d


def ribbon_of(xs, ys, cand, S=8, ratio=1.5):
    """The rule for one candidate: xs, ys the integer pixel coordinates of its component, cand its ordered rectangle before unclip.
    Returns {'why', 'knots', 'top', 'bot' (lists of (x, y) in MAP coordinates, empty without a ribbon), 'd', 'sums', 'centres'}."""
    out = {'why': SHORT, 'knots': 0, 'top': [], 'bot': [], 'd': None, 'sums': None, 'centres': None}
    (ox, oy), (ex, ey), L = axis_of(cand)
    if not L > 0.0:
        return out
    P = len(xs)
    tbar = float(P) / (L + 1.0)
    Se = min(int(S), int((L + 1.0) / max(4.0, tbar)))
    if Se < 3:
        return out
    sw = (L + 1.0) / float(Se)
    sums = [[0] * 6 for _ in range(Se)]
    for x, y in zip((int(v) for v in xs), (int(v) for v in ys)):
        u = (float(x) - ox) * ex + (float(y) - oy) * ey
        f = math.floor((u + 0.5) / sw)
        j = Se - 1 if f >= Se - 1 else (int(f) if f > 0.0 else 0)
        s = sums[j]
        s[0] += 1; s[1] += x; s[2] += y; s[3] += x * x; s[4] += x * y; s[5] += y * y
    out['sums'] = sums
    if any(s[0] == 0 for s in sums):
        out['why'] = EMPTY
        return out
    m, cov = [], []
    for s in sums:
        n = float(s[0])
        mx, my = float(s[1]) / n, float(s[2]) / n
        m.append((mx, my))
        cov.append((float(s[3]) / n - mx * mx, float(s[4]) / n - mx * my, float(s[5]) / n - my * my))
    l = Se - 1
    t, cos, half = [], [], []
    for j in range(Se):
        if j == 0:
            tx = -3.0 * m[0][0] + 4.0 * m[1][0] - m[2][0]
            ty = -3.0 * m[0][1] + 4.0 * m[1][1] - m[2][1]
        elif j == l:
            tx = 3.0 * m[l][0] - 4.0 * m[l - 1][0] + m[l - 2][0]
            ty = 3.0 * m[l][1] - 4.0 * m[l - 1][1] + m[l - 2][1]
        else:
            tx, ty = m[j + 1][0] - m[j - 1][0], m[j + 1][1] - m[j - 1][1]
        ln = math.sqrt(tx * tx + ty * ty)
        if ln == 0.0:
            tx = ty = float('nan')
        else:
            tx, ty = tx / ln, ty / ln
        t.append((tx, ty))
        cos.append(tx * ex + ty * ey)
        nx, ny = -ty, tx
        var = nx * nx * cov[j][0] + 2.0 * nx * ny * cov[j][1] + ny * ny * cov[j][2]
        half.append((math.sqrt(12.0 * max(var, 0.0) + 1.0) - 1.0) / 2.0 if var == var else var)
    if not all(c > 0.25 for c in cos):
        out['why'] = STEEP
        return out
    kn = Se + 2
    c, kt, kh = [], [], []
    for i in range(kn):
        j = min(max(i - 1, 0), l)
        jh = min(max(j, 1), l - 1)
        cx, cy = m[j]
        if i == 0:
            back = (sw / 2.0) / cos[0]
            cx, cy = cx - t[j][0] * back, cy - t[j][1] * back
        elif i == kn - 1:
            on = (sw / 2.0) / cos[l]
            cx, cy = cx + t[j][0] * on, cy + t[j][1] * on
        c.append((cx, cy))
        kt.append(t[j])
        kh.append(half[jh])
    why, top, bot, d = finish(c, kt, kh, ratio)
    out.update(why=why, d=d, centres=c)
    if why == RIBBON:
        out.update(knots=kn, top=top, bot=bot)
    return out


def candidate(mask):
    """(xs, ys, ordered rectangle before unclip) of the raster-first component of a bool mask, as mr_db_boxes sees it."""
    root, roots = B.label_components(mask)
    ys, xs = np.nonzero(root == roots[0])
    box, _ = B.mini_box(B.hull_from_extremes(B.row_extremes(root, roots[0])))
    return xs, ys, box


# ---- painted shapes (bool [H, W]) -----------------------------------------------------------------------------------------------

def paint_bar(H, W, centre, length, thick, degrees):
    """A bar of `length` x `thick` pixels (odd numbers: the point extents are length - 1 and thick - 1) about `centre`."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    u = (xx - centre[0]) * c + (yy - centre[1]) * s
    v = -(xx - centre[0]) * s + (yy - centre[1]) * c
    return (np.abs(u) <= (length - 1) / 2.0 + 1e-9) & (np.abs(v) <= (thick - 1) / 2.0 + 1e-9)


def paint_sector(H, W, centre, R, thick, span_degrees, mid_degrees=-90.0):
    """An annular sector: |r - R| <= thick / 2 within span / 2 of the direction `mid_degrees` (-90: an arch, y down)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xx - centre[0], yy - centre[1]
    r = np.sqrt(dx * dx + dy * dy)
    ang = np.degrees(np.arctan2(dy, dx)) - mid_degrees
    ang = (ang + 180.0) % 360.0 - 180.0
    return (np.abs(r - R) <= thick / 2.0) & (np.abs(ang) <= span_degrees / 2.0)


def paint_sine(H, W, y0, amplitude, period, thick=14, x0=60, x1=260):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (np.abs(yy - (y0 + amplitude * np.sin(2.0 * math.pi * xx / period))) <= thick / 2.0) & (xx >= x0) & (xx <= x1)


def db_ribbons(seg_mask, dest, boxes_out, S=8, ratio=1.5):
    """The outputs of mr_db_ribbons behind `_db_boxes_ref.db_boxes(prob, seg_mask, dest, K)` (`boxes_out`: what it returned):
    ribbons f64 [N, K, 18, 2, 2], knots i32 [N, K], why i32 [N, K], in the compacted order of `boxes`."""
    N, H, W = seg_mask.shape
    K = boxes_out['status'].shape[1]
    out = {'ribbons': np.zeros((N, K, MAX_KNOTS, 2, 2)), 'knots': np.zeros((N, K), np.int32), 'why': np.zeros((N, K), np.int32)}
    for n in range(N):
        root, roots = B.label_components(seg_mask[n])
        dw, dh = float(dest[n][0]), float(dest[n][1])
        row = 0
        for k, r in enumerate(roots[:K]):
            if boxes_out['status'][n, k] != B.KEPT:
                continue
            ys, xs = np.nonzero(root == r)
            got = ribbon_of(xs, ys, boxes_out['cand'][n, k].tolist(), S, ratio)
            out['why'][n, row], out['knots'][n, row] = got['why'], got['knots']
            for i in range(got['knots']):
                (tx, ty), (bx, by) = got['top'][i], got['bot'][i]
                out['ribbons'][n, row, i] = ((tx / float(W) * dw, ty / float(H) * dh), (bx / float(W) * dw, by / float(H) * dh))
            row += 1
    return out
