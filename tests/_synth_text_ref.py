"""The rule of `mr_synth_render` as include/megreader_hip.h writes it, restated in numpy: float32 and float64 exactly where the
header names them, every product and sum rounded on its own, one canvas at a time.  It follows the header, not the kernel: no
tiles, no culling, the virtual line image is built whole and the blur runs over an edge-padded copy of the composite.

The tables are the structured arrays of megreader_amd.data.synth_text (ITEM_DTYPE, CANVAS_DTYPE: the C structs) and the fonts are
`GlyphAtlas` objects; `run_kernel` packs the same tables for the device and calls the entry point directly.
"""
import numpy as np

F32 = np.float32
MAX_GLYPHS, MAX_ITEMS, MAX_GLYPH_W = 32, 32, 65536


def line_image(atlas, glyphs):
    """uint8 [gh, Lw]: the advance boxes of the valid glyphs side by side."""
    cols = []
    aw = atlas.coverage.shape[1]
    for g in glyphs:
        g = int(g)
        if not 0 <= g < len(atlas.w):
            continue
        x0, w = int(atlas.x0[g]), int(atlas.w[g])
        if x0 >= 0 and 0 < w <= MAX_GLYPH_W and x0 + w <= aw:
            cols.append(atlas.coverage[:, x0:x0 + w])
    if not cols:
        return np.zeros((atlas.coverage.shape[0], 0), dtype=np.uint8)
    return np.concatenate(cols, axis=1)


def coverage(L, ok, u, v):
    """cov(u, v) over arrays u, v (float64) where `ok` (D > 0): float32."""
    gh, lw = L.shape
    with np.errstate(invalid='ignore'):
        inside = ok & (u > -1.0) & (u < float(lw)) & (v > -1.0) & (v < float(gh))
    us, vs = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
    uf, vf = np.floor(us), np.floor(vs)
    fu, fv = (us - uf).astype(F32), (vs - vf).astype(F32)
    iu, iv = uf.astype(np.int64), vf.astype(np.int64)

    def tap(ix, iy):
        hit = (ix >= 0) & (ix < lw) & (iy >= 0) & (iy < gh)
        if lw == 0:
            return np.zeros(ix.shape, dtype=F32)
        return np.where(hit, L[np.clip(iy, 0, gh - 1), np.clip(ix, 0, lw - 1)], 0).astype(F32)
    p00, p01, p10, p11 = tap(iu, iv), tap(iu + 1, iv), tap(iu, iv + 1), tap(iu + 1, iv + 1)
    gu, gv = F32(1) - fu, F32(1) - fv
    top = p00 * gu + p01 * fu
    bot = p10 * gu + p11 * fu
    val = top * gv + bot * fv
    return np.where(inside, val / F32(255), F32(0)).astype(F32)


def composite(canvas, index, items, atlases, H, W, photo=None):
    """comp [H, W, 3] float32 of one canvas record; `index`: the canvas's position in its call (items name it)."""
    xs = np.arange(W, dtype=F32)[None, :] + F32(0.5)
    ys = np.arange(H, dtype=F32)[:, None] + F32(0.5)
    if int(canvas["photo"]) != 0:
        col = photo[:H, :W, :].astype(F32)
    else:
        t = F32(canvas["gx"]) * xs + F32(canvas["gy"]) * ys + F32(canvas["g0"])
        t = np.fmin(np.fmax(t, F32(0)), F32(1))
        bg0, bg1 = canvas["bg0"].astype(F32), canvas["bg1"].astype(F32)
        col = np.stack([bg0[c] + (bg1[c] - bg0[c]) * t for c in range(3)], axis=-1).astype(F32)
    px = np.arange(W, dtype=np.float64)[None, :] + 0.5
    py = np.arange(H, dtype=np.float64)[:, None] + 0.5
    first, cnt = int(canvas["first_item"]), int(canvas["n_items"])
    for k in range(first, first + min(max(cnt, 0), MAX_ITEMS)):
        if not 0 <= k < len(items):
            continue
        it = items[k]
        if int(it["canvas"]) != index or not 0 <= int(it["font"]) < len(atlases) \
                or not 0 <= int(it["n_glyphs"]) <= MAX_GLYPHS:
            continue
        L = line_image(atlases[int(it["font"])], it["glyph"][:int(it["n_glyphs"])])
        x0, x1 = max(int(it["x0"]), 0), min(int(it["x1"]), W)
        y0, y1 = max(int(it["y0"]), 0), min(int(it["y1"]), H)
        if x0 >= x1 or y0 >= y1:
            continue
        h = it["h"].astype(np.float64)
        bx, by = px[:, x0:x1], py[y0:y1, :]
        with np.errstate(all='ignore'):
            X = h[0] * bx + h[1] * by + h[2]
            Y = h[3] * bx + h[4] * by + h[5]
            D = h[6] * bx + h[7] * by + h[8]
            u, v = X / D - 0.5, Y / D - 0.5
            ok = D > 0.0
            a = coverage(L, ok, u, v)
            sub = col[y0:y1, x0:x1, :]
            if F32(it["shadow_alpha"]) != F32(0):
                s = coverage(L, ok, u - float(it["shadow_dx"]), v - float(it["shadow_dy"]))
                ts = s * F32(it["shadow_alpha"])
                sub = np.stack([sub[..., c] * (F32(1) - ts) + F32(it["shadow"][c]) * ts for c in range(3)], axis=-1)
            sub = np.stack([sub[..., c] * (F32(1) - a) + F32(it["fg"][c]) * a for c in range(3)], axis=-1)
        col[y0:y1, x0:x1, :] = sub
    return col


def lowbias32(r):
    """uint64 arrays holding uint32 values."""
    m = np.uint64(0xFFFFFFFF)
    r = r ^ (r >> np.uint64(16))
    r = (r * np.uint64(0x7FEB352D)) & m
    r = r ^ (r >> np.uint64(15))
    r = (r * np.uint64(0x846CA68B)) & m
    r = r ^ (r >> np.uint64(16))
    return r


def render_canvas(canvas, index, items, atlases, H, W, mean, photo=None):
    """(uint8 [H, W, 3], float32 [3, H, W]) of one canvas."""
    col = composite(canvas, index, items, atlases, H, W, photo)
    if int(canvas["blur"]) != 0:
        k = [F32(canvas["w2"]), F32(canvas["w1"]), F32(canvas["w0"]), F32(canvas["w1"]), F32(canvas["w2"])]
        P = np.pad(col, ((2, 2), (2, 2), (0, 0)), mode='edge')              # comp at the clamped coordinates
        row = k[0] * P[:, 0:W] + k[1] * P[:, 1:W + 1] + k[2] * P[:, 2:W + 2] + k[3] * P[:, 3:W + 3] + k[4] * P[:, 4:W + 4]
        col = k[0] * row[0:H] + k[1] * row[1:H + 1] + k[2] * row[2:H + 2] + k[3] * row[3:H + 3] + k[4] * row[4:H + 4]
        assert col.dtype == F32
    m = np.uint64(0xFFFFFFFF)
    yy, xx, cc = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), np.arange(3, dtype=np.uint64),
                             indexing='ij')
    kk = ((yy * np.uint64(W) + xx) * np.uint64(3) + cc) & m
    seed = np.uint64(int(canvas["seed"]) & 0xFFFFFFFF)
    r = lowbias32((seed + ((kk * np.uint64(0x9E3779B9)) & m)) & m)
    unit = (r >> np.uint64(8)).astype(F32) * F32(2.0 ** -24) - F32(0.5)
    col = col + F32(canvas["noise_amp"]) * unit
    q = np.fmin(np.fmax(np.floor(col + F32(0.5)), F32(0)), F32(255)).astype(F32)
    f32 = np.stack([(q[..., c].astype(np.float64) - float(mean[c])).astype(F32) / F32(255) for c in range(3)], axis=0)
    return q.astype(np.uint8), f32


def render(canvases, items, atlases, H, W, mean, photos=None):
    """(uint8 [N, H, W, 3], float32 [N, 3, H, W]); photos: {canvas index: uint8 [h, w, 3]}."""
    out = [render_canvas(canvases[n], n, items, atlases, H, W, mean, (photos or {}).get(n)) for n in range(len(canvases))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


GUARD = 64          # guard bytes in front of and behind each output
GUARD_BYTE = 0xA5


def pack_tables(atlases, items, canvases, photos=None, pitches=None):
    """One uint8 numpy buffer [atlases | glyph pairs | fonts | photos | items | canvases] with every section 16-byte aligned, the
    canvases' photo fields filled in, and the offsets (pairs, fonts, items, canvases, n_pairs).  pitches: atlas row pitches."""
    from megreader_amd.data.synth_text import FONT_DTYPE
    from megreader_amd.data.staging import Sections
    photos = photos or {}
    canvases = canvases.copy()
    pitches = pitches or [a.coverage.shape[1] for a in atlases]
    cover = []
    for a, p in zip(atlases, pitches):
        c = np.full((a.coverage.shape[0], p), 0xEE, dtype=np.uint8)        # what lies beyond aw must never be read
        c[:, :a.coverage.shape[1]] = a.coverage
        cover.append(c)
    pairs = np.concatenate([np.stack([a.x0, a.w], axis=1) for a in atlases]).astype(np.int32)
    fonts = np.zeros(len(atlases), dtype=FONT_DTYPE)
    order = sorted(photos)
    lay = Sections(cover + [pairs, fonts] + [np.ascontiguousarray(photos[n]) for n in order]
                   + [items if len(items) else 16, canvases if len(canvases) else 16], pad_end=True)
    first = 0
    for f, (a, p) in enumerate(zip(atlases, pitches)):
        fonts["atlas_off"][f], fonts["pitch"][f] = lay.offsets[f], p
        fonts["gh"][f], fonts["aw"][f] = a.coverage.shape
        fonts["glyph_first"][f], fonts["n_classes"][f] = first, len(a.w)
        first += len(a.w)
    F = len(atlases)
    for n, off in zip(order, lay.offsets[F + 2:]):
        canvases["photo"][n], canvases["photo_off"][n], canvases["photo_pitch"][n] = 1, off, photos[n].shape[1] * 3
    buf = np.zeros(lay.total, dtype=np.uint8)
    for s, off in zip(lay.sections, lay.offsets):
        if not isinstance(s, int):
            buf[off:off + s.nbytes] = np.frombuffer(s.tobytes(), dtype=np.uint8)
    return buf, dict(pairs=lay.offsets[F], fonts=lay.offsets[F + 1], items=lay.offsets[-2], canvases=lay.offsets[-1],
                     n_pairs=first)


def kernel_args(base, off, F, I, N, H, W, mean, out_u8, out_f32):
    """The arguments of mr_synth_render (without the stream) for tables packed by `pack_tables` at address `base`."""
    return (base, base + off["fonts"], F, base + off["pairs"], off["n_pairs"], base + off["items"], I, base + off["canvases"],
            N, H, W, mean[0], mean[1], mean[2], out_u8, out_f32)


def run_kernel(atlases, items, canvases, H, W, mean, photos=None, u8=True, f32=True, pitches=None, device="cuda"):
    """`mr_synth_render` called directly on tables packed by `pack_tables`.  Both outputs lie between guard bytes, which are
    checked here.  Returns (uint8 [N, H, W, 3] or None, float32 [N, 3, H, W] or None) as numpy arrays."""
    import torch
    from megreader_amd._lib import call, ptr
    buf, off = pack_tables(atlases, items, canvases, photos, pitches)
    d = torch.from_numpy(buf).to(device)
    N = len(canvases)
    outs = []
    for want, nbytes in ((u8, N * H * W * 3), (f32, N * H * W * 3 * 4)):
        outs.append(torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device) if want else None)
    call("mr_synth_render", *kernel_args(d.data_ptr(), off, len(atlases), len(items), N, H, W, mean,
                                         ptr(outs[0]) + GUARD if u8 else 0, ptr(outs[1]) + GUARD if f32 else 0))
    torch.cuda.synchronize()
    res = []
    for o in outs:
        if o is None:
            res.append(None)
            continue
        o = o.cpu().numpy()
        assert (o[:GUARD] == GUARD_BYTE).all() and (o[-GUARD:] == GUARD_BYTE).all(), "guard bytes around an output were written"
        res.append(o[GUARD:-GUARD])
    return (res[0].reshape(N, H, W, 3) if u8 else None,
            res[1].view(np.float32).reshape(N, 3, H, W) if f32 else None)
