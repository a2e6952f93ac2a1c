"""numpy restatements of mr_tile_sample and mr_tile_stitch, made from the text of include/megreader_hip.h ("Tiled multi-scale
detection") in its operation order.  No product code is imported: the resize rule of oracle/pipeline.py (cv2's float32
INTER_LINEAR) is restated here with the scale handed in, as the kernel gets it.  float32 arrays keep every product and sum
rounded on its own, which is what the kernels promise (no fma)."""
import numpy as np

RGB_MEAN = np.array([122.67891434, 116.66876762, 104.00698793])
F32 = np.float32


def entries(table, n=None):
    """A ctypes array of structs as a list of dicts (field -> value)."""
    rows = list(table)[:n] if n is not None else list(table)
    return [{name: getattr(e, name) for name, _ in e._fields_} for e in rows]


def resize_taps(coords, src, scale):
    """Per canvas coordinate of `coords`: (s0, s1, frac f32) of cv2.resize's float32 rule along one axis of `src` pixels."""
    coords = np.asarray(coords, dtype=np.int64)
    f = ((coords.astype(np.float64) + 0.5) * np.float64(scale) - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, F32(0), f).astype(F32)
    return s, np.minimum(s + 1, src - 1), f


def resize_window(photo, hc, wc, scale_x, scale_y, xs, ys):
    """The pixels (xs x ys, all inside the canvas) of the resize of uint8 HWC `photo` to hc x wc, float32 [len(ys), len(xs), 3]."""
    h, w = photo.shape[:2]
    img = photo.astype(F32)
    xs, ys = np.asarray(xs, dtype=np.int64), np.asarray(ys, dtype=np.int64)
    if (h, w) == (hc, wc):
        return img[ys][:, xs]
    sx, sx1, fx = resize_taps(xs, w, scale_x)
    sy, sy1, fy = resize_taps(ys, h, scale_y)
    a0, a1 = (F32(1) - fx)[None, :, None], fx[None, :, None]
    b0, b1 = (F32(1) - fy)[:, None, None], fy[:, None, None]
    top = img[sy][:, sx] * a0 + img[sy][:, sx1] * a1
    bot = img[sy1][:, sx] * a0 + img[sy1][:, sx1] * a1
    return (top * b0 + bot * b1).astype(F32)


def normalized(val):
    """float32 [.., .., 3] -> the normalising store's float32 [3, .., ..]: (float)((double)val - mean) / 255.f."""
    return ((val.astype(np.float64) - RGB_MEAN).astype(F32) / F32(255)).transpose(2, 0, 1)


def whole_canvas(photo, hc, wc):
    """mr_resize_normalize of `photo` onto a whole hc x wc canvas (mode 'resize'): float32 [3, hc, wc]."""
    h, w = photo.shape[:2]
    sx, sy = 1.0 / (float(wc) / float(w)), 1.0 / (float(hc) / float(h))
    return normalized(resize_window(photo, hc, wc, sx, sy, np.arange(wc), np.arange(hc)))


def tile_sample_ref(photos, tiles, th, tw):
    """photos: uint8 HWC arrays; tiles: dicts of mr_tile_desc.  float32 [T, 3, th, tw]."""
    out = np.zeros((len(tiles), 3, th, tw), dtype=F32)
    for t, d in enumerate(tiles):
        if not 0 <= d['image'] < len(photos):
            continue
        us = np.array([u for u in range(tw) if 0 <= d['x0'] + u < d['wc']], dtype=np.int64)
        vs = np.array([v for v in range(th) if 0 <= d['y0'] + v < d['hc']], dtype=np.int64)
        if len(us) == 0 or len(vs) == 0:
            continue
        val = resize_window(photos[d['image']], d['hc'], d['wc'], d['scale_x'], d['scale_y'], d['x0'] + us, d['y0'] + vs)
        out[t][:, vs[:, None], us[None, :]] = normalized(val)
    return out


def owner(p, t, h, K):
    s = t - 2 * h
    return np.where(p < t - h, 0, np.minimum(K - 1, (p - h) // s))


def tile_value(maps, th, tw, halo, lv, x, y):
    """maps float32 [T, th, tw]; x [n], y [m] canvas coordinates of level `lv` -> float32 [m, n]."""
    ky, kx = owner(y, th, halo[0], lv['ky']), owner(x, tw, halo[1], lv['kx'])
    ly, lx = y - ky * (th - 2 * halo[0]), x - kx * (tw - 2 * halo[1])
    t = lv['first'] + ky[:, None] * lv['kx'] + kx[None, :]
    ok = (t >= 0) & (t < len(maps)) & ((ly >= 0) & (ly < th))[:, None] & ((lx >= 0) & (lx < tw))[None, :]
    tt, yy, xx = np.where(ok, t, 0), np.where(ok, ly[:, None], 0), np.where(ok, lx[None, :], 0)
    if len(maps) == 0:
        return np.zeros(t.shape, dtype=F32)
    return np.where(ok, maps[tt, yy, xx], F32(0)).astype(F32)


def level_axis(P, side, ratio):
    x = (P.astype(np.float64) + 0.5) * np.float64(ratio) - 0.5
    x = np.minimum(np.maximum(x, 0.0), np.float64(side - 1))
    xf = np.floor(x)
    i0 = xf.astype(np.int64)
    return i0, np.minimum(i0 + 1, side - 1), (x - xf).astype(F32)


def tile_stitch_ref(maps, th, tw, halo, levels, photos, fuse, out):
    """maps: float32 [T, th, tw] (bf16 maps widened); levels, photos: dicts of mr_stitch_level / mr_stitch_photo; fuse 'max' or
    'mean'; out: the packed float32 buffer, written in place where the kernel writes and returned."""
    maps = np.asarray(maps, dtype=F32).reshape(-1, th, tw)
    for ph in photos:
        hb, wb = ph['hb'], ph['wb']
        X, Y = np.arange(wb, dtype=np.int64), np.arange(hb, dtype=np.int64)
        acc = None
        for l in range(ph['levels']):
            lv = levels[ph['first_level'] + l]
            if l == ph['base']:
                val = tile_value(maps, th, tw, halo, lv, X, Y)
            else:
                ix, ix1, fx = level_axis(X, lv['wc'], lv['ratio_x'])
                iy, iy1, fy = level_axis(Y, lv['hc'], lv['ratio_y'])
                p00, p01 = tile_value(maps, th, tw, halo, lv, ix, iy), tile_value(maps, th, tw, halo, lv, ix1, iy)
                p10, p11 = tile_value(maps, th, tw, halo, lv, ix, iy1), tile_value(maps, th, tw, halo, lv, ix1, iy1)
                gx, gy = (F32(1) - fx)[None, :], (F32(1) - fy)[:, None]
                top = p00 * gx + p01 * fx[None, :]
                bot = p10 * gx + p11 * fx[None, :]
                val = (top * gy + bot * fy[:, None]).astype(F32)
            acc = val if acc is None else (np.fmax(acc, val) if fuse == 'max' else (acc + val).astype(F32))
        if fuse == 'mean':
            acc = (acc / F32(ph['levels'])).astype(F32)
        out[ph['offset']:ph['offset'] + hb * wb] = acc.reshape(-1)
    return out
