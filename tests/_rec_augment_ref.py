"""The rule of `mr_rec_augment` as include/megreader_hip.h writes it, restated in numpy: float32 and float64 exactly where the
header names them, every product and sum rounded on its own (numpy never contracts), one descriptor at a time.  It follows the
header, not the kernel: no tiles, the blur runs over an edge-padded copy of comp over the valid columns.

A descriptor is one record of megreader_amd.data.recognition_augment.AUG_DTYPE (the C struct); `run_kernel` packs photos and tables
for the device and calls the entry point directly, with dst between guard bytes and pre-filled with NaN bits.
"""
import numpy as np

from _quad_crop_ref import RGB_MEAN, _bilinear_zero_border, zero_pixel
from _synth_text_ref import lowbias32

F32 = np.float32
MAX_ERASE = 4
NAN_BITS = 0x7FC00ABC          # what dst holds before the call: a NaN with a payload


def comp_ref(d, photo, H, W):
    """comp over the valid columns: float32 [H, Wv, 3] (Wv >= 1)."""
    wv = min(max(int(d["dst_w"]), 0), W)
    q = max(int(d["quant"]), 1)
    u = np.arange(wv, dtype=np.int64)[None, :]
    v = np.arange(H, dtype=np.int64)[:, None]
    bu, bv = (u // q) * q, (v // q) * q
    half = 0.5 * np.float64(q)
    U = bu.astype(np.float64) + half
    V = bv.astype(np.float64) + half
    dx, dy = d["dx"].astype(np.float64), d["dy"].astype(np.float64)
    with np.errstate(all='ignore'):
        t = U * 8.0 / np.float64(wv)
        j = np.fmin(np.fmax(np.floor(t), 0.0), 7.0).astype(np.int64)
        f = t - j.astype(np.float64)
        U1 = U + (dx[j] + (dx[j + 1] - dx[j]) * f)
        V1 = V + (dy[j] + (dy[j + 1] - dy[j]) * f)
        cx = U1 * np.float64(d["sx"]) - 0.5
        cy = V1 * np.float64(d["sy"]) - 0.5
        g = [np.float64(x) for x in d["g"]]
        X = g[0] * cx + g[1] * cy + g[2]
        Y = g[3] * cx + g[4] * cy + g[5]
        D = g[6] * cx + g[7] * cy + g[8]
        px = np.fmin(np.fmax(X / D, np.float64(d["cu0"])), np.float64(d["cu1"]))
        py = np.fmin(np.fmax(Y / D, np.float64(d["cv0"])), np.float64(d["cv1"]))
        h = [np.float64(x) for x in d["h"]]
        X2 = h[0] * px + h[1] * py + h[2]
        Y2 = h[3] * px + h[4] * py + h[5]
        D2 = h[6] * px + h[7] * py + h[8]
        x, y = X2 / D2, Y2 / D2
        ok = (D > 0.0) & (D2 > 0.0) & np.isfinite(x) & np.isfinite(y)
        ok, x, y = (np.broadcast_to(a, (H, wv)) for a in (ok, x, y))
        val = _bilinear_zero_border(photo, x, y, ok)
        m, b = d["m"].astype(F32), d["b"].astype(F32)
        col = np.stack([np.fmin(np.fmax(m[3 * c] * val[..., 0] + m[3 * c + 1] * val[..., 1] + m[3 * c + 2] * val[..., 2] + b[c],
                                        F32(0)), F32(255)) for c in range(3)], axis=-1)
    assert col.dtype == F32
    return col


def augment_ref(d, photos, H, W, mean=RGB_MEAN):
    """float32 [3, H, W]: the row descriptor `d` writes.  photos: the list the `image` index refers to."""
    zero = zero_pixel(mean)
    out = np.empty((3, H, W), dtype=F32)
    out[:] = zero[:, None, None]
    wv = min(max(int(d["dst_w"]), 0), W)
    image = int(d["image"])
    if wv < 1 or not 0 <= image < len(photos):
        return out
    col = comp_ref(d, photos[image], H, W)
    if int(d["blur"]) != 0:
        k = d["k"].astype(F32)
        P = np.pad(col, ((2, 2), (2, 2), (0, 0)), mode='edge')              # comp at the clamped coordinates
        acc = None
        with np.errstate(all='ignore'):
            for j in range(5):
                for i in range(5):
                    term = k[j * 5 + i] * P[j:j + H, i:i + wv]
                    acc = term if acc is None else acc + term
        col = acc
        assert col.dtype == F32
    col = col.copy()
    for e in range(min(max(int(d["n_erase"]), 0), MAX_ERASE)):
        x0, x1, y0, y1 = (int(t) for t in d["erase"][4 * e:4 * e + 4])
        x0, x1, y0, y1 = max(x0, 0), min(x1, wv), max(y0, 0), min(y1, H)
        if x0 < x1 and y0 < y1:
            col[y0:y1, x0:x1, :] = d["erase_col"][3 * e:3 * e + 3].astype(F32)
    mask = np.uint64(0xFFFFFFFF)
    yy, xx, cc = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(wv, dtype=np.uint64), np.arange(3, dtype=np.uint64),
                             indexing='ij')
    kk = ((yy * np.uint64(W) + xx) * np.uint64(3) + cc) & mask
    seed = np.uint64(int(d["seed"]) & 0xFFFFFFFF)
    r = lowbias32((seed + ((kk * np.uint64(0x9E3779B9)) & mask)) & mask)
    unit = (r >> np.uint64(8)).astype(F32) * F32(2.0 ** -24) - F32(0.5)
    with np.errstate(all='ignore'):
        col = col + F32(d["noise_amp"]) * unit
        col = np.fmin(np.fmax(col, F32(0)), F32(255))
    for c in range(3):
        out[c, :, :wv] = (col[..., c].astype(np.float64) - float(mean[c])).astype(F32) / F32(255)
    return out


def batch_ref(table, photos, N, H, W, mean=RGB_MEAN, before=None):
    """float32 [N, 3, H, W] as uint32 bits: `before` (default: NAN_BITS everywhere) with the rows of `table` overwritten."""
    out = np.full((N, 3, H, W), NAN_BITS, dtype=np.uint32) if before is None else before.view(np.uint32).copy()
    for d in table:
        if 0 <= int(d["row"]) < N:
            out[int(d["row"])] = augment_ref(d, photos, H, W, mean).view(np.uint32)
    return out


# ---- the device call (GPU tests) --------------------------------------------------------------------------------------------------

GUARD = 256
GUARD_BYTE = 0xA5


def pack_photos(photos, pad=0):
    """One uint8 buffer holding the photos at 16-byte aligned offsets with `pad` extra bytes per row; every byte that belongs to no
    photo is 255, so a read outside a photo shows in the result.  Returns (buffer, CropImage table)."""
    from megreader_amd.data.quad_crop import CropImage
    table = (CropImage * max(len(photos), 1))()
    off = 16
    for i, im in enumerate(photos):
        table[i].offset, table[i].pitch, table[i].h, table[i].w = off, 3 * im.shape[1] + pad, im.shape[0], im.shape[1]
        off += (im.shape[0] * table[i].pitch + 15) // 16 * 16 + 16
    host = np.full(off, 255, dtype=np.uint8)
    for i, im in enumerate(photos):
        rows = host[table[i].offset:table[i].offset + im.shape[0] * table[i].pitch].reshape(im.shape[0], table[i].pitch)
        rows[:, :3 * im.shape[1]] = im.reshape(im.shape[0], -1)
    return host, table


def run_kernel(photos, table, N, H, W, mean=RGB_MEAN, pad=0, pinned=False, n_images=None, shift=0):
    """`mr_rec_augment` called directly.  dst lies between guard bytes, which are checked here, and holds NAN_BITS before the call.
    pinned: the descriptor table stays in pinned host memory (the entry point then checks it).  shift: `src` is passed that many
    bytes behind the buffer's start and the table's offsets are smaller by as much (negative for shift > 16: a photo resident in
    another allocation).  Returns uint32 bits [N, 3, H, W]."""
    import torch
    from megreader_amd._lib import call
    host, images = pack_photos(photos, pad)
    for i in range(len(photos)):
        images[i].offset -= shift
    dev = torch.device("cuda")
    d_src = torch.from_numpy(host).to(dev)
    d_images = torch.from_numpy(np.frombuffer(bytes(images), dtype=np.uint8).copy()).to(dev)
    raw = np.frombuffer(table.tobytes(), dtype=np.uint8).copy() if len(table) else np.zeros(16, dtype=np.uint8)
    d_table = torch.from_numpy(raw).pin_memory() if pinned else torch.from_numpy(raw).to(dev)
    nbytes = N * 3 * H * W * 4
    buf = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    buf[GUARD:GUARD + nbytes].view(torch.int32).fill_(NAN_BITS)
    call("mr_rec_augment", d_src.data_ptr() + shift, d_images.data_ptr(), len(photos) if n_images is None else n_images,
         d_table.data_ptr(), len(table), N, H, W, mean[0], mean[1], mean[2], buf.data_ptr() + GUARD)
    torch.cuda.synchronize()
    o = buf.cpu().numpy()
    assert (o[:GUARD] == GUARD_BYTE).all() and (o[-GUARD:] == GUARD_BYTE).all(), "guard bytes around dst were written"
    return o[GUARD:GUARD + nbytes].view(np.uint32).reshape(N, 3, H, W)
