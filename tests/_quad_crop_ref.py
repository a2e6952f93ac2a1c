"""numpy restatements for the quad crops (megreader_amd/data/quad_crop.py, megreader_amd/csrc/image_sample.hip).

`quad_crop_ref` is `quad_crop_kernel` in the kernel's own operation order: float64 coordinates with every product and sum
rounded on its own (numpy never contracts), two correctly rounded float64 divisions, float32 blends, the normalisation of
`mr_resize_normalize`.  Every operation is an IEEE basic operation, so the device result must equal it bit for bit.

`two_pass_ref` restates what `ImageCropper.crop` (data/crop_file_dataset.py:105-124) does with the SAME plan: a bilinear
warpPerspective of the uint8 photo into the cw x ch crop frame (float weights, BORDER_CONSTANT 0, result rounded to uint8
as cv2 stores it), `ensure_horizontal`, then oracle/pipeline.py's cv2.resize + normalisation.  It is for REPORTING how far
the fused pass is from the two-pass chain, not a parity bar: cv2 cannot be run beside this code."""
import numpy as np

from oracle.pipeline import process_sample

RGB_MEAN = (122.67891434, 116.66876762, 104.00698793)


def zero_pixel(mean=RGB_MEAN):
    """The normalised value of a zero pixel, per channel."""
    return (np.float64(0) - np.array(mean, dtype=np.float64)).astype(np.float32) / np.float32(255)


def _bilinear_zero_border(photo, x, y, ok):
    """float32 [..., 3]: the kernel's taps and blend at float64 (x, y) where `ok`, 0 elsewhere; taps outside the photo are 0."""
    h, w = photo.shape[:2]
    near = ok & (x > -1.0) & (x < w) & (y > -1.0) & (y < h)         # otherwise all four taps are outside the photo
    xs, ys = np.where(near, x, 0.0), np.where(near, y, 0.0)
    xf, yf = np.floor(xs), np.floor(ys)
    fx, fy = (xs - xf).astype(np.float32)[..., None], (ys - yf).astype(np.float32)[..., None]
    ix, iy = xf.astype(np.int64), yf.astype(np.int64)

    def tap(dx, dy):
        xx, yy = ix + dx, iy + dy
        inside = near & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        p = photo[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float32)
        return np.where(inside[..., None], p, np.float32(0))

    p00, p01, p10, p11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
    gx, gy = np.float32(1) - fx, np.float32(1) - fy
    top = p00 * gx + p01 * fx
    bot = p10 * gx + p11 * fx
    value = np.where(near[..., None], top * gy + bot * fy, np.float32(0))
    assert value.dtype == np.float32
    return value


def source_points(plan):
    """(x, y, D, valid) of every canvas pixel of a plan, float64 [H, W]: the kernel's coordinate arithmetic."""
    H, W = plan.canvas
    h = [np.float64(t) for t in plan.h9]
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    cx = np.minimum(np.maximum((u + 0.5) * np.float64(plan.sx) - 0.5, 0.0), np.float64(plan.cu1))
    cy = np.minimum(np.maximum((v + 0.5) * np.float64(plan.sy) - 0.5, 0.0), np.float64(plan.cv1))
    X = h[0] * cx + h[1] * cy + h[2]
    Y = h[3] * cx + h[4] * cy + h[5]
    D = h[6] * cx + h[7] * cy + h[8]
    with np.errstate(divide='ignore', invalid='ignore'):
        x, y = X / D, Y / D
    valid = np.broadcast_to(u < plan.dst_w, (H, W))
    return x, y, np.broadcast_to(D, (H, W)), valid


def quad_crop_ref(photo, plan, mean=RGB_MEAN):
    """photo: uint8 [h, w, 3]; plan: a CropPlan.  Returns f32 [3, H, W]: what mr_quad_crop writes for this crop."""
    x, y, D, valid = source_points(plan)
    ok = valid & (D > 0.0) & np.isfinite(x) & np.isfinite(y)
    value = _bilinear_zero_border(photo, x, y, ok)
    image = (value.astype(np.float64) - np.array(mean, dtype=np.float64)).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(image.transpose(2, 0, 1))


def two_pass_ref(photo, plan, mode):
    """`ImageCropper.crop` with this plan's frame: warp into cw x ch, rotate if tall, resize, normalise.  f32 [3, H, W]."""
    m = np.asarray(plan.crop_map, dtype=np.float64)
    xc = np.arange(plan.cw, dtype=np.float64)[None, :]
    yc = np.arange(plan.ch, dtype=np.float64)[:, None]
    X = m[0, 0] * xc + m[0, 1] * yc + m[0, 2]
    Y = m[1, 0] * xc + m[1, 1] * yc + m[1, 2]
    D = m[2, 0] * xc + m[2, 1] * yc + m[2, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        x, y = X / D, Y / D
    ok = np.broadcast_to(D > 0.0, x.shape) & np.isfinite(x) & np.isfinite(y)
    crop = np.clip(np.rint(_bilinear_zero_border(photo, x, y, ok)), 0, 255).astype(np.uint8)      # warpPerspective of uint8
    if crop.shape[0] > crop.shape[1] * 1.5:                                                          # ensure_horizontal
        crop = np.flip(np.swapaxes(crop, 0, 1), 0)
    assert crop.shape[:2] == tuple(plan.frame)
    return process_sample(np.ascontiguousarray(crop), '', tuple(plan.canvas), mode)[0]


# ---- the device call (GPU tests) ----------------------------------------------------------------------------------------------

def device_crop(photos, plans, canvas, pad=0, mean=RGB_MEAN, images=None):
    """`mr_quad_crop` called directly.  photos: uint8 [h, w, 3] arrays packed at 16-byte aligned offsets with `pad` extra bytes
    per row; plans: [(photo index, CropPlan)].  Every byte that belongs to no photo is 255, so a read outside a photo shows in
    the result; the output is pre-filled with NaN.  `images` overrides the `image` index written into each descriptor.
    Returns f32 [M, 3, H, W] on the host."""
    import torch

    from megreader_amd._lib import call, ptr
    from megreader_amd.data.quad_crop import CropDesc, CropImage
    H, W = canvas
    table = (CropImage * max(len(photos), 1))()
    off = 16
    for i, im in enumerate(photos):
        table[i].offset, table[i].pitch, table[i].h, table[i].w = off, 3 * im.shape[1] + pad, im.shape[0], im.shape[1]
        off += (im.shape[0] * table[i].pitch + 15) // 16 * 16 + 16
    host = np.full(off, 255, dtype=np.uint8)
    for i, im in enumerate(photos):
        rows = host[table[i].offset:table[i].offset + im.shape[0] * table[i].pitch].reshape(im.shape[0], table[i].pitch)
        rows[:, :3 * im.shape[1]] = im.reshape(im.shape[0], -1)
    descs = (CropDesc * max(len(plans), 1))()
    for m, (i, plan) in enumerate(plans):
        plan.fill(descs[m], i if images is None else images[m])
    dev = torch.device("cuda")
    d_src = torch.from_numpy(host).to(dev)
    d_table = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    out = torch.full((len(plans), 3, H, W), float('nan'), dtype=torch.float32, device=dev)
    call("mr_quad_crop", ptr(d_src), ptr(d_table), len(photos), ptr(d_desc), len(plans), H, W, mean[0], mean[1], mean[2],
         ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()
