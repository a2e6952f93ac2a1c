"""numpy restatement of `mr_strip_crop` (megreader_amd/csrc/image_sample.hip, arithmetic in include/megreader_hip.h) in the
kernel's own operation order: per column the cell search, one division and four float64 blends; per pixel one division and two
blends; then the taps, the float32 blend and the normalisation of `mr_quad_crop` (tests/_quad_crop_ref.py).  Every operation is
an IEEE basic operation rounded on its own, so the device result must equal it bit for bit.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from _quad_crop_ref import RGB_MEAN, _bilinear_zero_border, zero_pixel  # noqa: F401


def source_points(plan):
    """(x, y, valid) of every canvas pixel of a StripPlan, float64 [H, W]: the kernel's coordinate arithmetic."""
    H, W = plan.canvas
    s = np.asarray(plan.s, dtype=np.float64)
    top, bot = plan.ribbon.top, plan.ribbon.bottom
    k = len(s)
    u = np.arange(W, dtype=np.float64)
    v = np.arange(H, dtype=np.float64)
    cx = np.minimum(np.maximum((u + 0.5) * np.float64(plan.sx) - 0.5, 0.0), np.float64(plan.cu1))
    cy = np.minimum(np.maximum((v + 0.5) * np.float64(plan.sy) - 0.5, 0.0), np.float64(plan.cv1))
    i = np.zeros(W, dtype=np.int64)
    for j in range(1, k - 1):                               # the last knot with s[j] <= cx, at most k - 2
        i = np.where(s[j] <= cx, j, i)
    with np.errstate(divide='ignore', invalid='ignore'):
        a = (cx - s[i]) / (s[i + 1] - s[i])
        g = 1.0 - a
        tx, ty = top[i, 0] * g + top[i + 1, 0] * a, top[i, 1] * g + top[i + 1, 1] * a
        bx, by = bot[i, 0] * g + bot[i + 1, 0] * a, bot[i, 1] * g + bot[i + 1, 1] * a
        b = (cy / np.float64(plan.hgt))[:, None]
        gb = 1.0 - b
        x = tx[None, :] * gb + bx[None, :] * b
        y = ty[None, :] * gb + by[None, :] * b
    valid = np.broadcast_to(u[None, :] < plan.dst_w, (H, W))
    return x, y, valid


def strip_crop_ref(photo, plan, mean=RGB_MEAN):
    """photo: uint8 [h, w, 3]; plan: a StripPlan.  Returns f32 [3, H, W]: what mr_strip_crop writes for this crop."""
    x, y, valid = source_points(plan)
    ok = valid & np.isfinite(x) & np.isfinite(y)
    value = _bilinear_zero_border(photo, x, y, ok)
    image = (value.astype(np.float64) - np.array(mean, dtype=np.float64)).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(image.transpose(2, 0, 1))


def device_strips(photos, plans, canvas, pad=0, mean=RGB_MEAN, images=None, resident=None, guard=64):
    """`mr_strip_crop` called directly.  photos: uint8 [h, w, 3] arrays packed at 16-byte aligned offsets with `pad` extra bytes
    per row; plans: [(photo index, StripPlan)].  Every byte that belongs to no photo is 255, so a read outside a photo shows in
    the result; the output is pre-filled with NaN and has `guard` floats in front of and behind it.  `images` overrides the
    `image` index written into each descriptor; `resident`: photo indices that are not packed but lie in front of the packed
    buffer in device memory (their table entries' offsets, relative to src, are negative).  Returns (f32 [M, 3, H, W], the guard floats) on the host."""
    import torch

    from megreader_amd._lib import call, ptr
    from megreader_amd.data.quad_crop import CropImage
    from megreader_amd.data.strip_crop import StripDesc
    H, W = canvas
    resident = set(resident or ())
    table = (CropImage * max(len(photos), 1))()
    off = 16
    for i, im in enumerate(photos):
        table[i].offset, table[i].pitch, table[i].h, table[i].w = off, 3 * im.shape[1] + pad, im.shape[0], im.shape[1]
        if i not in resident:
            off += (im.shape[0] * table[i].pitch + 15) // 16 * 16 + 16
    host = np.full(off, 255, dtype=np.uint8)
    for i, im in enumerate(photos):
        if i in resident:
            continue
        rows = host[table[i].offset:table[i].offset + im.shape[0] * table[i].pitch].reshape(im.shape[0], table[i].pitch)
        rows[:, :3 * im.shape[1]] = im.reshape(im.shape[0], -1)
    dev = torch.device("cuda")
    # resident photos lie IN FRONT of src in the same allocation, tightly packed: their offsets from src are negative
    front = sum((photos[i].size + 15) // 16 * 16 for i in resident)
    whole = torch.full((front + len(host),), 255, dtype=torch.uint8, device=dev)
    d_src = whole[front:]
    d_src.copy_(torch.from_numpy(host))
    at = 0
    for i in sorted(resident):
        whole[at:at + photos[i].size].copy_(torch.from_numpy(np.array(photos[i]).reshape(-1)))
        table[i].offset, table[i].pitch = at - front, 3 * photos[i].shape[1]
        at += (photos[i].size + 15) // 16 * 16
    descs = (StripDesc * max(len(plans), 1))()
    for m, (i, plan) in enumerate(plans):
        plan.fill(descs[m], i if images is None else images[m])
    d_table = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    M = len(plans)
    buf = torch.full((M * 3 * H * W + 2 * guard,), float('nan'), dtype=torch.float32, device=dev)
    buf[:guard] = -7.0
    buf[guard + M * 3 * H * W:] = -7.0
    out = buf[guard:guard + M * 3 * H * W].view(M, 3, H, W)
    call("mr_strip_crop", ptr(d_src), ptr(d_table), len(photos), ptr(d_desc), M, H, W, mean[0], mean[1], mean[2],
         out.data_ptr())
    torch.cuda.synchronize()
    host_buf = buf.cpu().numpy()
    return host_buf[guard:guard + M * 3 * H * W].reshape(M, 3, H, W), np.concatenate([host_buf[:guard], host_buf[-guard:]])
