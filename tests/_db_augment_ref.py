"""numpy restatement of `warp_normalize_kernel` (megreader_amd/csrc/image_sample.hip) in the kernel's own operation order:
float64 coordinates, each product and sum rounded on its own (numpy never contracts), float32 blends, the normalisation of
`mr_resize_normalize`.  Every operation is an IEEE basic operation, so the device result must equal this one bit for bit.
Beside the image it reports every tap's source index, so that tests/test_db_augment_cpu.py can check the plan's window."""
import numpy as np

from megreader_amd.data.detection_augment import DetectionAugmenter, apply_points

RGB_MEAN = (122.67891434, 116.66876762, 104.00698793)


def warp_normalize_ref(src, plan, canvas=None, window=None, mean=RGB_MEAN):
    """src: the FULL uint8 [H, W, 3] source; window (x, y, w, h): what was uploaded (default: the plan's window).
    Returns {'image': f32 [3, Hd, Wd], 'value': f32 [Hd, Wd, 3] before the normalisation, 'valid': bool [Hd, Wd],
    'taps': int64 [K, 2] the (x, y) of every tap that lies inside the image}."""
    Hd, Wd = plan.canvas if canvas is None else canvas
    H, W = src.shape[:2]
    assert (H, W) == tuple(plan.shape)
    a = [np.float64(t) for t in plan.pixels_inv]
    cu0, cu1, cv0, cv1 = (np.float64(c) for c in plan.clamp)
    vw, vh = plan.valid
    wx, wy, ww, wh = plan.window if window is None else window
    u = np.arange(Wd, dtype=np.float64)[None, :]
    v = np.arange(Hd, dtype=np.float64)[:, None]
    uc = np.minimum(np.maximum(u, cu0), cu1)
    vc = np.minimum(np.maximum(v, cv0), cv1)
    x = a[0] * uc + a[1] * vc + a[2]
    y = a[3] * uc + a[4] * vc + a[5]
    valid = (v < vh) & (u < vw)
    near = valid & (x > -1.0) & (x < W) & (y > -1.0) & (y < H)      # otherwise all four taps are outside the image
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf).astype(np.float32)[..., None], (y - yf).astype(np.float32)[..., None]
    ix, iy = np.where(near, xf, 0).astype(np.int64), np.where(near, yf, 0).astype(np.int64)
    taps = []

    def tap(dx, dy):
        xx, yy = ix + dx, iy + dy
        inside = near & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        taps.append(np.stack([xx[inside], yy[inside]], axis=1))
        read = inside & (xx >= wx) & (xx < wx + ww) & (yy >= wy) & (yy < wy + wh)
        p = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float32)
        return np.where(read[..., None], p, np.float32(0))

    p00, p01, p10, p11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
    gx, gy = np.float32(1) - fx, np.float32(1) - fy
    top = p00 * gx + p01 * fx
    bot = p10 * gx + p11 * fx
    value = np.where(near[..., None], top * gy + bot * fy, np.float32(0))
    assert value.dtype == np.float32
    image = (value.astype(np.float64) - np.array(mean, dtype=np.float64)).astype(np.float32) / np.float32(255)
    return {'image': np.ascontiguousarray(image.transpose(2, 0, 1)), 'value': value, 'valid': np.broadcast_to(valid, (Hd, Wd)),
            'taps': np.concatenate(taps, axis=0)}


def zero_pixel(mean=RGB_MEAN):
    """The normalised value of a zero pixel, per channel (the canvas outside the valid region)."""
    return (np.float64(0) - np.array(mean, dtype=np.float64)).astype(np.float32) / np.float32(255)


# ---- the image / label consistency case (tests/test_db_augment_cpu.py, tests/test_db_augment_gpu.py) -------------------------

CASE_SHAPE, CASE_CANVAS = (48, 80), (64, 96)
CASE_QUAD = np.array([[18, 12], [62, 15], [60, 36], [16, 33]], dtype=np.float64)


def middle_crop(shape, scale):
    """The middle 70 % x 75 % (width x height) of the source resized by `scale`."""
    nh, nw = max(1, int(round(shape[0] * scale))), max(1, int(round(shape[1] * scale)))
    cw, ch = int(round(0.70 * nw)), int(round(0.75 * nh))
    return (nw - cw) // 2, (nh - ch) // 2, cw, ch


def case_plans(shape=CASE_SHAPE, canvas=CASE_CANVAS, polygons=(CASE_QUAD,), ignore_tags=(False,)):
    """The seven plans: identity; flip; +10 deg; flip -10 deg at scale 0.5; 7 deg at scale 3 with the middle crop;
    flip -4 deg at scale 1.7 with the middle crop; 10 deg at scale 3 with the middle crop."""
    aug = DetectionAugmenter(size=(canvas[1], canvas[0]))
    params = [(False, 0.0, 1.0, None), (True, 0.0, 1.0, None), (False, 10.0, 1.0, None), (True, -10.0, 0.5, None),
              (False, 7.0, 3.0, middle_crop(shape, 3.0)), (True, -4.0, 1.7, middle_crop(shape, 1.7)),
              (False, 10.0, 3.0, middle_crop(shape, 3.0))]
    return [aug.plan(shape, polygons, ignore_tags, flip, angle, scale, crop) for flip, angle, scale, crop in params]


def quad_mask_image(shape=CASE_SHAPE, quad=CASE_QUAD):
    """uint8 [H, W, 3]: 255 at the integer points inside the quad, 0 outside."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    inside, _ = inside_and_distance(quad, xx, yy)
    return np.repeat((inside * 255).astype(np.uint8)[..., None], 3, axis=2)


def inside_and_distance(quad, xx, yy):
    """Even-odd inside test and the distance to the boundary of a polygon [K, 2] at the points (xx, yy), float64."""
    quad = np.asarray(quad, dtype=np.float64)
    inside = np.zeros(xx.shape, dtype=bool)
    dist = np.full(xx.shape, np.inf)
    for k in range(len(quad)):
        (x0, y0), (x1, y1) = quad[k], quad[(k + 1) % len(quad)]
        if y0 != y1:
            cross = ((y0 <= yy) != (y1 <= yy)) & (xx < x0 + (yy - y0) * (x1 - x0) / (y1 - y0))
            inside ^= cross
        ex, ey = x1 - x0, y1 - y0
        t = np.clip(((xx - x0) * ex + (yy - y0) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
        dist = np.minimum(dist, np.hypot(xx - (x0 + t * ex), yy - (y0 + t * ey)))
    return inside, dist


def transformed_quad(plan, quad=CASE_QUAD):
    return apply_points(plan.points, quad)


# ---- the device call (GPU tests) ----------------------------------------------------------------------------------------------

def device_warp(sources, plans, canvas, windows=None, pad=0, mean=RGB_MEAN):
    """`mr_warp_normalize` called directly: each plan's window (or the one given) of its full source is packed at a 16-byte
    aligned offset with `pad` extra bytes per row; every byte that is no window pixel is 255, so a read outside a window
    shows in the result; the output is pre-filled with NaN.  Returns f32 [N, 3, H, W] on the host."""
    import torch

    from megreader_amd._lib import call, ptr
    from megreader_amd.data import WarpDesc
    n = len(plans)
    Hd, Wd = canvas
    windows = [p.window for p in plans] if windows is None else windows
    descs = (WarpDesc * max(n, 1))()
    off, spans = 16, []
    for i, (plan, (x, y, w, h)) in enumerate(zip(plans, windows)):
        pitch = 3 * w + pad
        plan.fill(descs[i], off, pitch)
        descs[i].win_x, descs[i].win_y, descs[i].win_w, descs[i].win_h = x, y, w, h
        spans.append((off, pitch))
        off += (h * pitch + 15) // 16 * 16 + 16
    host = np.full(off, 255, dtype=np.uint8)
    for src, (x, y, w, h), (o, pitch) in zip(sources, windows, spans):
        rows = host[o:o + h * pitch].reshape(h, pitch) if h else host[o:o].reshape(0, pitch)
        rows[:, :3 * w] = src[y:y + h, x:x + w].reshape(h, 3 * w)
    dev = torch.device("cuda")
    d_src = torch.from_numpy(host).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(dev)
    out = torch.full((n, 3, Hd, Wd), float('nan'), dtype=torch.float32, device=dev)
    call("mr_warp_normalize", ptr(d_src), ptr(d_desc), n, Hd, Wd, mean[0], mean[1], mean[2], ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()
