"""The recognisers' training augmentation as a per-sample DESCRIPTOR: host only, vectorised numpy float64, no pixel is read.

A recognition batch is otherwise the bare resize of the stored crop.  Here every sample may get geometric jitter, a wavy baseline,
a colour change, blur, noise, pixelation and erased rectangles -- what one expects when training on MJSynth / SynthText / real
crops -- and `mr_rec_augment` (csrc/rec_augment.hip, arithmetic in include/megreader_hip.h) applies all of it in ONE bilinear pass
from the resident uint8 pixels to the normalised f32 planes:

    aug = RecognitionAugmenter(seed=0, p=0.5)
    pipe = DevicePipeline(image_size=(32, 128), augmenter=aug)          # also EncodedDevicePipeline and QuadCropper
    table, rows = aug.sample([im.shape for im in images], (32, 128), 'resize', index)      # what `pack` does per batch

Frames and conventions.  A sample's FRAME is the (rotated) crop the resize reads: Hr rows and Wr columns, pixel centres at the
integers, so its outline is [-0.5, Wr - 0.5] x [-0.5, Hr - 0.5] and its centre c = ((Wr - 1) / 2, (Hr - 1) / 2); y grows
downwards.  The visible motion F of the content, about c, is in this order

    scale     d -> s d                                      s > 1 enlarges the content
    shear     x -> x + sh y                                 sh > 0 moves what lies below the centre to the right
    rotate    x' = cos(t) x - sin(t) y, y' = sin(t) x + cos(t) y      a positive angle moves the point right of the centre
                                                            DOWNWARDS: clockwise on screen; +90 degrees takes the top-left
                                                            corner of a square frame onto its top-right corner
    translate d -> d + (tx, ty) Hr                          positive tx moves the content to the right, positive ty down
    perspective   the four outline corners (TL, TR, BR, BL), moved by the above, are displaced by persp[k] Hr each

and `g` is the projective map that takes the four moved corners back onto the outline's corners (`homographies` of quad_crop.py):
g maps the OUTPUT frame to the SOURCE frame, the inverse of the visible motion.  The output pixel at p shows the source at g(p): for a
translation g(p) = p - (tx, ty) Hr, for the +90 degree rotation g(top-right) = top-left.  With no motion at all g is the exact identity.
All geometric magnitudes are fractions of the frame height Hr (`translate`, `perspective`) or of the canvas height H (`distort`,
`stretch`: the knots are canvas pixels) where they are not degrees or ratios.

The knots.  dx / dy displace the sampling point by up to `stretch` H / `distort` H canvas pixels at 9 knots over [0, dst_w], linear
in between: dy is the wavy baseline, dx a local stretch.  `sample` draws 9 values each and smooths them once with (1/4, 1/2, 1/4)
(the end knots repeat themselves).  The displacement is of the SAMPLING point: a positive dy shows what lies below.

Colour.  One affine map per sample, composed in float64 in this order: grey mix (all three channels become the luma
0.114 B + 0.587 G + 0.299 R), contrast about 127.5 and brightness (x -> contrast (x - 127.5) + 127.5 + brightness), channel gains,
inversion (x -> 255 - x); the kernel clamps to [0, 255].

The 5 x 5 kernel.  The outer product of the 5-tap Gaussian `blur_taps(sigma)` of synth_text.py (sigma <= MIN_SIGMA: no blur), or,
for motion blur, an anti-aliased line through the centre: the weight of cell (i, j) is max(0, 1 - distance to the segment of the
drawn length and angle), normalised.  Computed in float64, stored as float32, and the centre entry then absorbs the rounding so
that the float32 entries sum to 1 within 2^-24.

The clamp.  A stored crop's frame coordinate is clamped to [0, Wr - 1] x [0, Hr - 1], a replicated border.  A quad crop's is
widened by `context` Hr on every side: jitter then reveals the photo around the word, not smeared edge pixels.

Draws.  `sample(..., index)` draws ONE matrix `default_rng([seed, index]).random((n, N_DRAWS))`: row k belongs to sample k and
column j to one quantity (`DRAWS` names them), mapped affinely onto its range.  Every quantity is drawn for every sample whatever
the settings, so a sample's values depend on (seed, index, k) and its own ranges alone: changing one range shifts no other stream,
and neither does the batch size.

The default ranges are choices, not measurements: nothing here was tuned against real data.
"""
import ctypes
import math

import numpy as np

from .._lib import STRUCTS
from .device_pipeline import target_width
from .quad_crop import CropPlan, homographies
from .synth_text import blur_taps


class AugDesc(ctypes.Structure):
    """struct mr_aug_desc of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_aug_desc"]


AUG_DTYPE = np.dtype(AugDesc)
KNOTS, MAX_ERASE = 9, 4
MIN_SIGMA = 0.1           # below it the Gaussian's neighbours are < 1e-21: no blur

# Column j of the draw matrix -> the quantity it drives (a name with a count takes that many consecutive columns).
DRAWS = (("apply", 1), ("rotate", 1), ("shear", 1), ("scale", 1), ("translate", 2), ("perspective", 8), ("dx", KNOTS),
         ("dy", KNOTS), ("contrast", 1), ("brightness", 1), ("channel_gain", 3), ("gray", 1), ("invert", 1), ("sigma", 1),
         ("motion", 1), ("motion_length", 1), ("motion_angle", 1), ("noise", 1), ("seed", 1), ("pixelate_on", 1), ("pixelate", 1),
         ("erase_on", 1), ("erase_count", 1), ("erase", MAX_ERASE * 7))
N_DRAWS = sum(c for _, c in DRAWS)


def _columns(R):
    out, at = {}, 0
    for name, count in DRAWS:
        out[name] = R[:, at] if count == 1 else R[:, at:at + count]
        at += count
    return out


def _between(r, lo_hi):
    lo, hi = float(lo_hi[0]), float(lo_hi[1])
    return lo + (hi - lo) * r


def smooth_knots(raw):
    """[n, 9] -> [n, 9]: one pass of (1/4, 1/2, 1/4), the end knots repeating themselves."""
    raw = np.asarray(raw, dtype=np.float64)
    pad = np.concatenate([raw[:, :1], raw, raw[:, -1:]], axis=1)
    return 0.25 * pad[:, :-2] + 0.5 * pad[:, 1:-1] + 0.25 * pad[:, 2:]


def knot_displacement(knots, U, dst_w):
    """The displacement the kernel adds at canvas abscissa U (float64 array): its knot rule restated (include/megreader_hip.h)."""
    knots = np.asarray(knots, dtype=np.float32).astype(np.float64)
    t = np.asarray(U, dtype=np.float64) * 8.0 / float(dst_w)
    j = np.fmin(np.fmax(np.floor(t), 0.0), 7.0).astype(np.int64)
    f = t - j.astype(np.float64)
    return knots[j] + (knots[j + 1] - knots[j]) * f


def gaussian_kernels(sigma):
    """[n] -> float64 [n, 5, 5]: the outer products of the 5-tap Gaussians; the identity kernel where sigma <= MIN_SIGMA."""
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    on = sigma > MIN_SIGMA
    w = blur_taps(np.where(on, sigma, 1.0)).astype(np.float64)                       # [n, 3]: w0, w1, w2
    taps = np.stack([w[:, 2], w[:, 1], w[:, 0], w[:, 1], w[:, 2]], axis=1)
    taps = np.where(on[:, None], taps / taps.sum(axis=1, keepdims=True), np.array([0.0, 0.0, 1.0, 0.0, 0.0]))
    return taps[:, :, None] * taps[:, None, :]


def motion_kernels(length, angle):
    """[n], [n] (cells, degrees) -> float64 [n, 5, 5]: normalised anti-aliased lines through the centre.  Rows are v (y down): a
    positive angle turns the line clockwise on screen."""
    length = np.asarray(length, dtype=np.float64).reshape(-1, 1, 1)
    th = np.radians(np.asarray(angle, dtype=np.float64)).reshape(-1, 1, 1)
    i = np.arange(-2, 3, dtype=np.float64)[None, None, :]
    j = np.arange(-2, 3, dtype=np.float64)[None, :, None]
    dx, dy = np.cos(th), np.sin(th)
    half = np.maximum(length - 1.0, 0.0) / 2.0
    along = np.clip(i * dx + j * dy, -half, half)
    dist = np.hypot(i - along * dx, j - along * dy)
    k = np.maximum(0.0, 1.0 - dist)
    return k / k.sum(axis=(1, 2), keepdims=True)


def kernels_f32(k64):
    """float64 [n, 5, 5] of sum 1 -> float32 [n, 25] whose entries sum to 1 within 2^-24: the centre absorbs the rounding."""
    k = np.asarray(k64, dtype=np.float64).reshape(-1, 25).astype(np.float32)
    others = k.astype(np.float64).sum(axis=1) - k[:, 12].astype(np.float64)
    k[:, 12] = (1.0 - others).astype(np.float32)
    return k


def colour_maps(contrast, brightness, gain, gray, invert):
    """[n], [n], [n, 3], bool [n], bool [n] -> (float64 [n, 3, 3], float64 [n, 3]): the composed map col = m val + b."""
    n = len(contrast)
    M = np.zeros((n, 4, 4), dtype=np.float64)
    M[:] = np.eye(4)
    luma = np.array([0.114, 0.587, 0.299], dtype=np.float64)                         # B, G, R as the pixels are
    M[gray, :3, :3] = luma[None, :]
    C = np.zeros((n, 4, 4), dtype=np.float64)
    C[:] = np.eye(4)
    for c in range(3):
        C[:, c, c] = contrast
        C[:, c, 3] = 127.5 - contrast * 127.5 + brightness
    G = np.zeros((n, 4, 4), dtype=np.float64)
    G[:, 3, 3] = 1.0
    for c in range(3):
        G[:, c, c] = gain[:, c]
    V = np.zeros((n, 4, 4), dtype=np.float64)
    V[:] = np.eye(4)
    for c in range(3):
        V[invert, c, c] = -1.0
        V[invert, c, 3] = 255.0
    T = V @ G @ C @ M
    return T[:, :3, :3], T[:, :3, 3]


def jitter_maps(frames, rotate, shear, scale, translate, perspective):
    """frames [n, 2] (Hr, Wr); angles in degrees [n]; shear, scale [n]; translate [n, 2] and perspective [n, 4, 2] as fractions of
    Hr -> g float64 [n, 9]: output frame -> source frame (module docstring).  Exactly the identity where nothing moves."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, 2)
    n = len(frames)
    Hr, Wr = frames[:, 0], frames[:, 1]
    cx, cy = (Wr - 1.0) / 2.0, (Hr - 1.0) / 2.0
    corners = np.stack([np.stack([-0.5 + 0 * Wr, -0.5 + 0 * Hr], -1), np.stack([Wr - 0.5, -0.5 + 0 * Hr], -1),
                        np.stack([Wr - 0.5, Hr - 0.5], -1), np.stack([-0.5 + 0 * Wr, Hr - 0.5], -1)], axis=1)     # [n, 4, 2]
    x = (corners[..., 0] - cx[:, None]) * np.asarray(scale, dtype=np.float64).reshape(n, 1)
    y = (corners[..., 1] - cy[:, None]) * np.asarray(scale, dtype=np.float64).reshape(n, 1)
    x = x + np.asarray(shear, dtype=np.float64).reshape(n, 1) * y
    th = np.radians(np.asarray(rotate, dtype=np.float64)).reshape(n, 1)
    c, s = np.cos(th), np.sin(th)
    x, y = c * x - s * y, s * x + c * y
    t = np.asarray(translate, dtype=np.float64).reshape(n, 1, 2) + np.asarray(perspective, dtype=np.float64).reshape(n, 4, 2)
    moved = np.stack([x + cx[:, None], y + cy[:, None]], axis=-1) + t * Hr[:, None, None]
    still = (moved == corners).all(axis=(1, 2))
    g = np.tile(np.eye(3).reshape(1, 9), (n, 1))
    if (~still).any():
        g[~still] = homographies(moved[~still], corners[~still]).reshape(-1, 9)
    return g


def apply_map(m9, points):
    """The projective map m9 (9 numbers, row major) on points [..., 2]."""
    m = np.asarray(m9, dtype=np.float64).reshape(9)
    p = np.asarray(points, dtype=np.float64)
    X = m[0] * p[..., 0] + m[1] * p[..., 1] + m[2]
    Y = m[3] * p[..., 0] + m[4] * p[..., 1] + m[5]
    D = m[6] * p[..., 0] + m[7] * p[..., 1] + m[8]
    return np.stack([X / D, Y / D], axis=-1)


class RecognitionAugmenter(object):
    """See the module docstring.  The defaults are choices, not measurements.  Ranges are (low, high); `translate`, `perspective`,
    `distort` and `stretch` are magnitudes drawn symmetrically about 0; the `*_prob` are per-sample probabilities; `pixelate` and
    `erase_count` are inclusive integer ranges; `erase_size`: each side of a rectangle as a fraction of the canvas height;
    `motion_length` in kernel cells, its angle is uniform over [0, 180) degrees; `p`: the share of samples augmented at all."""

    def __init__(self, seed=0, p=0.5, rotate=(-5, 5), shear=(-0.2, 0.2), scale=(0.9, 1.1), translate=0.05, perspective=0.08,
                 distort=0.08, stretch=0.05, contrast=(0.6, 1.4), brightness=(-30, 30), channel_gain=(0.9, 1.1), gray_prob=0.1,
                 invert_prob=0.05, gaussian_sigma=(0.0, 1.2), motion_prob=0.15, motion_length=(3, 5), noise=(0.0, 16.0),
                 pixelate_prob=0.1, pixelate=(2, 3), erase_prob=0.1, erase_count=(1, 2), erase_size=(0.1, 0.3), context=0.25):
        def pair(name, v, lo=None, hi=None):
            v = (float(v[0]), float(v[1]))
            if not (math.isfinite(v[0]) and math.isfinite(v[1]) and v[0] <= v[1]) or (lo is not None and v[0] < lo) \
                    or (hi is not None and v[1] > hi):
                raise ValueError("RecognitionAugmenter: %s=%r is not a range (low, high)%s" % (
                    name, v, "" if lo is None else " within [%g, %s]" % (lo, "inf" if hi is None else "%g" % hi)))
            return v

        def amount(name, v, hi=None):
            v = float(v)
            if not (math.isfinite(v) and v >= 0.0) or (hi is not None and v > hi):
                raise ValueError("RecognitionAugmenter: %s=%r must lie in [0, %s]" % (name, v, "inf" if hi is None else "%g" % hi))
            return v
        self.seed = int(seed)
        if self.seed < 0:
            raise ValueError("RecognitionAugmenter: seed=%r must be >= 0" % (seed,))
        self.p = amount("p", p, 1.0)
        self.rotate = pair("rotate", rotate, -180.0, 180.0)
        self.shear = pair("shear", shear)
        self.scale = pair("scale", scale, 1e-3)
        self.translate = amount("translate", translate)
        self.perspective = amount("perspective", perspective)
        self.distort = amount("distort", distort)
        self.stretch = amount("stretch", stretch)
        self.contrast = pair("contrast", contrast, 0.0)
        self.brightness = pair("brightness", brightness)
        self.channel_gain = pair("channel_gain", channel_gain, 0.0)
        self.gray_prob = amount("gray_prob", gray_prob, 1.0)
        self.invert_prob = amount("invert_prob", invert_prob, 1.0)
        self.gaussian_sigma = pair("gaussian_sigma", gaussian_sigma, 0.0)
        self.motion_prob = amount("motion_prob", motion_prob, 1.0)
        self.motion_length = pair("motion_length", motion_length, 1.0, 5.0)
        self.noise = pair("noise", noise, 0.0)
        self.pixelate_prob = amount("pixelate_prob", pixelate_prob, 1.0)
        self.pixelate = (int(pixelate[0]), int(pixelate[1]))
        if not 1 <= self.pixelate[0] <= self.pixelate[1]:
            raise ValueError("RecognitionAugmenter: pixelate=%r is not an integer range within [1, inf]" % (pixelate,))
        self.erase_prob = amount("erase_prob", erase_prob, 1.0)
        self.erase_count = (int(erase_count[0]), int(erase_count[1]))
        if not 0 <= self.erase_count[0] <= self.erase_count[1] <= MAX_ERASE:
            raise ValueError("RecognitionAugmenter: erase_count=%r is not an integer range within [0, %d]"
                             % (erase_count, MAX_ERASE))
        self.erase_size = pair("erase_size", erase_size, 0.0)
        self.context = amount("context", context)

    # ---- frames ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _frames(items, canvas, mode):
        """(frame [n, 2], dst_w [n], sx [n], sy [n], h [n, 9], quad [n] bool) of shapes (h, w[, c]) or CropPlans."""
        if mode not in ('resize', 'pad'):
            raise NotImplementedError("RecognitionAugmenter supports the batched modes 'resize' and 'pad'")
        H, W = int(canvas[0]), int(canvas[1])
        if H < 1 or W < 1:
            raise ValueError("RecognitionAugmenter: canvas %r" % (canvas,))
        n = len(items)
        frame, dst_w = np.zeros((n, 2), dtype=np.float64), np.zeros(n, dtype=np.int64)
        sx, sy = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        h9, quad = np.tile(np.eye(3).reshape(1, 9), (n, 1)), np.zeros(n, dtype=bool)
        for k, it in enumerate(items):
            if isinstance(it, CropPlan):
                if tuple(it.canvas) != (H, W):
                    raise ValueError("RecognitionAugmenter: a crop plan onto %s for a canvas of %s" % (tuple(it.canvas), (H, W)))
                frame[k], dst_w[k], sx[k], sy[k], h9[k], quad[k] = it.frame, it.dst_w, it.sx, it.sy, it.h9, True
            else:
                hr, wr = int(it[0]), int(it[1])
                if hr < 1 or wr < 1:
                    raise ValueError("RecognitionAugmenter: a crop of shape %r" % (tuple(it),))
                frame[k] = hr, wr
                dst_w[k] = W if mode == 'resize' else target_width('pad', (H, W), (hr, wr))
                # cv2: inv_scale = (double)dsize / ssize; scale = 1. / inv_scale   (as DevicePipeline._describe)
                sx[k], sy[k] = 1.0 / (float(dst_w[k]) / float(wr)), 1.0 / (float(H) / float(hr))
        return frame, dst_w, sx, sy, h9, quad

    def _table(self, frames, canvas, image, row, rotate, shear, scale, translate, perspective, dx, dy, contrast, brightness, gain,
               gray, invert, kernel, blur, noise, seed, quant, erase, erase_col, n_erase):
        """The descriptor table of n samples from their parameters, all arrays of length n."""
        frame, dst_w, sx, sy, h9, quad = frames
        n = len(frame)
        t = np.zeros(n, dtype=AUG_DTYPE)
        t["image"], t["row"], t["dst_w"], t["quant"], t["blur"], t["n_erase"], t["seed"] = image, row, dst_w, quant, blur, n_erase, seed
        t["sx"], t["sy"] = sx, sy
        margin = np.where(quad, self.context * frame[:, 0], 0.0)
        t["cu0"], t["cu1"] = 0.0 - margin, frame[:, 1] - 1.0 + margin
        t["cv0"], t["cv1"] = 0.0 - margin, frame[:, 0] - 1.0 + margin
        t["g"] = jitter_maps(frame, rotate, shear, scale, translate, perspective)
        t["h"] = h9
        t["dx"], t["dy"] = dx, dy
        m, b = colour_maps(contrast, brightness, gain, gray, invert)
        t["m"], t["b"] = m.reshape(n, 9), b
        t["k"] = kernel
        t["noise_amp"] = noise
        t["erase"], t["erase_col"] = erase.reshape(n, 16), erase_col.reshape(n, 12)
        return t

    # ---- explicit plans ----------------------------------------------------------------------------------------------------------
    def plan(self, shape, canvas, mode='resize', rotate=0.0, shear=0.0, scale=1.0, translate=(0.0, 0.0),
             perspective=((0.0, 0.0),) * 4, dx=(0.0,) * KNOTS, dy=(0.0,) * KNOTS, contrast=1.0, brightness=0.0,
             channel_gain=(1.0, 1.0, 1.0), gray=False, invert=False, sigma=0.0, motion=None, kernel=None, noise=0.0, seed=0,
             pixelate=1, erase=(), image=0, row=0):
        """One descriptor (an AUG_DTYPE array of length 1) of GIVEN values, no randomness.  shape: (h, w[, c]) of a stored crop, or
        a `CropPlan`.  translate, perspective (TL, TR, BR, BL): fractions of the frame height; dx, dy: the 9 knots in canvas
        pixels, as given (not smoothed); motion: (length, angle in degrees) in the place of the Gaussian of `sigma`; kernel: 25
        numbers in the place of both; erase: up to 4 rectangles ((x0, x1, y0, y1), (c0, c1, c2)) in canvas pixels."""
        frames = self._frames([shape], canvas, mode)
        erase = list(erase)
        if len(erase) > MAX_ERASE:
            raise ValueError("RecognitionAugmenter.plan: %d rectangles, at most %d" % (len(erase), MAX_ERASE))
        if len(dx) != KNOTS or len(dy) != KNOTS:
            raise ValueError("RecognitionAugmenter.plan: dx and dy take %d knots" % KNOTS)
        if int(pixelate) < 1:
            raise ValueError("RecognitionAugmenter.plan: pixelate=%r" % (pixelate,))
        rect, col = np.zeros((1, MAX_ERASE, 4), dtype=np.int64), np.zeros((1, MAX_ERASE, 3), dtype=np.float64)
        for e, (r, c) in enumerate(erase):
            rect[0, e], col[0, e] = r, c
        if kernel is not None:
            k, blur = np.asarray(kernel, dtype=np.float32).reshape(1, 25), 1
        elif motion is not None:
            k, blur = kernels_f32(motion_kernels([motion[0]], [motion[1]])), 1
        else:
            k, blur = kernels_f32(gaussian_kernels([sigma])), int(float(sigma) > MIN_SIGMA)
        one = lambda v: np.array([v])
        return self._table(frames, canvas, one(int(image)), one(int(row)), one(float(rotate)), one(float(shear)), one(float(scale)),
                           np.asarray(translate, dtype=np.float64).reshape(1, 2),
                           np.asarray(perspective, dtype=np.float64).reshape(1, 4, 2), np.asarray(dx, dtype=np.float64)[None],
                           np.asarray(dy, dtype=np.float64)[None], one(float(contrast)), one(float(brightness)),
                           np.asarray(channel_gain, dtype=np.float64).reshape(1, 3), one(bool(gray)), one(bool(invert)), k,
                           one(blur), one(float(noise)), np.array([int(seed) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32),
                           one(int(pixelate)), rect, col, one(len(erase)))

    def identity(self, shape, canvas, mode='resize', image=0, row=0):
        """The identity descriptor of a stored crop's shape or a `CropPlan`: the row `mr_quad_crop` writes, bit for bit."""
        t = self.plan(shape, canvas, mode, image=image, row=row)
        if isinstance(shape, CropPlan):                  # (the identity has no use for context around the word)
            t["cu0"], t["cv0"], t["cu1"], t["cv1"] = 0.0, 0.0, shape.cu1, shape.cv1
        return t

    # ---- drawn plans -------------------------------------------------------------------------------------------------------------
    def draw(self, n, canvas, dst_w, index):
        """The drawn parameters of batch `index` as a dict of arrays of length n (the columns of the draw matrix, mapped onto their
        ranges; module docstring).  `apply`: which samples are augmented."""
        H = int(canvas[0])
        R = _columns(np.random.default_rng([self.seed, int(index)]).random((n, N_DRAWS)))
        sym = lambda r, a: (2.0 * r - 1.0) * a
        d = {"apply": R["apply"] < self.p}
        d["rotate"], d["shear"], d["scale"] = _between(R["rotate"], self.rotate), _between(R["shear"], self.shear), \
            _between(R["scale"], self.scale)
        d["translate"] = sym(R["translate"], self.translate)
        d["perspective"] = sym(R["perspective"], self.perspective).reshape(n, 4, 2)
        d["dx"] = smooth_knots(sym(R["dx"], self.stretch * H))
        d["dy"] = smooth_knots(sym(R["dy"], self.distort * H))
        d["contrast"], d["brightness"] = _between(R["contrast"], self.contrast), _between(R["brightness"], self.brightness)
        d["channel_gain"] = _between(R["channel_gain"], self.channel_gain)
        d["gray"], d["invert"] = R["gray"] < self.gray_prob, R["invert"] < self.invert_prob
        d["sigma"] = _between(R["sigma"], self.gaussian_sigma)
        d["motion"] = R["motion"] < self.motion_prob
        d["motion_length"] = _between(R["motion_length"], self.motion_length)
        d["motion_angle"] = 180.0 * R["motion_angle"]
        d["noise"] = _between(R["noise"], self.noise)
        d["seed"] = np.minimum(np.floor(R["seed"] * 4294967296.0), 4294967295.0).astype(np.uint32).view(np.int32)
        span = self.pixelate[1] - self.pixelate[0] + 1
        d["pixelate"] = np.where(R["pixelate_on"] < self.pixelate_prob,
                                 self.pixelate[0] + np.minimum(np.floor(R["pixelate"] * span), span - 1), 1).astype(np.int64)
        span = self.erase_count[1] - self.erase_count[0] + 1
        d["n_erase"] = np.where(R["erase_on"] < self.erase_prob,
                                self.erase_count[0] + np.minimum(np.floor(R["erase_count"] * span), span - 1), 0).astype(np.int64)
        E = R["erase"].reshape(n, MAX_ERASE, 7)
        ew, eh = _between(E[..., 0], self.erase_size) * H, _between(E[..., 1], self.erase_size) * H
        wv = np.asarray(dst_w, dtype=np.float64)[:, None]
        x0 = np.floor(-ew / 2.0 + E[..., 2] * wv)                     # may hang over either edge by half its size
        y0 = np.floor(-eh / 2.0 + E[..., 3] * H)
        d["erase"] = np.stack([x0, x0 + np.maximum(np.rint(ew), 1.0), y0, y0 + np.maximum(np.rint(eh), 1.0)], axis=-1).astype(np.int64)
        d["erase_col"] = 255.0 * E[..., 4:7]
        return d

    def sample(self, items, canvas, mode='resize', index=0, images=None):
        """The descriptor table of batch `index`: items are the samples' shapes (h, w[, c]) (stored crops: `h` is the identity)
        or `CropPlan`s (quad crops: `h` is the plan's `h9`, the clamp is widened by `context`); images: the photo index of each
        sample in the `mr_crop_image` table (default: its position).  Returns (AUG_DTYPE array [M], int64 rows [M]): the
        descriptors of the samples that are augmented, in order, and their positions -- the rows of the batch they overwrite."""
        n = len(items)
        frames = self._frames(items, canvas, mode)
        d = self.draw(n, canvas, frames[1], index)
        rows = np.nonzero(d["apply"])[0].astype(np.int64)
        images = np.arange(n, dtype=np.int64) if images is None else np.asarray(images, dtype=np.int64).reshape(n)
        if len(rows) == 0:
            return np.zeros(0, dtype=AUG_DTYPE), rows
        s = {k: v[rows] for k, v in d.items()}
        gk = gaussian_kernels(s["sigma"])
        mk = motion_kernels(s["motion_length"], s["motion_angle"])
        kernel = kernels_f32(np.where(s["motion"][:, None, None], mk, gk))
        blur = (s["motion"] | (s["sigma"] > MIN_SIGMA)).astype(np.int64)
        table = self._table(tuple(f[rows] for f in frames), canvas, images[rows], rows, s["rotate"], s["shear"], s["scale"],
                            s["translate"], s["perspective"], s["dx"], s["dy"], s["contrast"], s["brightness"],
                            s["channel_gain"], s["gray"], s["invert"], kernel, blur, s["noise"], s["seed"], s["pixelate"],
                            s["erase"], s["erase_col"], s["n_erase"])
        return table, rows


def augment_crops(photos, table, image_size, out=None):
    """The direct call, for crops already on the device (rendered uint8 crops, say).  photos: uint8 HWC CUDA tensors (a list, or
    one tensor [n, h, w, 3]); table: an AUG_DTYPE array whose `image` names a photo and whose `row` names a row of the result
    (what `RecognitionAugmenter.sample` returns for the photos' shapes).  out: f32 [N, 3, H, W] on the photos' device, of which
    only the rows the table names are written; None: a new batch [n, 3, H, W] in which every other row is the bare resize of its
    photo (mr_resize_normalize, mode 'resize').  The tables are copied from pageable memory, so the call may be repeated at
    once; it runs on the current stream."""
    import torch

    from .._lib import call, ptr
    from .device_pipeline import RGB_MEAN, ImgDesc
    from .quad_crop import CropImage
    H, W = int(image_size[0]), int(image_size[1])
    photos = list(photos)
    n = len(photos)
    table = np.ascontiguousarray(table)
    if table.dtype != AUG_DTYPE or table.ndim != 1:
        raise TypeError("augment_crops: the table is a one-dimensional array of AUG_DTYPE")
    for k, im in enumerate(photos):
        if not (isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.uint8 and im.ndim == 3 and im.shape[2] == 3):
            raise TypeError("augment_crops: photos are uint8 HWC CUDA tensors")
        if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * im.shape[1]:
            photos[k] = im.contiguous()
    rows, image = table["row"], table["image"]
    if len(table) and (image.min() < 0 or image.max() >= n):
        raise ValueError("augment_crops: a descriptor names photo %d of %d" % (int(image.max() if image.max() >= n else image.min()), n))
    N = n if out is None else int(out.shape[0])
    if len(table) and (rows.min() < 0 or rows.max() >= N or len(np.unique(rows)) != len(rows)):
        raise ValueError("augment_crops: the rows %s do not name %d rows once each" % (rows.tolist(), N))
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape[1:]) != (3, H, W) or not out.is_contiguous()
                            or not out.is_cuda):
        raise TypeError("augment_crops: out is a contiguous f32 [N, 3, %d, %d] CUDA tensor" % (H, W))
    if n == 0:
        return torch.empty((0, 3, H, W), dtype=torch.float32, device="cuda") if out is None else out
    device = photos[0].device
    images, plain = (CropImage * n)(), (ImgDesc * n)()
    host = np.zeros(ctypes.sizeof(images) + ctypes.sizeof(plain) + max(table.nbytes, 16), dtype=np.uint8)
    dbuf = torch.empty((host.size,), dtype=torch.uint8, device=device)
    for k, im in enumerate(photos):
        h, w = int(im.shape[0]), int(im.shape[1])
        images[k].offset = plain[k].offset = im.data_ptr() - dbuf.data_ptr()      # relative to the tables' buffer, may be negative
        images[k].pitch = plain[k].pitch = int(im.stride(0))
        images[k].h, images[k].w = plain[k].h, plain[k].w = h, w
        plain[k].dst_w = W
        plain[k].scale_x, plain[k].scale_y = 1.0 / (float(W) / float(w)), 1.0 / (float(H) / float(h))
    plain_off, aug_off = ctypes.sizeof(images), ctypes.sizeof(images) + ctypes.sizeof(plain)
    host[:plain_off] = np.frombuffer(images, dtype=np.uint8)
    host[plain_off:aug_off] = np.frombuffer(plain, dtype=np.uint8)
    host[aug_off:aug_off + table.nbytes] = np.frombuffer(table.tobytes(), dtype=np.uint8)
    dbuf.copy_(torch.from_numpy(host))
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=device)
        call("mr_resize_normalize", ptr(dbuf), dbuf.data_ptr() + plain_off, n, H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(out))
    call("mr_rec_augment", ptr(dbuf), ptr(dbuf), n, dbuf.data_ptr() + aug_off, len(table), N, H, W, RGB_MEAN[0], RGB_MEAN[1],
         RGB_MEAN[2], ptr(out))
    return out
