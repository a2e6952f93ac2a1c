"""The DB detector's training augmentation as a per-image PLAN: host only, numpy float64, no pixel is read.

The reference augments every sample in its DataLoader workers (experiments/seg_detector/community-base.yaml):

    Fliplr 0.5 -> Affine rotate +-10 deg -> Resize x[0.5, 3.0]        data/processes/augment_data.py (imgaug)
    -> RandomCropData 640 x 640                                         data/processes/random_crop_data.py (cv2.resize)

resampling the image three times.  None of the decisions looks at a pixel: the flip, the angle, the scale and the crop
rectangle depend on the image shape and the polygons only (`crop_area` reads `img.shape` and the polygon boxes).  So the
chain collapses to a plan -- a few drawn numbers, one affine map for the polygon points (source -> canvas) and one inverse
affine map (canvas -> source) along which `mr_warp_normalize` (csrc/image_sample.hip) samples the decoded source once and
writes the normalised canvas:

    aug = DetectionAugmenter(size=(640, 640), seed=0)
    pipe = DetectionPipeline(image_size=(640, 640), augmenter=aug)     # takes photos of any size plus their quads

`size` is (width, height) as `RandomCropData.size` is; shapes are (rows, columns).  The stages, each with the convention
the reference's stage uses for that kind of data (the point map and the pixel map differ on purpose), for a source of
H rows and W columns:

  flip     points and pixels: x -> (W - 1) - x.
  rotate   by theta about (cx, cy) = ((W - 1) / 2, (H - 1) / 2), c = cos theta, s = sin theta: points and pixels
           x' = c dx - s dy + cx, y' = s dx + c dy + cy; the output keeps the size.  A positive angle moves the point
           right of the centre downwards (y grows downwards).
  resize   to (nh, nw) = (max(1, int(round(H s))), max(1, int(round(W s)))).  Points are multiplied by nw / W and nh / H
           (imgaug's keypoint rule); pixels are centre-aligned: x_src = (x_dst + 0.5) W / nw - 0.5.
  crop     `crop_area` restated step by step on the non-ignored augmented polygons and (nh, nw) -- its integer rounding,
           numpy's slicing of negative coordinates, `ymax = ymin + width` (the reference's use of `width` for the crop
           height), its `min_crop_side_ratio` filter and its fallback recursion without a target size -- with this object's
           Generator in the place of `np.random`.  For the rectangle (cx, cy, cw, ch): scale = min(size_w / cw, size_h / ch),
           h = int(ch scale), w = int(cw scale); points (p - (cx, cy)) scale; pixels centre-aligned inside the crop,
           x_c = (u + 0.5) cw / w - 0.5 clamped to [0, cw - 1] -- "cut out first, then resized with replicated borders", so
           nothing outside the rectangle bleeds in.  The clamp is carried in canvas coordinates.  Polygons for which
           `is_poly_outside_rect(poly, 0, 0, w, h)` holds are dropped; the others keep their ignore flag.

`pixels_inv` is the product of the four inverse pixel stages.  Canvas pixels outside the valid (w, h) region are the zero
canvas of RandomCropData; source taps outside the image read as 0 (imgaug `cval=0`).  The window is the part of the source
the valid canvas can touch: the bounding box of the source coordinates of the clamped valid rectangle's corners, grown by
one pixel and cut to the image (an affine map takes a rectangle into the hull of its corners; the extra pixel holds the
second bilinear tap and any last-bit rounding).  Only the window is uploaded.

Draw order of `sample` (fixed; all three are drawn whatever the settings): flip = random() < fliplr; angle =
uniform(rotate); scale = uniform(scale); then per crop try `choice(w_axis, 2)`, `choice(h_axis, 2)`.

Parity unpinned: imgaug and cv2 are not dependencies and cannot be run beside this code, so
  * imgaug's flip and rotation-centre conventions changed between its versions (W - 1 - x against W - x, (W - 1) / 2
    against W / 2); the ones above are this module's own, half a pixel from the alternatives;
  * imgaug's `Resize` interpolates with its "cubic" default and `Affine` with order 1; here every stage is bilinear;
  * three resamplings are fused into one bilinear one: the result is sharper than the reference's and differs from it
    at every pixel that is not a flat region;
  * the random streams cannot be compared: imgaug draws from its own global generator and `crop_area` from `np.random`;
    a seed here reproduces this module only.
"""
import ctypes
import math

import numpy as np

from .._lib import STRUCTS
from .staging import as_quads


class WarpDesc(ctypes.Structure):
    """struct mr_warp_desc of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_warp_desc"]


def is_poly_outside_rect(poly, x, y, w, h):
    """random_crop_data.py:63-69."""
    poly = np.asarray(poly, dtype=np.float64)
    if poly[:, 0].max() < x or poly[:, 0].min() > x + w:
        return True
    if poly[:, 1].max() < y or poly[:, 1].min() > y + h:
        return True
    return False


def crop_area(rng, shape, polys, width=None, height=None, max_tries=10, min_crop_side_ratio=0.1):
    """random_crop_data.py:71-124 for an image of `shape` = (h, w); `rng.choice` stands in for `np.random.choice`.
    Returns python ints (x, y, w, h)."""
    h, w = int(shape[0]), int(shape[1])
    h_array = np.zeros(h, dtype=np.int32)
    w_array = np.zeros(w, dtype=np.int32)
    for points in polys:
        points = np.round(np.asarray(points, dtype=np.float64), decimals=0).astype(np.int32)
        minx, maxx = np.min(points[:, 0]), np.max(points[:, 0])
        w_array[minx:maxx] = 1                  # numpy's slicing: a negative bound counts from the end
        miny, maxy = np.min(points[:, 1]), np.max(points[:, 1])
        h_array[miny:maxy] = 1
    h_axis = np.where(h_array == 0)[0]          # rows and columns no cared-for text crosses
    w_axis = np.where(w_array == 0)[0]
    if len(h_axis) == 0 or len(w_axis) == 0:
        return 0, 0, w, h
    for _ in range(max_tries):
        xx = rng.choice(w_axis, size=2)
        xmin = np.min(xx)
        xmax = xmin + width if width is not None else np.max(xx)
        xmin = np.clip(xmin, 0, w - 1)
        xmax = np.clip(xmax, 0, w - 1)
        yy = rng.choice(h_axis, size=2)
        ymin = np.min(yy)
        ymax = ymin + width if height is not None else np.max(yy)      # `width`: as the reference
        ymin = np.clip(ymin, 0, h - 1)
        ymax = np.clip(ymax, 0, h - 1)
        if xmax - xmin < min_crop_side_ratio * w or ymax - ymin < min_crop_side_ratio * h:
            continue                            # area too small
        for poly in polys:
            if not is_poly_outside_rect(poly, xmin, ymin, xmax - xmin, ymax - ymin):
                return int(xmin), int(ymin), int(xmax - xmin), int(ymax - ymin)
    if height is not None:
        return crop_area(rng, shape, polys, None, None, max_tries, min_crop_side_ratio)
    return 0, 0, w, h


def _affine(a, b, tx, c, d, ty):
    return np.array([[a, b, tx], [c, d, ty], [0.0, 0.0, 1.0]], dtype=np.float64)


def apply_points(matrix, points):
    """The 3 x 3 point map on an array [..., 2] of (x, y), each coordinate as m0 x + m1 y + m2 (left to right)."""
    p = np.asarray(points, dtype=np.float64)
    x, y = p[..., 0], p[..., 1]
    return np.stack([matrix[0, 0] * x + matrix[0, 1] * y + matrix[0, 2],
                     matrix[1, 0] * x + matrix[1, 1] * y + matrix[1, 2]], axis=-1)


class AugmentPlan(object):
    """One image's augmentation: the drawn parameters (`shape` (H, W) of the source, `flip`, `angle` in degrees, `scale`,
    `resized` (nh, nw), `crop` (x, y, w, h) in the resized image, `canvas` (H, W)), `points` (3 x 3, source -> canvas),
    `pixels_inv` (a[6], canvas -> source), `valid` (w, h), `clamp` (cu0, cu1, cv0, cv1), `window` (x, y, w, h) in the
    source, and the surviving transformed `polygons` [K, 4, 2] with their `ignore_tags` [K] and `kept` (indices into the
    polygons the plan was made from)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def fill(self, desc, offset, pitch=None):
        """Write this plan into a `WarpDesc` whose window was uploaded at byte `offset` with `pitch` bytes per row."""
        wx, wy, ww, wh = self.window
        desc.offset, desc.pitch = int(offset), int(3 * ww if pitch is None else pitch)
        desc.src_h, desc.src_w = int(self.shape[0]), int(self.shape[1])
        desc.win_x, desc.win_y, desc.win_h, desc.win_w = int(wx), int(wy), int(wh), int(ww)
        desc.dst_h, desc.dst_w = int(self.valid[1]), int(self.valid[0])
        desc.reserved = 0
        desc.cu0, desc.cu1, desc.cv0, desc.cv1 = (float(c) for c in self.clamp)
        for k in range(6):
            desc.a[k] = float(self.pixels_inv[k])
        return desc


def source_window(shape, valid, clamp, a):
    """(x, y, w, h): the bounding box, grown by one pixel and cut to the image, of the source coordinates of the clamped
    valid canvas rectangle's corners."""
    H, W = int(shape[0]), int(shape[1])
    w, h = valid
    if w <= 0 or h <= 0:
        return 0, 0, 0, 0
    us = [min(max(float(u), clamp[0]), clamp[1]) for u in (0, w - 1)]
    vs = [min(max(float(v), clamp[2]), clamp[3]) for v in (0, h - 1)]
    xs = [a[0] * u + a[1] * v + a[2] for u in us for v in vs]
    ys = [a[3] * u + a[4] * v + a[5] for u in us for v in vs]
    x0 = max(int(math.floor(min(xs))) - 1, 0)
    y0 = max(int(math.floor(min(ys))) - 1, 0)
    x1 = min(int(math.floor(max(xs))) + 2, W - 1)          # inclusive; floor + 1 is the second tap
    y1 = min(int(math.floor(max(ys))) + 2, H - 1)
    if x1 < x0 or y1 < y0:
        return 0, 0, 0, 0
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def _quads(polygons):
    """Any array of 8 K numbers is K quadrilaterals here: reshaped before the shared check, which then never refuses."""
    return as_quads(np.asarray(polygons, dtype=np.float64).reshape(-1, 4, 2), "DetectionAugmenter takes")


class DetectionAugmenter(object):
    def __init__(self, size=(640, 640), fliplr=0.5, rotate=(-10, 10), scale=(0.5, 3.0), max_tries=10,
                 min_crop_side_ratio=0.1, seed=None):
        self.size = (int(size[0]), int(size[1]))        # (width, height), as RandomCropData.size
        self.fliplr = float(fliplr)
        self.rotate = (float(rotate[0]), float(rotate[1]))
        self.scale = (float(scale[0]), float(scale[1]))
        self.max_tries = int(max_tries)
        self.min_crop_side_ratio = float(min_crop_side_ratio)
        self.rng = np.random.default_rng(seed)

    # ---- the stages --------------------------------------------------------------------------------------------------
    @staticmethod
    def stages(shape, flip, angle, scale):
        """The first three stages for a source of `shape`: (points 3 x 3 source -> resized, pixels_inv 3 x 3 resized ->
        source, (nh, nw))."""
        H, W = int(shape[0]), int(shape[1])
        points = np.eye(3)
        inv = np.eye(3)
        if flip:
            f = _affine(-1.0, 0.0, W - 1.0, 0.0, 1.0, 0.0)          # its own inverse
            points = f @ points
            inv = inv @ f
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        th = math.radians(float(angle))
        c, s = math.cos(th), math.sin(th)
        #   x' = c (x - cx) - s (y - cy) + cx ; y' = s (x - cx) + c (y - cy) + cy   and the same with -theta
        points = _affine(c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy) @ points
        inv = inv @ _affine(c, s, cx - c * cx - s * cy, -s, c, cy + s * cx - c * cy)
        nh, nw = max(1, int(round(H * float(scale)))), max(1, int(round(W * float(scale))))
        points = _affine(nw / W, 0.0, 0.0, 0.0, nh / H, 0.0) @ points
        inv = inv @ _affine(W / nw, 0.0, 0.5 * W / nw - 0.5, 0.0, H / nh, 0.5 * H / nh - 0.5)
        return points, inv, (nh, nw)

    def plan(self, shape, polygons=(), ignore_tags=(), flip=False, angle=0.0, scale=1.0, crop=None, size=None):
        """The plan of GIVEN parameters (what `sample` calls after drawing them).  crop: (x, y, w, h) in the resized image,
        None = all of it; size: (width, height) of the canvas, None = this augmenter's."""
        H, W = int(shape[0]), int(shape[1])
        size_w, size_h = self.size if size is None else (int(size[0]), int(size[1]))
        quads = _quads(polygons)
        tags = np.asarray(ignore_tags).astype(bool).reshape(-1)
        if len(quads) != len(tags):
            raise ValueError("DetectionAugmenter: %d polygons with %d ignore tags" % (len(quads), len(tags)))
        points, inv, (nh, nw) = self.stages((H, W), flip, angle, scale)
        crop_x, crop_y, cw, ch = (0, 0, nw, nh) if crop is None else (int(c) for c in crop)
        if cw < 1 or ch < 1 or crop_x < 0 or crop_y < 0 or crop_x + cw > nw or crop_y + ch > nh:
            raise ValueError("crop %s does not lie in the resized image %d x %d" % ((crop_x, crop_y, cw, ch), nw, nh))
        s = min(size_w / cw, size_h / ch)
        h, w = int(ch * s), int(cw * s)
        points = _affine(s, 0.0, -crop_x * s, 0.0, s, -crop_y * s) @ points
        if w >= 1 and h >= 1:
            inv = inv @ _affine(cw / w, 0.0, 0.5 * cw / w - 0.5 + crop_x, 0.0, ch / h, 0.5 * ch / h - 0.5 + crop_y)
            # x_c in [0, cw - 1]  <=>  u in [(0 + 0.5) w / cw - 0.5, (cw - 1 + 0.5) w / cw - 0.5]
            clamp = (0.5 * w / cw - 0.5, (cw - 0.5) * w / cw - 0.5, 0.5 * h / ch - 0.5, (ch - 0.5) * h / ch - 0.5)
        else:                                                   # a crop thinner than one canvas pixel: nothing valid
            w = h = 0
            clamp = (0.0, 0.0, 0.0, 0.0)
        a = inv[:2].reshape(6).copy()
        out = apply_points(points, quads)
        kept = [k for k in range(len(out)) if not is_poly_outside_rect(out[k], 0, 0, w, h)]
        return AugmentPlan(shape=(H, W), flip=bool(flip), angle=float(angle), scale=float(scale), resized=(nh, nw),
                           crop=(crop_x, crop_y, cw, ch), canvas=(size_h, size_w), points=points, pixels_inv=a,
                           valid=(w, h), clamp=clamp, window=source_window((H, W), (w, h), clamp, a),
                           polygons=out[kept].reshape(-1, 4, 2), ignore_tags=tags[kept], kept=np.array(kept, dtype=np.int64))

    def sample(self, shape, polygons=(), ignore_tags=()):
        """Draw one plan for an image of `shape` (H, W[, C]) with its quads: flip, angle, scale, then the crop tries."""
        quads = _quads(polygons)
        tags = np.asarray(ignore_tags).astype(bool).reshape(-1)
        if len(quads) != len(tags):
            raise ValueError("DetectionAugmenter: %d polygons with %d ignore tags" % (len(quads), len(tags)))
        flip = bool(self.rng.random() < self.fliplr)
        angle = float(self.rng.uniform(self.rotate[0], self.rotate[1]))
        scale = float(self.rng.uniform(self.scale[0], self.scale[1]))
        points, _, resized = self.stages(shape[:2], flip, angle, scale)
        care = [q for q, t in zip(apply_points(points, quads), tags) if not t]
        crop = crop_area(self.rng, resized, care, self.size[0], self.size[1], self.max_tries, self.min_crop_side_ratio)
        return self.plan(shape[:2], quads, tags, flip, angle, scale, crop)

    @staticmethod
    def resize_to(width, height, shape, polygons=(), ignore_tags=()):
        """The validation chain (`Resize {width, height}` alone): canvas (height, width), everything valid, the clamp the
        full canvas, no polygon dropped."""
        H, W = int(shape[0]), int(shape[1])
        width, height = int(width), int(height)
        quads = _quads(polygons)
        tags = np.asarray(ignore_tags).astype(bool).reshape(-1)
        if len(quads) != len(tags):
            raise ValueError("DetectionAugmenter: %d polygons with %d ignore tags" % (len(quads), len(tags)))
        points = _affine(width / W, 0.0, 0.0, 0.0, height / H, 0.0)
        inv = _affine(W / width, 0.0, 0.5 * W / width - 0.5, 0.0, H / height, 0.5 * H / height - 0.5)
        a = inv[:2].reshape(6).copy()
        clamp = (0.0, width - 1.0, 0.0, height - 1.0)
        return AugmentPlan(shape=(H, W), flip=False, angle=0.0, scale=None, resized=(height, width),
                           crop=(0, 0, width, height), canvas=(height, width), points=points, pixels_inv=a,
                           valid=(width, height), clamp=clamp, window=source_window((H, W), (width, height), clamp, a),
                           polygons=apply_points(points, quads).reshape(-1, 4, 2), ignore_tags=tags,
                           kept=np.arange(len(quads), dtype=np.int64))
