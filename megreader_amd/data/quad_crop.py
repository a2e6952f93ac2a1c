"""Quad crops: from a detected or annotated quadrilateral in a photo to the recogniser's input, planned on the host and
sampled ONCE on the GPU.

The reference does it per text line on the host (data/crop_file_dataset.py:105-124, `ImageCropper.crop(image, poly)`):

    box = min_area_rect(poly)                           concern/cv.py:5-12 (cv2.minAreaRect + cv2.boxPoints)
    w, h = |box[1] - box[0]|, |box[2] - box[1]|
    mat = getPerspectiveTransform(box, [(0, 0), (w, 0), (w, h), (0, h)]);  image = warpPerspective(image, mat, (w, h))
    image = ensure_horizontal(image)                    np.flip(np.swapaxes(image, 0, 1), 0) if height > 1.5 * width
    image = ResizeImage(image_size, mode)(image);  image -= RGB_MEAN;  image /= 255.

None of these decisions reads a pixel.  `plan_crop` composes them, in float64, into one projective map from the (rotated)
crop frame to the photo plus cv2.resize's sampling rule, and `mr_quad_crop` (csrc/image_sample.hip, arithmetic in
include/megreader_hip.h) samples the raw uint8 photo once along it and writes the normalised batch:

    cropper = QuadCropper(image_size=(32, 128))
    batch = cropper.crop(photos, quads)         # photos: uint8 HWC numpy arrays or CUDA tensors; quads: K x 4 x 2 per photo
    batch['image'], batch['index'], batch['quad']       # f32 [M, 3, H, W], i32 [M] source photo, f64 [M, 4, 2]

Frames.  The crop frame has `cw = max(int(w), 1)` columns and `ch = max(int(h), 1)` rows (warpPerspective's dsize); its point
(xc, yc) lies in the photo at p0 + xc / w (p1 - p0) + yc / h (p3 - p0).  When `ch > 1.5 * cw` the frame is rotated as the
reference rotates the pixels, R[i][j] = crop[j][cw - 1 - i]: the rotated frame has cw rows and ch columns and its point
(xr, yr) is the crop's (cw - 1 - yr, xr); the rotation is folded into `h[9]`.  The resize samples the (rotated) frame of
Hr rows and Wr columns at ((u + 0.5) sx - 0.5, (v + 0.5) sy - 0.5) clamped to [0, Wr - 1] x [0, Hr - 1], with
sx = 1. / ((double)dst_w / Wr) and sy = 1. / ((double)H / Hr) as cv2.resize and `DevicePipeline.pack` compute them; in mode
'pad' dst_w = `target_width('pad', ...)` of the (rotated) frame and the columns beyond it are the zero canvas.

`rectify='quad'` is an extension: the four corners themselves (no rectangle fitted), made clockwise and started at the
top edge, are mapped to a frame whose sides are the longer of each pair of opposite sides -- a true homography, for
annotated word quadrilaterals seen in perspective.

Known differences from the reference (parity unpinned, DESIGN.md §5: cv2 is not a dependency and cannot be run beside
this code):
  * ONE bilinear resampling instead of two (warpPerspective, then cv2.resize): sharper, and different at every pixel that
    is not in a flat region; tests/_quad_crop_ref.py restates the two-pass chain and the tests report the deviation;
  * warpPerspective's fixed-point weights (1/32 pixel, INTER_BITS = 5) and its rounding of the result to uint8 before the
    resize are not modelled;
  * the rectangle comes from the float64 calipers of structure/db_geometry.py, cv2.minAreaRect works in float32 and
    getPerspectiveTransform on the float32 corners;
  * the corner order is stated on its own terms (`rect_corners`) after OpenCV 3.4 / 4.0's angle range; OpenCV 4.5.1 changed
    that range, and the reference's two branches with it.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from .._lib import STRUCTS, call, load, ptr
from ..structure.db_geometry import min_area_rect
from .device_pipeline import RGB_MEAN, target_width
from .staging import Sections, Staging, as_quads, check_images, upload


class CropImage(ctypes.Structure):
    """struct mr_crop_image of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_crop_image"]


class CropDesc(ctypes.Structure):
    """struct mr_crop_desc of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_crop_desc"]


def top_edge_rule(d):
    """The corner rule for an edge direction d: d.x > 0 and -d.x <= d.y < d.x (within [-45, 45) degrees of the x axis)."""
    return bool(d[0] > 0.0 and -d[0] <= d[1] < d[0])


def _from_top_edge(corners):
    """The four corners clockwise on screen (y grows downwards: reversed when the shoelace sum is negative), started so that
    edge 0 -> 1 satisfies the rule; among several (or none, which rounding at exactly 45 degrees or a general quadrilateral can
    produce) the edge with the largest d.x / |d|, the first of equal ones.  Plain floats: four points, called per text line."""
    c = [(float(x), float(y)) for x, y in corners]
    if len(c) != 4:
        raise ValueError("expected four corners, got %d" % len(c))
    if sum(c[k][0] * c[(k + 1) % 4][1] - c[(k + 1) % 4][0] * c[k][1] for k in range(4)) < 0.0:
        c.reverse()
    best = None
    for k in range(4):
        d = (c[(k + 1) % 4][0] - c[k][0], c[(k + 1) % 4][1] - c[k][1])
        ln = math.hypot(d[0], d[1])
        key = (ln > 0.0 and top_edge_rule(d), d[0] / ln if ln > 0.0 else -2.0)
        if best is None or key > best[0]:
            best = (key, k)
    k = best[1]
    return np.array(c[k:] + c[:k], dtype=np.float64)


def rect_corners(quad):
    """`concern/cv.py::min_area_rect` restated: the minimum-area rectangle of the points as corners [4, 2] float64 in the
    order top-left, top-right, bottom-right, bottom-left.

    Derivation (OpenCV 3.4 / 4.0).  `minAreaRect` returns (centre, (w, h), angle) with angle in [-90, 0), and
    `boxPoints((c, (w, h), t))` returns, with a = sin(t) / 2 and b = cos(t) / 2,
        pt0 = c + (-a h - b w,  b h - a w),  pt1 = c + (a h - b w, -b h - a w),  pt2 = 2 c - pt0,  pt3 = 2 c - pt1,
    so pt1 - pt0 = h (sin t, -cos t) and pt2 - pt1 = w (cos t, sin t): their cross product is w h > 0, the corners run
    clockwise on screen (y down) for every t.  The reference calls boxPoints with
        angle < -45:   (w, h), t = angle + 180 in [90, 135):  d = pt1 - pt0 has d.x = sin t in (0.707, 1], d.y = -cos t in [0, 0.707)
        otherwise:     (h, w), t = angle + 90  in [45, 90):   d.x = sin t in [0.707, 1),  d.y = -cos t in [-0.707, 0)
    Both branches give a first edge with d.x > 0 and -d.x <= d.y < d.x (equality at angle = -45 exactly), and of the four
    edge directions of a rectangle, 90 degrees apart, exactly one lies in that half-open quarter.  So the rule -- clockwise
    on screen, edge 0 -> 1 within [-45, 45) degrees of the x axis -- picks the reference's order whatever rectangle
    representation minAreaRect chose.  Parity unpinned: cv2 cannot be run beside this code."""
    corners, _ = min_area_rect(np.asarray(quad, dtype=np.float64).reshape(-1, 2).tolist())
    return _from_top_edge(corners)


def homographies(src, dst):
    """The projective maps (3 x 3, h[8] = 1) that take the four points src[k] to dst[k]: src, dst [n, 4, 2] -> [n, 3, 3], n 8 x 8
    float64 systems in one batched solve."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 4, 2), np.asarray(dst, dtype=np.float64).reshape(-1, 4, 2)
    n = len(src)
    (xs, ys), (xd, yd) = (src[..., 0], src[..., 1]), (dst[..., 0], dst[..., 1])
    A = np.zeros((n, 8, 8), dtype=np.float64)
    A[:, 0::2, 0], A[:, 0::2, 1], A[:, 0::2, 2], A[:, 0::2, 6], A[:, 0::2, 7] = xs, ys, 1.0, -xs * xd, -ys * xd
    A[:, 1::2, 3], A[:, 1::2, 4], A[:, 1::2, 5], A[:, 1::2, 6], A[:, 1::2, 7] = xs, ys, 1.0, -xs * yd, -ys * yd
    b = np.stack([xd, yd], axis=-1).reshape(n, 8, 1)
    return np.concatenate([np.linalg.solve(A, b)[..., 0], np.ones((n, 1))], axis=1).reshape(n, 3, 3)


def _homography(src, dst):
    """The projective map (3 x 3, h[8] = 1) that takes the four points src [4, 2] to dst [4, 2]."""
    return homographies(np.asarray(src, dtype=np.float64)[None], np.asarray(dst, dtype=np.float64)[None])[0]


def crop_frame(quad, rectify='min_area_rect'):
    """(corners [4, 2] TL TR BR BL, w, h) of the crop frame: `rect_corners` with w = |p1 - p0|, h = |p2 - p1|, or ('quad') the
    four corners themselves, clockwise on screen and started by the same rule, with the longer of each pair of opposite sides."""
    if rectify == 'min_area_rect':
        p = rect_corners(quad)
        return p, float(np.linalg.norm(p[1] - p[0])), float(np.linalg.norm(p[2] - p[1]))
    if rectify == 'quad':
        p = _from_top_edge(np.asarray(quad, dtype=np.float64).reshape(4, 2))
        return p, float(max(np.linalg.norm(p[1] - p[0]), np.linalg.norm(p[2] - p[3]))), \
            float(max(np.linalg.norm(p[2] - p[1]), np.linalg.norm(p[3] - p[0])))
    raise ValueError("rectify must be 'min_area_rect' or 'quad', got %r" % (rectify,))


class DegenerateQuad(ValueError):
    """A quadrilateral with a zero side: there is no frame to crop."""


class CropPlan(object):
    """One crop: `shape` (H, W) of the photo, `corners` [4, 2] (TL, TR, BR, BL in the photo), `w`, `h` (the frame's real
    sides), `cw`, `ch` (its integer size), `rotated`, `frame` (Hr, Wr) of the (rotated) frame the resize reads, `canvas`
    (H, W), `dst_w`, `sx`, `sy`, `cu1`, `cv1`, `h9` (the 3 x 3 map from the (rotated) frame to the photo, row major) and
    `crop_map` (3 x 3, the crop frame before the rotation -> photo: what warpPerspective inverts)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def fill(self, desc, image):
        """Write this plan into a `CropDesc` that reads photo number `image` of the table."""
        desc.image, desc.dst_w = int(image), int(self.dst_w)
        desc.sx, desc.sy, desc.cu1, desc.cv1 = float(self.sx), float(self.sy), float(self.cu1), float(self.cv1)
        for k in range(9):
            desc.h[k] = float(self.h9[k])
        return desc

    def canvas_to_photo(self, points):
        """Continuous canvas coordinates (U, V), points [..., 2] with pixel u covering [u, u + 1), to photo coordinates (x, y),
        float64 [..., 2]: the sampling rule of mr_quad_crop (include/megreader_hip.h) continued beyond the pixel centres and
        without its clamp -- cx = U sx - 0.5, cy = V sy - 0.5, then `h9` with the division by D.  At a pixel centre
        (u + 0.5, v + 0.5) it is the (x, y) that pixel is sampled at wherever the clamp is inactive; the rectangle
        [0, dst_w] x [0, H] is the outline of the (rotated) frame, [-0.5, Wr - 0.5] x [-0.5, Hr - 0.5].  The rotation of a vertical
        crop is inside `h9`: boxes on the canvas come out rotated with it."""
        pts = np.asarray(points, dtype=np.float64)
        if pts.shape[-1:] != (2,):
            raise ValueError("canvas_to_photo takes points [..., 2], got %s" % (pts.shape,))
        cx = pts[..., 0] * self.sx - 0.5
        cy = pts[..., 1] * self.sy - 0.5
        h = [float(v) for v in self.h9]
        X = h[0] * cx + h[1] * cy + h[2]
        Y = h[3] * cx + h[4] * cy + h[5]
        D = h[6] * cx + h[7] * cy + h[8]
        return np.stack([X / D, Y / D], axis=-1)


def plan_crop(shape, quad, image_size=(64, 512), mode='resize', rectify='min_area_rect'):
    """The plan of one quadrilateral `quad` [4, 2] (any point set for 'min_area_rect') of a photo of `shape` (H, W[, C]) onto a
    canvas `image_size` (H, W).  Raises DegenerateQuad (a ValueError) for a quadrilateral with a zero side."""
    if mode not in ('resize', 'pad'):
        raise NotImplementedError("quad crops support the batched modes 'resize' and 'pad' "
                                  "(keep_size / keep_ratio produce per-sample shapes)")
    H, W = int(image_size[0]), int(image_size[1])
    p, w, h = crop_frame(quad, rectify)
    if not (w > 0.0 and h > 0.0 and math.isfinite(w) and math.isfinite(h)):
        raise DegenerateQuad("quad crop: the quadrilateral %s has a zero side" % (np.asarray(quad).tolist(),))
    cw, ch = max(int(w), 1), max(int(h), 1)
    if rectify == 'min_area_rect':                      # a rectangle: the map is affine, D == 1 exactly
        ex, ey = (p[1] - p[0]) / w, (p[3] - p[0]) / h
        m = np.array([[ex[0], ey[0], p[0][0]], [ex[1], ey[1], p[0][1]], [0.0, 0.0, 1.0]], dtype=np.float64)
    else:
        m = _homography([(0.0, 0.0), (w, 0.0), (w, h), (0.0, h)], p)
    crop_map = m
    rotated = ch > 1.5 * cw                             # is_vertival(height, width): height > width * 1.5
    if rotated:                                         # (xr, yr) -> (xc, yc) = (cw - 1 - yr, xr)
        m = m @ np.array([[0.0, -1.0, cw - 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64)
    Hr, Wr = (cw, ch) if rotated else (ch, cw)
    dst_w = W if mode == 'resize' else target_width('pad', (H, W), (Hr, Wr))
    return CropPlan(shape=(int(shape[0]), int(shape[1])), corners=p, w=w, h=h, cw=cw, ch=ch, rotated=bool(rotated),
                    frame=(Hr, Wr), canvas=(H, W), dst_w=int(dst_w),
                    # cv2: inv_scale = (double)dsize / ssize; scale = 1. / inv_scale
                    sx=1.0 / (float(dst_w) / float(Wr)), sy=1.0 / (float(H) / float(Hr)),
                    cu1=float(Wr - 1), cv1=float(Hr - 1), h9=m.reshape(9).copy(), crop_map=crop_map)


# aug: None, or with an augmenter (slot, number of augmented crops, offset of their mr_aug_desc table, their rows)
CropLayout = namedtuple("CropLayout", "M I table_off desc_off index_off quad_off resident plans dropped aug", defaults=(None,))


class QuadCropper(object):
    """`ImageCropper` on the GPU (the defaults are its defaults); see the module docstring.  augmenter: a
    `RecognitionAugmenter` (data/recognition_augment.py), or None.  With one, `pack` draws a descriptor per planned crop whose
    frame -> photo map is the plan's `h9` (batch index: a counter of this cropper, or `pack(..., index=)`), and `upload` runs
    mr_rec_augment over the augmented rows behind mr_quad_crop: augmented word crops straight from annotated scenes."""

    def __init__(self, image_size=(64, 512), mode='resize', rectify='min_area_rect', device=None, augmenter=None):
        if mode not in ('resize', 'pad'):
            raise NotImplementedError("QuadCropper supports the batched modes 'resize' and 'pad' "
                                      "(keep_size / keep_ratio produce per-sample shapes)")
        if rectify not in ('min_area_rect', 'quad'):
            raise ValueError("rectify must be 'min_area_rect' or 'quad', got %r" % (rectify,))
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.mode = mode
        self.rectify = rectify
        self.device = torch.device(device if device is not None else "cuda")
        load()
        self._staging = Staging()
        self.augmenter = augmenter
        self.index = 0                          # the next batch's number in the augmenter's stream
        self._copied = {}                       # slot -> the event behind the last H2D copy of its staging buffer

    def pack(self, images, quads, slot=0, plans=None, index=None):
        """Host side: plan every quadrilateral and lay the numpy photos, the photo table, the crop descriptors, the source
        indices (int32 [M]) and the quads (float64 [M][4][2]) out in ONE pinned staging buffer (per prefetch slot).  Photos that
        are CUDA tensors are not copied: their table entries are completed by `upload`.  `plans`: ready-made
        [(photo index, CropPlan)] in the place of the planning (the quads are then recorded as the plans' corners).
        Returns (pinned uint8 tensor, CropLayout)."""
        n = len(images)
        if plans is None and len(quads) != n:
            raise ValueError("QuadCropper: %d images, %d quad lists" % (n, len(quads)))
        check_images(images, tensors=True)
        for im in images:
            if isinstance(im, torch.Tensor) and not im.is_cuda:
                raise TypeError("images are numpy arrays (staged and uploaded) or CUDA tensors (used in place)")
        kept, dropped = [], []
        if plans is None:
            for i, q in enumerate(quads):
                for k, quad in enumerate(as_quads(q, "QuadCropper takes")):
                    try:
                        kept.append((i, plan_crop(images[i].shape, quad, self.image_size, self.mode, self.rectify), quad))
                    except DegenerateQuad:
                        dropped.append((i, k))
        else:
            kept = [(int(i), plan, plan.corners) for i, plan in plans]
        for i, plan, _ in kept:
            if not 0 <= i < n:
                raise ValueError("QuadCropper: a crop names photo %d of %d" % (i, n))
            if tuple(plan.canvas) != self.image_size:
                raise ValueError("QuadCropper: a plan onto %s for a canvas of %s" % (tuple(plan.canvas), self.image_size))
        M = len(kept)
        table = (CropImage * max(n, 1))()
        staged_photos, resident = [], []
        for i, im in enumerate(images):
            table[i].h, table[i].w, table[i].reserved = int(im.shape[0]), int(im.shape[1]), 0
            if isinstance(im, torch.Tensor):
                if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * im.shape[1]:
                    im = im.contiguous()
                table[i].pitch = int(im.stride(0))
                resident.append((i, im))                # .offset: relative to the device buffer `upload` allocates
            else:
                table[i].pitch = int(im.shape[1]) * 3
                staged_photos.append((i, im))
        descs = (CropDesc * max(M, 1))()
        for m, (i, plan, _) in enumerate(kept):
            plan.fill(descs[m], i)
        sections = [im for _, im in staged_photos] + [
            table, descs, np.array([i for i, _, _ in kept], dtype=np.int32),
            np.asarray([q for _, _, q in kept], dtype=np.float64).reshape(-1)]
        aug = None
        if self.augmenter is not None:
            if index is None:
                index, self.index = self.index, self.index + 1
            aug_table, rows = self.augmenter.sample([plan for _, plan, _ in kept], self.image_size, self.mode, index,
                                                    images=[i for i, _, _ in kept])
            sections.append(aug_table)
            if self._copied.get(slot) is not None:      # drawn ahead of the device: the slot's last copy must have run
                self._copied[slot].synchronize()
        lay = Sections(sections, pad_end=True)
        for (i, _), off in zip(staged_photos, lay.offsets):
            table[i].offset = off
        staged, _ = self._staging.stage(slot, lay)
        table_off, desc_off, index_off, quad_off = lay.offsets[len(staged_photos):len(staged_photos) + 4]
        if self.augmenter is not None:
            aug = (slot, len(rows), lay.offsets[-1], rows)
        return staged, CropLayout(M, n, table_off, desc_off, index_off, quad_off, resident,
                                  [plan for _, plan, _ in kept], dropped, aug)

    def upload(self, staged, layout):
        """One async H2D copy of the staging buffer, then the one launch, on the CURRENT stream (resident photos must be
        ready on it)."""
        H, W = self.image_size
        M = layout.M

        def place_resident(dbuf):
            table = staged.numpy()[layout.table_off:layout.table_off + layout.I * ctypes.sizeof(CropImage)]
            offsets = table.view(np.int64).reshape(layout.I, ctypes.sizeof(CropImage) // 8)[:, 0]
            for i, im in layout.resident:
                offsets[i] = im.data_ptr() - dbuf.data_ptr()
        dbuf = upload(staged, self.device, place_resident if layout.resident else None)
        if layout.aug is not None:
            ev = self._copied[layout.aug[0]] = torch.cuda.Event()
            ev.record()
        image = torch.empty((M, 3, H, W), dtype=torch.float32, device=self.device)
        call("mr_quad_crop", ptr(dbuf), dbuf.data_ptr() + layout.table_off, layout.I, dbuf.data_ptr() + layout.desc_off, M,
             H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(image))
        if layout.aug is not None:
            call("mr_rec_augment", ptr(dbuf), dbuf.data_ptr() + layout.table_off, layout.I, dbuf.data_ptr() + layout.aug[2],
                 layout.aug[1], M, H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(image))
        index = dbuf[layout.index_off:layout.index_off + 4 * M].view(torch.int32)
        quad = dbuf[layout.quad_off:layout.quad_off + 64 * M].view(torch.float64).view(M, 4, 2)
        return {'image': image, 'index': index, 'quad': quad, 'dropped': list(layout.dropped),
                '_keepalive': (dbuf, [im for _, im in layout.resident])}

    def crop(self, images, quads):
        """images: uint8 HWC numpy arrays or uint8 HWC CUDA tensors; quads: one K x 4 x 2 array, list or tensor per image.
        Returns {'image': f32 [M, 3, H, W], 'index': i32 [M], 'quad': f64 [M, 4, 2], 'dropped': [(image, k)]} in input order."""
        staged, layout = self.pack(images, quads)
        return self.upload(staged, layout)
