"""Detection input pipeline on the GPU: the counterpart of `DevicePipeline` for the DB detector.

The reference builds the four maps `L1BalanceCELoss` consumes on the host, per sample, in its DataLoader workers:
data/processes/make_seg_detection_data.py (`gt`, `mask`) and data/processes/make_border_map.py (`thresh_map`,
`thresh_mask`), with pyclipper, shapely and cv2 -- per polygon a [4, h, w] float array over the padded box.  Here the host
hands over the DECODED (augmented, cropped) uint8 pixels and the quadrilaterals; one async copy, `mr_resize_normalize`
at identity scale (after the crop the image chain is `NormalizeImage` only) and `mr_db_targets` (csrc/db_targets.hip) make
the batch dict of `synthetic.detection_batch` on the device:

    pipe = DetectionPipeline(image_size=(640, 640))
    for batch in Prefetcher(loader_of_(images, polygons, ignore_tags), pipe):
        loss, metrics = criterion(model(batch['image']), batch)

What the maps are (include/megreader_hip.h states it per output).  Pixel (x, y) is the integer point (x, y); all geometry
is float64.  Per polygon, in the order of `MakeSegDetectionData.process`: clip to the image, `polygon_area`, reorder,
size filter, D = |a| (1 - r^2) / perimeter, and the polygon is ignored as well when its shrunk region covers no pixel --
no pixel is both inside the polygon and at squared true distance >= D^2 from its boundary.  That restates
`shrinked == []`: for a convex polygon the inradius is at least area / perimeter, which is greater than
D = (1 - r^2) area / perimeter, so the exact inward offset by D is never empty for a convex polygon, and the pixel rule
and the reference can differ only on slivers thinner than the grid (a shrunk region that exists but holds no pixel
centre).  `gt` is the shrunk region (inside at d^2 >= D^2), `thresh_mask` the filled outward offset (inside or d^2 <= D^2),
`mask` is zeroed over the truncated points of every ignored polygon (inside, or within half a pixel of an edge -- the
stand-in for `fillPoly`'s drawn boundary), `thresh_map` is `MakeBorderMap.distance` over the polygon's padded box.

Parity unpinned: pyclipper, shapely and cv2 are not dependencies and cannot be run beside this code, so
  * pyclipper's integer vertex rounding and its arc tolerance are not modelled: the offsets here are exact;
  * `fillPoly`'s scanline and line-drawing rules are not modelled; they affect pixels within about one pixel of a
    boundary;
  * D uses the shoelace area and the summed edge lengths in place of shapely's `area` and `length`: a few ulps of D;
  * the single pixel where the reference produces NaN for a degenerate edge is not reproduced: a pixel on an end point
    gets distance 0 (its `nan_to_num` path), zero-length edges (clipping makes them) are skipped in every distance, and
    1 - cosin^2 is clamped at 0 where rounding leaves it negative.
Only quadrilaterals are supported (`validate_polygons` and the size filter index points 0..3).  Augmentation
(`AugmentDetectionData`, `RandomCropData`) is one more stage of the same pipeline when an `augmenter` is given
(data/detection_augment.py): the host draws a plan per image from the shape and the quads, uploads only the part of the raw
photo the plan can touch, and `mr_warp_normalize` (csrc/image_sample.hip) takes the place of `mr_resize_normalize`.
"""
import numpy as np
import torch

from .._lib import call, load, ptr
from .detection_augment import WarpDesc
from .device_pipeline import RGB_MEAN, ImgDesc
from .staging import Sections, Staging, as_quads, check_images, upload

MAX_POLYGONS = 1024     # mr_db_targets: polygon slots per image


class DetectionPipeline(object):
    def __init__(self, image_size=(640, 640), min_text_size=8, shrink_ratio=0.4, thresh_min=0.3, thresh_max=0.7,
                 max_polygons=None, device=None, augmenter=None):
        self.image_size = tuple(image_size)
        self.min_text_size = float(min_text_size)
        self.shrink_ratio = float(shrink_ratio)
        self.thresh_min = float(thresh_min)
        self.thresh_max = float(thresh_max)
        if max_polygons is not None and not 0 <= int(max_polygons) <= MAX_POLYGONS:
            raise ValueError("max_polygons must be in [0, %d], got %r" % (MAX_POLYGONS, max_polygons))
        self.max_polygons = None if max_polygons is None else int(max_polygons)   # None: the batch's largest count
        self.device = torch.device(device if device is not None else "cuda")
        self.augmenter = augmenter      # a DetectionAugmenter: pack() takes raw photos of any size (module docstring)
        self._staging = Staging()

    def pack(self, images, polygons, ignore_tags, slot=0, plans=None):
        """Host side: lay the uint8 HWC images (already of `image_size`), their descriptors, the quads padded to G slots
        per image (float64 [N][G][4][2]), the counts (int32 [N]) and the ignore tags (int32 [N][G]) out in ONE pinned staging
        buffer (per prefetch slot).  Returns (pinned uint8 tensor, layout tuple).
        With an augmenter (or ready-made `plans`, one AugmentPlan per image) the images are raw photos of any size: one plan
        per image is sampled, only each plan's source window is copied, warp descriptors stand in the place of `ImgDesc`,
        and the quads and tags packed are the plan's surviving, transformed ones."""
        n = len(images)
        H, W = self.image_size
        if len(polygons) != n or len(ignore_tags) != n:
            raise ValueError("DetectionPipeline: %d images, %d polygon lists, %d tag lists" % (n, len(polygons), len(ignore_tags)))
        quads = [as_quads(p, "DetectionPipeline takes") for p in polygons]
        tags = [np.asarray(t).astype(bool).reshape(-1) for t in ignore_tags]
        for q, t in zip(quads, tags):
            if len(q) != len(t):
                raise ValueError("DetectionPipeline: %d polygons with %d ignore tags" % (len(q), len(t)))
        check_images(images)
        warp = self.augmenter is not None or plans is not None
        if warp:
            if plans is None:
                plans = [self.augmenter.sample(im.shape, q, t) for im, q, t in zip(images, quads, tags)]
            if len(plans) != n:
                raise ValueError("DetectionPipeline: %d images, %d plans" % (n, len(plans)))
            for im, plan in zip(images, plans):
                if tuple(plan.canvas) != (H, W) or tuple(plan.shape) != im.shape[:2]:
                    raise ValueError("DetectionPipeline: a plan from %s onto %s for an image of %s and a canvas of %s"
                                     % (tuple(plan.shape), tuple(plan.canvas), im.shape[:2], (H, W)))
            quads = [as_quads(plan.polygons, "DetectionPipeline takes") for plan in plans]
            tags = [np.asarray(plan.ignore_tags).astype(bool).reshape(-1) for plan in plans]
        most = max([len(q) for q in quads] or [0])
        G = most if self.max_polygons is None else self.max_polygons
        if most > G or G > MAX_POLYGONS:
            raise ValueError("DetectionPipeline: %d polygons in one image exceed the %d slots" % (most, min(G, MAX_POLYGONS)))
        descs = ((WarpDesc if warp else ImgDesc) * n)()
        if warp:                                        # only each plan's source window is uploaded
            pixels = [im[y:y + h, x:x + w] for im, (x, y, w, h) in zip(images, (plan.window for plan in plans))]
        else:
            pixels = list(images)
            for im in images:
                if im.shape[:2] != (H, W):
                    raise ValueError("DetectionPipeline takes images already cropped to %s, got %s" % ((H, W), im.shape[:2]))
        lay = Sections(pixels + [descs, n * G * 64, n * 4, n * G * 4], pad_end=True)
        for i, off in enumerate(lay.offsets[:n]):
            if warp:
                plans[i].fill(descs[i], off)
            else:
                descs[i].offset, descs[i].h, descs[i].w, descs[i].pitch, descs[i].dst_w = off, H, W, W * 3, W
                descs[i].scale_x = descs[i].scale_y = 1.0
        desc_off, poly_off, count_off, tag_off = lay.offsets[n:]
        staged, views = self._staging.stage(slot, lay)
        staged.numpy()[poly_off:] = 0                   # the empty polygon slots and the padding between the sections
        pv = views[n + 1].view(np.float64).reshape(n, G, 4, 2)
        cv = views[n + 2].view(np.int32)
        tv = views[n + 3].view(np.int32).reshape(n, G)
        for i, (q, t) in enumerate(zip(quads, tags)):
            pv[i, :len(q)] = q
            cv[i] = len(q)
            tv[i, :len(t)] = t
        return staged, (n, G, desc_off, poly_off, count_off, tag_off) + (('warp',) if warp else ())

    def upload(self, staged, layout):
        """One async H2D copy of the staging buffer, then the two kernels' launches, on the CURRENT stream."""
        n, G, desc_off, poly_off, count_off, tag_off = layout[:6]
        H, W = self.image_size
        dev = self.device
        dbuf = upload(staged, dev)
        image = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
        call("mr_warp_normalize" if layout[6:] == ('warp',) else "mr_resize_normalize", ptr(dbuf), dbuf.data_ptr() + desc_off,
             n, H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(image))
        records = torch.empty((max(n * G * load().mr_sizeof_db_record(), 8) // 8,), dtype=torch.float64, device=dev)
        ignore = torch.empty((n, G), dtype=torch.int32, device=dev)
        dist = torch.empty((n, G), dtype=torch.float64, device=dev)
        gt = torch.empty((n, 1, H, W), dtype=torch.float32, device=dev)
        mask = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        thresh_map = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        thresh_mask = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        call("mr_db_targets", dbuf.data_ptr() + poly_off, dbuf.data_ptr() + count_off, dbuf.data_ptr() + tag_off, n, G, H, W,
             self.min_text_size, self.shrink_ratio, self.thresh_min, self.thresh_max, ptr(records), ptr(ignore), ptr(dist),
             ptr(gt), ptr(mask), ptr(thresh_map), ptr(thresh_mask))
        return {'image': image, 'gt': gt, 'mask': mask, 'thresh_map': thresh_map, 'thresh_mask': thresh_mask,
                'ignore_tags': ignore, '_keepalive': dbuf}

    def process(self, images, polygons, ignore_tags, plans=None):
        staged, layout = self.pack(images, polygons, ignore_tags, plans=plans)
        return self.upload(staged, layout)
