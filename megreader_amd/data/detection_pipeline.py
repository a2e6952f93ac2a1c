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
        quads, tags, plans, G = self._targets([im.shape for im in images], polygons, ignore_tags, plans,
                                              check=lambda: check_images(images))
        warp = plans is not None
        descs = ((WarpDesc if warp else ImgDesc) * n)()
        if warp:                                        # only each plan's source window is uploaded
            pixels = [im[y:y + h, x:x + w] for im, (x, y, w, h) in zip(images, (plan.window for plan in plans))]
        else:
            pixels = list(images)
        lay = Sections(pixels + self._target_sections(descs, n, G), pad_end=True)
        for i, off in enumerate(lay.offsets[:n]):
            if warp:
                plans[i].fill(descs[i], off)
            else:
                self._identity(descs[i], off)
        staged, views = self._staging.stage(slot, lay)
        return staged, self._fill_targets(staged, lay, views, n, quads, tags, G, warp)

    def _targets(self, shapes, polygons, ignore_tags, plans, check=None):
        """Checks one batch's annotations against its image shapes (h, w[, 3]) and draws the augmentation plans where the
        pipeline has an augmenter: (quads, tags, plans or None, G polygon slots per image) -- with plans, the quads and tags
        are the plans' surviving, transformed ones."""
        n = len(shapes)
        H, W = self.image_size
        if len(polygons) != n or len(ignore_tags) != n:
            raise ValueError("DetectionPipeline: %d images, %d polygon lists, %d tag lists" % (n, len(polygons), len(ignore_tags)))
        quads = [as_quads(p, "DetectionPipeline takes") for p in polygons]
        tags = [np.asarray(t).astype(bool).reshape(-1) for t in ignore_tags]
        for q, t in zip(quads, tags):
            if len(q) != len(t):
                raise ValueError("DetectionPipeline: %d polygons with %d ignore tags" % (len(q), len(t)))
        if check is not None:
            check()
        if self.augmenter is not None or plans is not None:
            if plans is None:
                plans = [self.augmenter.sample(shape, q, t) for shape, q, t in zip(shapes, quads, tags)]
            if len(plans) != n:
                raise ValueError("DetectionPipeline: %d images, %d plans" % (n, len(plans)))
            for shape, plan in zip(shapes, plans):
                if tuple(plan.canvas) != (H, W) or tuple(plan.shape) != tuple(shape[:2]):
                    raise ValueError("DetectionPipeline: a plan from %s onto %s for an image of %s and a canvas of %s"
                                     % (tuple(plan.shape), tuple(plan.canvas), tuple(shape[:2]), (H, W)))
            quads = [as_quads(plan.polygons, "DetectionPipeline takes") for plan in plans]
            tags = [np.asarray(plan.ignore_tags).astype(bool).reshape(-1) for plan in plans]
        else:
            for shape in shapes:
                if tuple(shape[:2]) != (H, W):
                    raise ValueError("DetectionPipeline takes images already cropped to %s, got %s" % ((H, W), tuple(shape[:2])))
        most = max([len(q) for q in quads] or [0])
        G = most if self.max_polygons is None else self.max_polygons
        if most > G or G > MAX_POLYGONS:
            raise ValueError("DetectionPipeline: %d polygons in one image exceed the %d slots" % (most, min(G, MAX_POLYGONS)))
        return quads, tags, plans, G

    def _identity(self, desc, offset):
        """The `ImgDesc` of an image of `image_size` at byte `offset`: mr_resize_normalize at identity scale."""
        H, W = self.image_size
        desc.offset, desc.h, desc.w, desc.pitch, desc.dst_w = offset, H, W, W * 3, W
        desc.scale_x = desc.scale_y = 1.0

    @staticmethod
    def _target_sections(descs, n, G):
        """The four sections behind the pixels: descriptors, quads, counts, tags."""
        return [descs, n * G * 64, n * 4, n * G * 4]

    @staticmethod
    def _fill_targets(staged, lay, views, n, quads, tags, G, warp):
        """Fills the last three sections of a staged layout and returns the layout tuple `upload` takes."""
        desc_off, poly_off, count_off, tag_off = lay.offsets[-4:]
        staged.numpy()[poly_off:] = 0                   # the empty polygon slots and the padding between the sections
        pv = views[-3].view(np.float64).reshape(n, G, 4, 2)
        cv = views[-2].view(np.int32)
        tv = views[-1].view(np.int32).reshape(n, G)
        for i, (q, t) in enumerate(zip(quads, tags)):
            pv[i, :len(q)] = q
            cv[i] = len(q)
            tv[i, :len(t)] = t
        return (n, G, desc_off, poly_off, count_off, tag_off) + (('warp',) if warp else ())

    def upload(self, staged, layout):
        """One async H2D copy of the staging buffer, then the two kernels' launches, on the CURRENT stream."""
        return self._kernels(upload(staged, self.device), layout)

    def _kernels(self, dbuf, layout):
        """mr_warp_normalize / mr_resize_normalize and mr_db_targets over the uploaded buffer."""
        n, G, desc_off, poly_off, count_off, tag_off = layout[:6]
        H, W = self.image_size
        dev = self.device
        image = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
        call("mr_warp_normalize" if layout[6:7] == ('warp',) else "mr_resize_normalize", ptr(dbuf), dbuf.data_ptr() + desc_off,
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


class EncodedDetectionPipeline(DetectionPipeline):
    """`DetectionPipeline` fed with ENCODED photos: `pack(blobs, polygons, ignore_tags, slot=0, plans=None)` / `upload` /
    `process` have the same shape, so `Prefetcher` drives it unchanged.  The host reads only the JPEG headers (data/jpeg_decode.py);
    the image shapes come from that plan, so the augmenter draws its plans without any pixels.  The device buffer of `upload` is
    [staged bytes | workspace | decoded photos]: a photo without restart markers, one long work item, is decoded by many lanes
    (csrc/jpeg_split.hip; `split_above`, `subseq_bytes`: data/jpeg_decode.py), and the descriptors address the decoded photos --
    the whole photo without an augmenter, the plan's window INSIDE the whole decoded photo (offset of its first pixel, the
    photo's pitch) with one.  What the device does not decode (progressive JPEG, PNG, ...) is decoded on the host and staged as
    whole photos beside the blobs.  The batch also carries 'jpeg_status', int32 [n] on the device (MR_JPEG_CORRUPT: a damaged
    stream; nothing synchronises to look at it here)."""

    def __init__(self, image_size=(640, 640), min_text_size=8, shrink_ratio=0.4, thresh_min=0.3, thresh_max=0.7,
                 max_polygons=None, device=None, augmenter=None, host_above=None, split_above=None, subseq_bytes=None):
        super().__init__(image_size, min_text_size, shrink_ratio, thresh_min, thresh_max, max_polygons, device, augmenter)
        from .jpeg_decode import HOST_ABOVE, SPLIT_ABOVE, JpegDecoder
        self.decoder = JpegDecoder(self.device, 'BGR', HOST_ABOVE if host_above is None else host_above,
                                   SPLIT_ABOVE if split_above is None else split_above, subseq_bytes)

    def pack(self, blobs, polygons, ignore_tags, slot=0, plans=None):
        """Host side: ONE staging buffer [blobs | plan | host-decoded photos | descriptors | quads | counts | tags].  Raises
        ValueError for blobs whose headers are corrupt."""
        from .jpeg_decode import plan_layout, stage_plan
        jplan = self.decoder.plan(blobs)
        if jplan.corrupt():
            raise ValueError("corrupt JPEG data at batch indices %s" % jplan.corrupt())
        n = jplan.n
        shapes = [tuple(jplan.shape(i)) + (3,) for i in range(n)]
        quads, tags, plans, G = self._targets(shapes, polygons, ignore_tags, plans)
        warp = plans is not None
        descs = ((WarpDesc if warp else ImgDesc) * n)()
        lay, jpeg = plan_layout(jplan, self._target_sections(descs, n, G))
        at = dict(zip(sorted(jplan.host), lay.offsets[lay.first:]))
        out_off = jpeg[4]
        for i in range(n):
            base = at[i] if i in at else out_off + jplan.images[i].out_off
            if warp:
                wx, wy = plans[i].window[:2]
                plans[i].fill(descs[i], base + (wy * shapes[i][1] + wx) * 3, shapes[i][1] * 3)
            else:
                self._identity(descs[i], base)
        staged, views = stage_plan(jplan, lay, self._staging, slot)
        return staged, self._fill_targets(staged, lay, views, n, quads, tags, G, warp) + (jpeg,)

    def upload(self, staged, layout):
        """One device buffer, one async H2D copy of the staged part, the JPEG decode and the two kernels of `DetectionPipeline`,
        on the CURRENT stream."""
        from .jpeg_decode import upload_and_launch
        dbuf, status = upload_and_launch(staged, layout[-1], self.device)
        batch = self._kernels(dbuf, layout)
        batch['jpeg_status'] = status
        return batch
