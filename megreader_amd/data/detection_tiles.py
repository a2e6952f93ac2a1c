"""Tiled multi-scale detection: read large photos at their own scale.

A DB detector has one input size.  `TextReader` without this module squeezes every photo onto that one canvas, so a
2160 x 3840 photo loses a factor of 3.75 per axis and a 12 px word arrives 3 px high.  Here the photo is resized to a CANVAS at
its own scale (`scales`: one canvas per entry, a "level"), the canvas is covered by overlapping detector-sized tiles, the
detector runs on the tiles, and the tiles' probability maps are fused into ONE map per photo before any box is read -- so a word
cut by a tile border comes back as one box, which fusing boxes afterwards cannot repair.

    tiler = DetectionTiler(tile=(576, 1024), halo=(64, 64), scales=('fit', 1.0))
    maps = tiler.detect(detector, photos)       # photos: uint8 HWC numpy arrays or CUDA tensors; one f32 [1, 1, Hb, Wb] per photo

The plan is made on the host from shapes alone, in Python integers and float64; the pixel work is two launches
(csrc/det_tiles.hip, arithmetic in include/megreader_hip.h): `mr_tile_sample` draws all tiles of all photos and levels from the
resident uint8 photos, `mr_tile_stitch` gathers the tiles' maps of all levels into one packed buffer of fused maps.

Levels.  'fit' is the detector's own canvas, `tile`, with the photo resized to it anisotropically: what `TextReader` does
without tiles, always one tile.  A float s > 0 is the canvas Hc = max(align, int(h*s/align + 0.5)*align), Wc likewise -- the
rounding form of the reference's `keep_ratio` (data/processes/resize_image.py:40-48).  The resize follows cv2's rule as
`DevicePipeline._describe` does: scale_x = 1.0 / (float(Wc) / float(w)).  The fused map has the size of the level with the
largest canvas area (the first listed of equal ones), the base level; the other levels are resampled onto it bilinearly.

The 1-D cover (`cover_1d`), applied to each axis on its own: a side L, tiles of side t with halo h, stride s = t - 2h.  L <= t is
one tile at 0.  Otherwise K = ceil((L - t)/s) + 1 tiles start at k*s -- every origin a multiple of `align`, none shifted back at
the end, so the last tile may overhang L -- and tile k answers for its CORE: [0, t - h) for the first, [k*s + h, k*s + t - h)
inside, [(K - 1)*s + h, L) for the last.  The cores partition [0, L); a fused pixel is the value of the one tile whose core holds
it (`cover_owner`), where the tile saw at least h pixels of context on every inner side.  There are no blending weights.

The invariant.  Pixels of a tile outside its canvas are 0.0f, which is what a detector's own zero padding supplies beyond a
whole canvas.  So for a detector whose output pixel depends on inputs within distance r <= halo, that pads with zeros and is
equivariant under shifts by multiples of `align`, `detect` at scale 1.0 equals the detector on the whole canvas bit for bit
(tests/test_det_tiles_gpu.py).

The halo default, (64, 64), is a choice: nobody has measured what a trained DB needs.  The receptive field of a ResNet
detector is far larger than any practical halo; what matters is how far the response to a stroke actually reaches.
"""
import ctypes
import math

import numpy as np
import torch

from .._lib import STRUCTS, call, dtype_code, ptr
from .device_pipeline import RGB_MEAN
from .quad_crop import CropImage
from .staging import Sections, Staging, check_images, upload

FUSE_CODES = {'max': 0, 'mean': 1}             # MR_TILE_FUSE_MAX, MR_TILE_FUSE_MEAN


class TileDesc(ctypes.Structure):
    """struct mr_tile_desc of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_tile_desc"]


class StitchLevel(ctypes.Structure):
    """struct mr_stitch_level of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_stitch_level"]


class StitchPhoto(ctypes.Structure):
    """struct mr_stitch_photo of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_stitch_photo"]


def check_cover(t, h, align):
    """The refusals of the 1-D cover: ValueError unless t % align == 0, h % align == 0, h >= 0 and t > 2h."""
    t, h, align = int(t), int(h), int(align)
    if align < 1:
        raise ValueError("align must be at least 1, got %r" % (align,))
    if t < 1 or t % align:
        raise ValueError("a tile side must be a positive multiple of align=%d, got %r" % (align, t))
    if h < 0 or h % align:
        raise ValueError("a halo must be a non-negative multiple of align=%d, got %r" % (align, h))
    if t <= 2 * h:
        raise ValueError("a tile side must exceed twice the halo (t > 2h), got t=%r h=%r" % (t, h))


def cover_1d(L, t, h, align=1):
    """The cover of a side L by tiles of side t with halo h: (origins [K], cores [K] of (lo, hi), half open)."""
    L = int(L)
    check_cover(t, h, align)
    if L < 1:
        raise ValueError("a canvas side must be at least 1, got %r" % (L,))
    if L <= t:
        return [0], [(0, L)]
    s = t - 2 * h
    K = -(-(L - t) // s) + 1
    origins = [k * s for k in range(K)]
    cores = [(0 if k == 0 else origins[k] + h, L if k == K - 1 else origins[k] + t - h) for k in range(K)]
    return origins, cores


def cover_owner(p, t, h, K):
    """The tile whose core holds canvas coordinate p (include/megreader_hip.h)."""
    return 0 if p < t - h else min(K - 1, (p - h) // (t - 2 * h))


def canvas_size(shape, scale, tile, align):
    """(Hc, Wc) of a photo of `shape` (h, w[, c]) at the level `scale`: 'fit' or a float."""
    if scale == 'fit':
        return int(tile[0]), int(tile[1])
    return (max(align, int(int(shape[0]) * scale / align + 0.5) * align),
            max(align, int(int(shape[1]) * scale / align + 0.5) * align))


class Level(object):
    """One level of one photo: `scale`, `canvas` (Hc, Wc), `scale_x`, `scale_y` (cv2.resize's), `ys`, `xs` (tile origins),
    `cores_y`, `cores_x`, `first` (index of its tile (0, 0); tile (ky, kx) is first + ky * len(xs) + kx)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


class TilePlan(object):
    """What `DetectionTiler.plan` returns: `shapes` [(h, w)], `tile`, `halo`, `fuse`, `levels` (per photo a list of `Level` in
    listed order), `base` (per photo the index of its base level), `sizes` (per photo (Hb, Wb)), `offsets` (per photo the first
    element of its fused map in the packed output), `total` (elements of that output), `T` and `tiles`: per tile (photo, level,
    ky, kx, x0, y0)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)
        self._tables = None                                                    # the stitch tables on the device, once uploaded

    def tile_descs(self):
        descs = (TileDesc * max(self.T, 1))()
        for d, (i, l, _, _, x0, y0) in zip(descs, self.tiles):
            lv = self.levels[i][l]
            d.image, d.x0, d.y0, d.wc, d.hc, d.reserved = i, x0, y0, lv.canvas[1], lv.canvas[0], 0
            d.scale_x, d.scale_y = lv.scale_x, lv.scale_y
        return descs

    def stitch_tables(self):
        """(the `StitchLevel` array, the `StitchPhoto` array, the largest Hb * Wb)."""
        n = len(self.shapes)
        levels = (StitchLevel * max(sum(len(lv) for lv in self.levels), 1))()
        photos = (StitchPhoto * max(n, 1))()
        at = 0
        for i in range(n):
            p = photos[i]
            p.offset, (p.hb, p.wb) = self.offsets[i], self.sizes[i]
            p.levels, p.first_level, p.base, p.reserved = len(self.levels[i]), at, self.base[i], 0
            for lv in self.levels[i]:
                e = levels[at]
                (e.hc, e.wc), e.ky, e.kx, e.first, e.reserved = lv.canvas, len(lv.ys), len(lv.xs), lv.first, 0
                e.ratio_x, e.ratio_y = float(e.wc) / float(p.wb), float(e.hc) / float(p.hb)
                at += 1
        return levels, photos, max([h * w for h, w in self.sizes] + [0])


def _eval(module, x):
    """module(x) under no_grad, in eval mode for the call (a module that was training is put back)."""
    was_training = bool(getattr(module, 'training', False))
    if was_training:
        module.eval()
    try:
        with torch.no_grad():
            return module(x)
    finally:
        if was_training:
            module.train()


class DetectionTiler(object):
    """See the module docstring.  tile, halo, max_canvas: (rows, columns).  `max_canvas` bounds the fused map: its default of
    2048 rows is `mr_db_boxes`' documented limit H <= 2048 (include/megreader_hip.h), which the representer's device path meets
    next."""

    def __init__(self, tile=(576, 1024), halo=(64, 64), scales=(1.0,), fuse='max', align=32, max_canvas=(2048, 4096),
                 device=None):
        scales = tuple(scales) if not isinstance(scales, str) else (scales,)
        if not scales:
            raise ValueError("scales must name at least one level, got %r" % (scales,))
        for s in scales:
            if s == 'fit':
                continue
            if isinstance(s, str) or not (math.isfinite(float(s)) and float(s) > 0.0):
                raise ValueError("a scale must be 'fit' or a finite number > 0, got %r" % (s,))
        if fuse not in FUSE_CODES:
            raise ValueError("fuse must be 'max' or 'mean', got %r" % (fuse,))
        self.tile = (int(tile[0]), int(tile[1]))
        self.halo = (int(halo[0]), int(halo[1]))
        self.align = int(align)
        for t, h in zip(self.tile, self.halo):
            check_cover(t, h, self.align)
        self.scales = tuple(s if s == 'fit' else float(s) for s in scales)
        self.fuse = fuse
        self.max_canvas = (int(max_canvas[0]), int(max_canvas[1]))
        self.device = torch.device(device if device is not None else "cuda")
        self._staging, self._stitch_staging = Staging(), Staging()

    def plan(self, shapes):
        """shapes: (h, w[, c]) per photo -> `TilePlan`.  Reads no pixel."""
        shapes = [(int(s[0]), int(s[1])) for s in shapes]
        th, tw = self.tile
        all_levels, base, sizes, offsets, tiles = [], [], [], [], []
        total = 0
        for i, (h, w) in enumerate(shapes):
            if h < 1 or w < 1:
                raise ValueError("photo %d has no pixels: shape %r" % (i, (h, w)))
            levels = []
            for l, s in enumerate(self.scales):
                Hc, Wc = canvas_size((h, w), s, self.tile, self.align)
                ys, cores_y = cover_1d(Hc, th, self.halo[0], self.align)
                xs, cores_x = cover_1d(Wc, tw, self.halo[1], self.align)
                levels.append(Level(scale=s, canvas=(Hc, Wc), ys=ys, xs=xs, cores_y=cores_y, cores_x=cores_x, first=len(tiles),
                                    # cv2: inv_scale = (double)dsize / ssize; scale = 1. / inv_scale
                                    scale_x=1.0 / (float(Wc) / float(w)), scale_y=1.0 / (float(Hc) / float(h))))
                tiles.extend((i, l, ky, kx, x0, y0) for ky, y0 in enumerate(ys) for kx, x0 in enumerate(xs))
            b = max(range(len(levels)), key=lambda k: (levels[k].canvas[0] * levels[k].canvas[1], -k))
            Hb, Wb = levels[b].canvas
            if Hb > self.max_canvas[0] or Wb > self.max_canvas[1]:
                raise ValueError("photo %d of shape %r has a base canvas of %r, beyond max_canvas=%r (mr_db_boxes reads maps of "
                                 "at most 2048 rows: H <= 2048)" % (i, (h, w), (Hb, Wb), self.max_canvas))
            all_levels.append(levels)
            base.append(b)
            sizes.append((Hb, Wb))
            offsets.append(total)
            total += Hb * Wb
        return TilePlan(shapes=shapes, tile=self.tile, halo=self.halo, fuse=self.fuse, levels=all_levels, base=base, sizes=sizes,
                        offsets=offsets, total=total, T=len(tiles), tiles=tiles)

    def sample(self, photos, plan=None):
        """photos: uint8 HWC numpy arrays (staged and uploaded) or CUDA tensors (used in place), as `QuadCropper.pack` takes
        them.  One staging copy of the numpy photos and all tables, one launch, on the CURRENT stream.  Returns {'tiles': f32
        [T, 3, th, tw], 'plan': the `TilePlan`}."""
        photos = list(photos)
        check_images(photos, tensors=True)
        for im in photos:
            if isinstance(im, torch.Tensor) and not im.is_cuda:
                raise TypeError("photos are numpy arrays (staged and uploaded) or CUDA tensors (used in place)")
        if plan is None:
            plan = self.plan([im.shape for im in photos])
        n = len(photos)
        if len(plan.shapes) != n or any(tuple(im.shape[:2]) != s for im, s in zip(photos, plan.shapes)):
            raise ValueError("DetectionTiler: the plan was made for shapes %r" % (plan.shapes,))
        table = (CropImage * max(n, 1))()
        staged_photos, resident = [], []
        for i, im in enumerate(photos):
            table[i].h, table[i].w, table[i].reserved = int(im.shape[0]), int(im.shape[1]), 0
            if isinstance(im, torch.Tensor):
                if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * im.shape[1]:
                    im = im.contiguous()
                table[i].pitch = int(im.stride(0))
                resident.append((i, im))                # .offset: relative to the device buffer, known once it is allocated
            else:
                table[i].pitch = int(im.shape[1]) * 3
                staged_photos.append((i, im))
        levels, stitch_photos, max_pixels = plan.stitch_tables()
        lay = Sections([im for _, im in staged_photos] + [table, plan.tile_descs(), levels, stitch_photos], pad_end=True)
        for (i, _), off in zip(staged_photos, lay.offsets):
            table[i].offset = off
        staged, _ = self._staging.stage(0, lay)
        table_off, desc_off, level_off, photo_off = lay.offsets[len(staged_photos):]

        def place_resident(dbuf):
            rows = staged.numpy()[table_off:table_off + n * ctypes.sizeof(CropImage)]
            offsets = rows.view(np.int64).reshape(n, ctypes.sizeof(CropImage) // 8)[:, 0]
            for i, im in resident:
                offsets[i] = im.data_ptr() - dbuf.data_ptr()
        dbuf = upload(staged, self.device, place_resident if resident else None)
        th, tw = self.tile
        tiles = torch.empty((plan.T, 3, th, tw), dtype=torch.float32, device=self.device)
        call("mr_tile_sample", ptr(dbuf), dbuf.data_ptr() + table_off, n, dbuf.data_ptr() + desc_off, plan.T, th, tw,
             RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(tiles))
        plan._tables = (dbuf, dbuf.data_ptr() + level_off, len(levels), dbuf.data_ptr() + photo_off, max_pixels)
        return {'tiles': tiles, 'plan': plan, '_keepalive': (dbuf, [im for _, im in resident])}

    def _stitch_tables(self, plan):
        if plan._tables is None:
            levels, photos, max_pixels = plan.stitch_tables()
            lay = Sections([levels, photos], pad_end=True)
            staged, _ = self._stitch_staging.stage(0, lay)
            dbuf = upload(staged, self.device)
            plan._tables = (dbuf, dbuf.data_ptr() + lay.offsets[0], len(levels), dbuf.data_ptr() + lay.offsets[1], max_pixels)
        return plan._tables

    def stitch(self, plan, maps, out=None):
        """maps: the detector's maps of the plan's tiles, [T, 1, th, tw] or [T, th, tw], f32 or bf16, contiguous, on the device.
        One launch on the CURRENT stream.  Returns one f32 [1, 1, Hb, Wb] view per photo of one packed buffer (`out`: that
        buffer, f32 [plan.total], when the caller owns it)."""
        th, tw = self.tile
        if tuple(maps.shape) not in ((plan.T, 1, th, tw), (plan.T, th, tw)):
            raise ValueError("the maps of %d tiles of %d x %d have shape [%d, 1, %d, %d], got %r"
                             % (plan.T, th, tw, plan.T, th, tw, tuple(maps.shape)))
        if tuple(plan.tile) != self.tile or tuple(plan.halo) != self.halo:
            raise ValueError("the plan was made for tiles %r with halo %r" % (plan.tile, plan.halo))
        if not maps.is_cuda:
            raise TypeError("maps must be on the device, got a %s tensor" % (maps.device,))
        if maps.dtype not in (torch.float32, torch.bfloat16):
            maps = maps.float()
        maps = maps.contiguous()
        if out is None:
            out = torch.empty((plan.total,), dtype=torch.float32, device=maps.device)
        elif out.dtype != torch.float32 or out.dim() != 1 or out.numel() < plan.total or not out.is_contiguous():
            raise ValueError("out must be a contiguous f32 [%d] buffer" % plan.total)
        dbuf, levels, L, photos, max_pixels = self._stitch_tables(plan)
        if plan.shapes:
            call("mr_tile_stitch", dtype_code(maps.dtype), ptr(maps), plan.T, th, tw, self.halo[0], self.halo[1], levels, L,
                 photos, len(plan.shapes), max_pixels, FUSE_CODES[plan.fuse], ptr(out), out.numel())
        return [out[o:o + h * w].view(1, 1, h, w) for o, (h, w) in zip(plan.offsets, plan.sizes)]

    def detect_maps(self, detector, photos, batch=8, keys=('binary',)):
        """`detect` for every map named in `keys` of a detector that returns a dict (a detector that returns a tensor returns
        'binary'): {key: one fused f32 [1, 1, Hb, Wb] map per photo}."""
        if int(batch) < 1:
            raise ValueError("batch must be at least 1, got %r" % (batch,))
        sampled = self.sample(photos)
        plan, tiles = sampled['plan'], sampled['tiles']
        th, tw = self.tile
        buffers = {}
        for lo in range(0, plan.T, int(batch)):
            chunk = tiles[lo:lo + int(batch)]
            pred = _eval(detector, chunk)
            if not isinstance(pred, dict):
                pred = {'binary': pred}
            for key in keys:
                m = pred[key]
                if not torch.is_tensor(m) or tuple(m.shape) != (chunk.shape[0], 1, th, tw):
                    raise ValueError("the detector's %r map of %d tiles of %d x %d must have shape %r, got %r: a detector whose "
                                     "map is not tile-sized cannot be stitched"
                                     % (key, chunk.shape[0], th, tw, (chunk.shape[0], 1, th, tw),
                                        tuple(m.shape) if torch.is_tensor(m) else type(m).__name__))
                if key not in buffers:
                    dtype = m.dtype if m.dtype in (torch.float32, torch.bfloat16) else torch.float32
                    buffers[key] = torch.empty((plan.T, 1, th, tw), dtype=dtype, device=m.device)
                buffers[key][lo:lo + chunk.shape[0]].copy_(m)
        return {key: self.stitch(plan, buffers[key]) if key in buffers else [] for key in keys}

    def detect(self, detector, photos, batch=8):
        """The detector (a callable tiles f32 [n, 3, th, tw] -> [n, 1, th, tw], or a dict with such a 'binary') on all tiles of
        all photos and levels, in eval mode under no_grad, in chunks of `batch` tiles into one [T, 1, th, tw] buffer, and the
        fused maps: one f32 [1, 1, Hb, Wb] per photo.  A detector whose map is not tile-sized raises ValueError."""
        return self.detect_maps(detector, photos, batch, ('binary',))['binary']
