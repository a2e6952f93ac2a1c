"""Strip crops: from a `Ribbon` (structure/ribbon.py) in a photo to the recogniser's input, planned on the host and sampled ONCE on
the GPU -- `QuadCropper` (data/quad_crop.py) with a piecewise-bilinear mesh in the place of the homography, for words that follow
a curve.

    cropper = StripCropper(image_size=(32, 128))
    batch = cropper.crop(photos, ribbons)       # photos: uint8 HWC numpy arrays or CUDA tensors; ribbons: a list of Ribbon per photo
    batch['image'], batch['index']              # f32 [M, 3, H, W], i32 [M] source photo

`plan_strip` reads points only.  The centre line c_i = (T_i + B_i) / 2 is the frame's horizontal axis, measured by its cumulative
length s; the frame is w = s[-1] wide and hgt = max |T_i - B_i| high, and from there on everything is `plan_crop`'s: the integer
frame cw x ch, cv2.resize's sampling rule, `dst_w` of mode 'pad'.  There is no rotation: a ribbon already runs along the reading
direction (`Ribbon.from_box` turns a vertical box).  `mr_strip_crop` (csrc/image_sample.hip, arithmetic in
include/megreader_hip.h) maps the frame point (cx, cy) into cell i of the mesh, s[i] <= cx < s[i+1], bilinearly between the
rulings i and i + 1.  Annotated curved words (`Ribbon.from_polygon`) are cropped for recogniser training the same way."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from .._lib import STRUCTS, call, load, ptr
from ..structure.ribbon import Ribbon
from .device_pipeline import RGB_MEAN, target_width
from .quad_crop import CropImage, DegenerateQuad
from .staging import Sections, Staging, check_images, upload


class StripDesc(ctypes.Structure):
    """struct mr_strip_desc of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_strip_desc"]


class StripPlan(object):
    """One strip crop: `shape` (H, W) of the photo, `ribbon`, `s` (arc length of the centre line at every knot), `w`, `hgt` (the
    frame's real sides), `cw`, `ch` (its integer size), `frame` (ch, cw), `canvas` (H, W), `dst_w`, `sx`, `sy`, `cu1`, `cv1`."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def fill(self, desc, image):
        """Write this plan into a `StripDesc` that reads photo number `image` of the table."""
        k = self.ribbon.knots
        desc.image, desc.dst_w, desc.knots, desc.reserved = int(image), int(self.dst_w), k, 0
        desc.sx, desc.sy, desc.cu1, desc.cv1, desc.hgt = (float(v) for v in (self.sx, self.sy, self.cu1, self.cv1, self.hgt))
        for i in range(k):
            desc.s[i] = float(self.s[i])
            desc.top[i][0], desc.top[i][1] = float(self.ribbon.top[i][0]), float(self.ribbon.top[i][1])
            desc.bot[i][0], desc.bot[i][1] = float(self.ribbon.bottom[i][0]), float(self.ribbon.bottom[i][1])
        return desc

    def canvas_to_photo(self, points):
        """`CropPlan.canvas_to_photo`'s contract: continuous canvas coordinates (U, V), points [..., 2] with pixel u covering
        [u, u + 1), to photo coordinates, float64 [..., 2] -- the sampling rule of mr_strip_crop continued beyond the pixel centres
        and without its clamp: cx = U sx - 0.5, cy = V sy - 0.5, the cell of cx (the first and the last cell continued beyond the
        ends), then the two blends.  Boxes on the canvas come out following the curve."""
        pts = np.asarray(points, dtype=np.float64)
        if pts.shape[-1:] != (2,):
            raise ValueError("canvas_to_photo takes points [..., 2], got %s" % (pts.shape,))
        cx = pts[..., 0] * self.sx - 0.5
        cy = pts[..., 1] * self.sy - 0.5
        s, top, bot = self.s, self.ribbon.top, self.ribbon.bottom
        i = np.clip(np.searchsorted(s, cx, side='right') - 1, 0, len(s) - 2)
        a = ((cx - s[i]) / (s[i + 1] - s[i]))[..., None]
        b = (cy / self.hgt)[..., None]
        t = top[i] * (1.0 - a) + top[i + 1] * a
        u = bot[i] * (1.0 - a) + bot[i + 1] * a
        return t * (1.0 - b) + u * b


def plan_strip(shape, ribbon, image_size=(64, 512), mode='resize'):
    """The plan of one `ribbon` of a photo of `shape` (H, W[, C]) onto a canvas `image_size` (H, W).  Raises DegenerateQuad (a
    ValueError) for a ribbon without length or height, or whose centre line stands still between two knots."""
    if mode not in ('resize', 'pad'):
        raise NotImplementedError("strip crops support the batched modes 'resize' and 'pad' "
                                  "(keep_size / keep_ratio produce per-sample shapes)")
    if not isinstance(ribbon, Ribbon):
        raise TypeError("plan_strip takes a Ribbon, got %r" % (type(ribbon).__name__,))
    H, W = int(image_size[0]), int(image_size[1])
    c = ribbon.centres()
    seg = np.sqrt(((c[1:] - c[:-1]) ** 2).sum(axis=1))
    s = np.concatenate([[0.0], np.cumsum(seg)])
    w = float(s[-1])
    hgt = float(np.sqrt(((ribbon.top - ribbon.bottom) ** 2).sum(axis=1)).max())
    if not (w > 0.0 and hgt > 0.0 and np.isfinite(w) and np.isfinite(hgt) and bool((s[1:] > s[:-1]).all())):
        raise DegenerateQuad("strip crop: the ribbon %r has no length or no height" % (ribbon,))
    cw, ch = max(int(w), 1), max(int(hgt), 1)
    dst_w = W if mode == 'resize' else target_width('pad', (H, W), (ch, cw))
    return StripPlan(shape=(int(shape[0]), int(shape[1])), ribbon=ribbon, s=s, w=w, hgt=hgt, cw=cw, ch=ch, frame=(ch, cw),
                     canvas=(H, W), dst_w=int(dst_w), sx=1.0 / (float(dst_w) / float(cw)), sy=1.0 / (float(H) / float(ch)),
                     cu1=float(cw - 1), cv1=float(ch - 1))


StripLayout = namedtuple("StripLayout", "M I table_off desc_off index_off resident plans dropped")


class StripCropper(object):
    """`QuadCropper` for ribbons: `pack` / `upload` / `crop`, the shared `Staging` packer, resident CUDA photos used in place,
    one launch of mr_strip_crop per batch.  (No augmenter.)"""

    def __init__(self, image_size=(64, 512), mode='resize', device=None):
        if mode not in ('resize', 'pad'):
            raise NotImplementedError("StripCropper supports the batched modes 'resize' and 'pad' "
                                      "(keep_size / keep_ratio produce per-sample shapes)")
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.mode = mode
        self.device = torch.device(device if device is not None else "cuda")
        load()
        self._staging = Staging()

    def pack(self, images, ribbons, slot=0, plans=None):
        """Host side: plan every ribbon and lay the numpy photos, the photo table, the strip descriptors and the source indices
        (int32 [M]) out in ONE pinned staging buffer (per prefetch slot).  Photos that are CUDA tensors are not copied: their
        table entries are completed by `upload`.  `plans`: ready-made [(photo index, StripPlan)] in the place of the planning.
        Returns (pinned uint8 tensor, StripLayout)."""
        n = len(images)
        if plans is None and len(ribbons) != n:
            raise ValueError("StripCropper: %d images, %d ribbon lists" % (n, len(ribbons)))
        check_images(images, tensors=True)
        for im in images:
            if isinstance(im, torch.Tensor) and not im.is_cuda:
                raise TypeError("images are numpy arrays (staged and uploaded) or CUDA tensors (used in place)")
        kept, dropped = [], []
        if plans is None:
            for i, found in enumerate(ribbons):
                for k, ribbon in enumerate(found):
                    try:
                        kept.append((i, plan_strip(images[i].shape, ribbon, self.image_size, self.mode)))
                    except DegenerateQuad:
                        dropped.append((i, k))
        else:
            kept = [(int(i), plan) for i, plan in plans]
        for i, plan in kept:
            if not 0 <= i < n:
                raise ValueError("StripCropper: a crop names photo %d of %d" % (i, n))
            if tuple(plan.canvas) != self.image_size:
                raise ValueError("StripCropper: a plan onto %s for a canvas of %s" % (tuple(plan.canvas), self.image_size))
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
        descs = (StripDesc * max(M, 1))()
        for m, (i, plan) in enumerate(kept):
            plan.fill(descs[m], i)
        lay = Sections([im for _, im in staged_photos] + [table, descs, np.array([i for i, _ in kept], dtype=np.int32)],
                       pad_end=True)
        for (i, _), off in zip(staged_photos, lay.offsets):
            table[i].offset = off
        staged, _ = self._staging.stage(slot, lay)
        table_off, desc_off, index_off = lay.offsets[len(staged_photos):len(staged_photos) + 3]
        return staged, StripLayout(M, n, table_off, desc_off, index_off, resident, [plan for _, plan in kept], dropped)

    def upload(self, staged, layout):
        """One async H2D copy of the staging buffer, then the one launch, on the CURRENT stream (resident photos must be ready
        on it)."""
        H, W = self.image_size
        M = layout.M

        def place_resident(dbuf):
            table = staged.numpy()[layout.table_off:layout.table_off + layout.I * ctypes.sizeof(CropImage)]
            offsets = table.view(np.int64).reshape(layout.I, ctypes.sizeof(CropImage) // 8)[:, 0]
            for i, im in layout.resident:
                offsets[i] = im.data_ptr() - dbuf.data_ptr()
        dbuf = upload(staged, self.device, place_resident if layout.resident else None)
        image = torch.empty((M, 3, H, W), dtype=torch.float32, device=self.device)
        call("mr_strip_crop", ptr(dbuf), dbuf.data_ptr() + layout.table_off, layout.I, dbuf.data_ptr() + layout.desc_off, M,
             H, W, RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(image))
        index = dbuf[layout.index_off:layout.index_off + 4 * M].view(torch.int32)
        return {'image': image, 'index': index, 'dropped': list(layout.dropped),
                '_keepalive': (dbuf, [im for _, im in layout.resident])}

    def crop(self, images, ribbons):
        """images: uint8 HWC numpy arrays or uint8 HWC CUDA tensors; ribbons: a list of `Ribbon` per image.  Returns {'image': f32
        [M, 3, H, W], 'index': i32 [M], 'dropped': [(image, k)]} in input order."""
        staged, layout = self.pack(images, ribbons)
        return self.upload(staged, layout)
