"""Baseline JPEG decode on the GPU (csrc/jpeg.hip; include/megreader_hip.h: mr_jpeg_plan, mr_jpeg_decode).

The reference decodes every sample on the host (data/unpack_msgpack_data.py:28-35 with PIL, data/lmdb_dataset.py:80-88 with
cv2.imdecode).  Here the host reads only the marker segments of a batch -- one C call, `mr_jpeg_plan` -- and the encoded bytes go
to the device, where one wavefront per image (or per restart interval) does the entropy decode and the inverse DCT and a second
kernel the chroma upsampling and colour conversion.  The pixels equal PIL's / cv2's bit for bit (tests/_jpeg_ref.py).

    dec = JpegDecoder()                       # mode='BGR': cv2.imdecode's channel order
    images = dec.decode(list_of_bytes)        # uint8 HWC device tensors, views of one buffer

What the device does not decode -- progressive, arithmetic, CMYK, PNG, ... (`MR_JPEG_UNSUPPORTED`) -- is decoded on the host with
PIL as before and uploaded in the same staging copy.  An item is decoded by ONE wavefront unless the decoder is given
`split_above`: items longer than that many bytes -- a whole photo without restart markers is one -- are then cut into
sub-sequences of `subseq_bytes` that 256-lane workgroups decode in parallel (csrc/jpeg_split.hip: 2.5 ms for a 1280x720 photo
instead of 130 ms; CHANGELOG.md has the measurements).  Without `split_above`, a supported image one of whose items is longer
than `host_above` bytes goes to the host as well; with it, `host_above` applies only to the items that are still one wavefront's.
`EncodedDevicePipeline` (data/device_pipeline.py) puts the same plan in front of `DevicePipeline`'s resize and label kernels,
`EncodedDetectionPipeline` (data/detection_pipeline.py) in front of the detector's augmentation and target kernels.
"""
import ctypes
import io

import numpy as np
import torch

from .._lib import STRUCTS, _DEFINES, call, load
from .staging import Sections, Staging, align16

OK, UNSUPPORTED, CORRUPT = _DEFINES["MR_JPEG_OK"], _DEFINES["MR_JPEG_UNSUPPORTED"], _DEFINES["MR_JPEG_CORRUPT"]
# Bytes of one work item above which the image goes to the host decoder.  Measured on an MI355X (CHANGELOG.md, "Baseline JPEG decode
# on the GPU"): one wavefront decodes about 2.3 MB/s of entropy-coded data, so a 16 KiB item takes about 7 ms -- more than the 5 ms one
# host core needs for a whole 1280x720 photo.  Recognition crops (1-2 KB) and photos with a restart interval per MCU row (7 KB) stay below.
HOST_ABOVE = 16384
# The defaults of the two entry points that take whole photos as bytes (EncodedDetectionPipeline, TextReader(encoded=True)): a work
# item above SPLIT_ABOVE bytes is decoded by many lanes, SUBSEQ_BYTES unstuffed bytes each (csrc/jpeg_split.hip).  Measured on an
# MI355X (CHANGELOG.md, "Parallel JPEG decode of whole photos"; tools/bench_jpeg_split.py): a 1280x720 q90 photo without restart
# markers (314 KB, one item) decodes in 2.79 / 2.48 / 2.68 / 3.41 ms at 64 / 128 / 256 / 512 bytes per lane, against 130 ms by one
# wavefront and 5.2 ms by PIL on one host core, so such photos stay on the device; and a single-item file of 1.0 KB takes 0.37 ms
# by one wavefront against 0.49 ms split, one of 2.1 KB 0.75 ms against 0.53 ms: the paths cross between the two.
SPLIT_ABOVE = 2048
SUBSEQ_BYTES = 128


class JpegImage(ctypes.Structure):
    """struct mr_jpeg_image of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_jpeg_image"]


class JpegItem(ctypes.Structure):
    """struct mr_jpeg_item of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_jpeg_item"]


class JpegSplit(ctypes.Structure):
    """struct mr_jpeg_split of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_jpeg_split"]


ITEM_DTYPE = np.dtype([(name, np.int64 if ctype is ctypes.c_longlong else np.int32) for name, ctype in STRUCTS["mr_jpeg_item"]])


def host_decode(blob, mode='BGR'):
    """The host decoder (PIL), as data/msgpack_records.py and data/lmdb_reader.py use it: uint8 [H, W, 3]."""
    from PIL import Image
    rgb = np.array(Image.open(io.BytesIO(blob)).convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1]) if mode == 'BGR' else rgb


class JpegPlan(object):
    """The host plan of one batch: `images` (ctypes array of JpegImage, one per blob), `items` (the first `n_items` entries are
    the work items), the byte totals of the three device regions, and `host`: {index: uint8 HWC pixels} of the images the host
    decoded.  `status[i]` / `shape(i)` are what `JpegDecoder.plan` promises per image."""

    def __init__(self, blobs, images, items, totals):
        self.blobs = blobs
        self.n = len(blobs)
        self.images = images
        self.items = items
        self.n_items, self.blob_bytes, self.workspace_bytes, self.out_bytes = (int(t) for t in totals)
        self.host = {}
        self.splits, self.n_splits = None, 0        # the split table (`split`): items decoded by many lanes each

    @property
    def status(self):
        return [im.status for im in self.images]

    def shape(self, i):
        """(h, w) of image i: from the plan, or from the host decoder's pixels."""
        if i in self.host:
            return self.host[i].shape[:2]
        im = self.images[i]
        return (im.h, im.w) if im.status == OK else None

    def corrupt(self):
        return [i for i, im in enumerate(self.images) if im.status == CORRUPT]

    def sections(self):
        """The staged sections of the plan, in order: the blob buffer (a byte count, filled by `fill_blobs`), the image table and,
        directly behind it (its size is a multiple of 16), the work items: what mr_jpeg_decode takes as `plan_dev`.  A plan that
        was `split` carries a fourth section, its split table (mr_jpeg_decode_split's `splits_dev`)."""
        assert ctypes.sizeof(JpegImage) % 16 == 0
        items = (JpegItem * self.n_items).from_buffer(self.items) if self.n_items else 0
        return [self.blob_bytes, self.images, items] + ([self.split_table()] if self.n_splits else [])

    def split_table(self):
        return (JpegSplit * self.n_splits).from_buffer(self.splits)

    def split(self, split_above, subseq_bytes):
        """mr_jpeg_plan_split: every work item longer than `split_above` bytes gets an entry in the split table (and
        `reserved` = 1 + its index there), and the workspace grows by its regions.  Host only; once per plan."""
        assert self.splits is None, "a plan is split once"
        lib = load()
        if lib.mr_sizeof_jpeg_split() != ctypes.sizeof(JpegSplit):
            raise RuntimeError("mr_jpeg_split: the library and include/megreader_hip.h disagree -- rebuild it")
        self.splits = (JpegSplit * max(self.n_items, 1))()
        totals = (ctypes.c_longlong * 4)(self.n_items, self.blob_bytes, self.workspace_bytes, self.out_bytes)
        count = ctypes.c_longlong(0)
        if lib.mr_jpeg_plan_split(self.n, self.images, self.items, self.n_items, int(split_above), int(subseq_bytes), self.splits,
                                  self.n_items, totals, ctypes.byref(count)) != 0:
            raise RuntimeError("mr_jpeg_plan_split failed: %s" % lib.mr_last_error().decode())
        self.n_splits, self.workspace_bytes = int(count.value), int(totals[2])
        return self

    def fill_blobs(self, view):
        """Copy every blob the device reads to its planned offset in `view` (the staged blob buffer)."""
        for im, blob in zip(self.images, self.blobs):
            if im.status == OK:
                view[im.blob_off:im.blob_off + len(blob)] = np.frombuffer(blob, dtype=np.uint8)


def make_plan(blobs):
    """mr_jpeg_plan over a list of bytes: one C call for the batch (a second one only when the batch holds more restart intervals
    than the first guess has room for).  Host only: no GPU."""
    lib = load()
    if lib.mr_sizeof_jpeg_image() != ctypes.sizeof(JpegImage) or lib.mr_sizeof_jpeg_item() != ctypes.sizeof(JpegItem):
        raise RuntimeError("mr_jpeg_image / mr_jpeg_item: the library and include/megreader_hip.h disagree -- rebuild it")
    blobs = [b if isinstance(b, bytes) else bytes(b) for b in blobs]
    n = len(blobs)
    ptrs = (ctypes.c_char_p * n)(*blobs)
    lens = (ctypes.c_longlong * n)(*[len(b) for b in blobs])
    images = (JpegImage * n)()
    totals = (ctypes.c_longlong * 4)()
    room = n + 256
    while True:
        items = (JpegItem * room)()
        if lib.mr_jpeg_plan(n, ptrs, lens, images, items, room, totals) != 0:
            raise RuntimeError("mr_jpeg_plan failed: %s" % lib.mr_last_error().decode())
        if totals[0] <= room:
            return JpegPlan(blobs, images, items, totals)
        room = int(totals[0])


def launch(plan, dbuf, blob_off, plan_off, workspace_off, out_off, rgb, split_off=None):
    """mr_jpeg_decode over the regions of one device byte buffer, on the current stream: returns the int32 [n] status tensor.
    split_off: where the fourth section of a split plan was staged (mr_jpeg_decode_split)."""
    status = torch.empty((plan.n,), dtype=torch.int32, device=dbuf.device)
    base = dbuf.data_ptr()
    if plan.n_splits:
        call("mr_jpeg_decode_split", base + blob_off, base + plan_off, plan.n, plan.n_items, plan.split_table(), base + split_off,
             plan.n_splits, base + workspace_off, base + out_off, status.data_ptr(), 1 if rgb else 0)
    else:
        call("mr_jpeg_decode", base + blob_off, base + plan_off, plan.n, plan.n_items, base + workspace_off, base + out_off,
             status.data_ptr(), 1 if rgb else 0)
    return status


def plan_layout(plan, extra):
    """The staging layout [blobs | images | items | (split table) | host-decoded pixels | extra sections] of a plan: (lay, jpeg)
    with lay.first the index of the first host-pixel section and jpeg = (plan, blob_off, plan_off, workspace_off, out_off, total
    bytes of the device buffer [staged | workspace | decoded pixels], split_off).  `stage_plan` fills it."""
    sections = plan.sections()
    lay = Sections(sections + [plan.host[i] for i in sorted(plan.host)] + list(extra), pad_end=True)
    lay.first = len(sections)
    workspace_off = lay.total
    out_off = workspace_off + align16(plan.workspace_bytes)
    split_off = lay.offsets[3] if plan.n_splits else None
    return lay, (plan, lay.offsets[0], lay.offsets[1], workspace_off, out_off, out_off + plan.out_bytes, split_off)


def stage_plan(plan, lay, staging, slot):
    """Stage a `plan_layout` (array sections are copied in as they are NOW) and the blobs: (staged, views)."""
    staged, views = staging.stage(slot, lay)
    plan.fill_blobs(views[0])
    return staged, views


def upload_and_launch(staged, jpeg, device, rgb=False):
    """One device buffer [staged | workspace | decoded pixels], one async H2D copy of the staged part and the decode launches,
    on the current stream: (the buffer, the int32 [n] status tensor)."""
    plan, blob_off, plan_off, workspace_off, out_off, total, split_off = jpeg
    dbuf = torch.empty((total,), dtype=torch.uint8, device=device)
    dbuf[:staged.numel()].copy_(staged, non_blocking=True)
    return dbuf, launch(plan, dbuf, blob_off, plan_off, workspace_off, out_off, rgb, split_off)


class JpegDecoder(object):
    def __init__(self, device=None, mode='BGR', host_above=HOST_ABOVE, split_above=None, subseq_bytes=None):
        if mode not in ('BGR', 'RGB'):
            raise ValueError("mode must be 'BGR' or 'RGB'")
        self.mode = mode
        self.device = torch.device(device if device is not None else "cuda")
        self.host_above = host_above
        self.split_above = split_above              # None: no item is split (every item is one wavefront's)
        self.subseq_bytes = SUBSEQ_BYTES if subseq_bytes is None else int(subseq_bytes)
        if self.subseq_bytes % 4 or not 16 <= self.subseq_bytes <= 1024:
            raise ValueError("subseq_bytes must be a multiple of 4 in [16, 1024], got %r" % (subseq_bytes,))
        self._staging = Staging()

    def plan(self, blobs):
        """Host side, no GPU: the batch's `JpegPlan`.  Images the device does not decode (status MR_JPEG_UNSUPPORTED, or a work
        item above `host_above` bytes that is not split, which is then marked MR_JPEG_UNSUPPORTED as well) are decoded here with
        PIL into `plan.host`; images that break the JPEG syntax keep MR_JPEG_CORRUPT.  With `split_above` the plan carries the
        split table of the longer items."""
        plan = make_plan(blobs)
        if self.split_above is not None:
            plan.split(self.split_above, self.subseq_bytes)
        if self.host_above is not None:
            items = np.frombuffer(plan.items, dtype=ITEM_DTYPE, count=plan.n_items)
            for i in np.unique(items['image'][(items['len'] > self.host_above) & (items['reserved'] == 0)]):
                plan.images[i].status = UNSUPPORTED                  # its items stay in the list; the kernel skips them
        for i, im in enumerate(plan.images):
            if im.status == UNSUPPORTED:
                plan.host[i] = host_decode(plan.blobs[i], self.mode)
        return plan

    def decode(self, blobs, check=True, slot=0):
        """[uint8 HWC device tensor per blob], views of one buffer, on the current stream.  check=True: one read of the device
        status afterwards, ValueError naming the corrupt images.  check=False: no synchronisation; returns (tensors, int32 [n]
        device status) and the entry of an image the plan already found corrupt is None."""
        plan = self.plan(blobs)
        if check and plan.corrupt():
            raise ValueError("corrupt JPEG data at batch indices %s" % plan.corrupt())
        lay, jpeg = plan_layout(plan, [])
        staged, _ = stage_plan(plan, lay, self._staging, slot)
        dbuf, status = upload_and_launch(staged, jpeg, self.device, self.mode == 'RGB')
        out_off = jpeg[4]
        at = dict(zip(sorted(plan.host), lay.offsets[lay.first:]))
        out = []
        for i, im in enumerate(plan.images):
            if im.status == CORRUPT:
                out.append(None)
                continue
            h, w = plan.shape(i)
            off = at[i] if i in at else out_off + im.out_off
            out.append(dbuf[off:off + h * w * 3].view(h, w, 3))
        if not check:
            return out, status
        bad = torch.nonzero(status == CORRUPT).flatten().tolist()
        if bad:
            raise ValueError("corrupt JPEG data at batch indices %s" % bad)
        return out
