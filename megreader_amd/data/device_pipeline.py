"""Input pipeline on the GPU.

The reference prepares every sample on the host -- cv2.resize of the float32 image (data/processes/resize_image.py:
29-38), mean subtraction / scaling / HWC->CHW (normalize_image.py:8-17), label encoding (concern/charsets.py:52-58,
make_recognition_label.py:11-24) -- in 2 DataLoader workers (data/data_loader.py:22) and moves the fp32 batch with a
blocking `.to(device)` (structure/model.py:173).  At > 70 k images/s per GPU that is the ceiling of any real run.
Here the host only hands over the DECODED uint8 pixels (4x fewer bytes than the fp32 batch) and the UTF-32 text:

    pipe = DevicePipeline(image_size=(32, 128), mode='resize', charset=charset)
    for batch in Prefetcher(loader_of_(images, texts), pipe):       # H2D copy + kernels of batch i+1 overlap step i
        step.copy_inputs(batch['image'], batch['label'], batch['length']); loss = step()

`process()` = one pinned staging copy (async, side stream) + mr_resize_normalize + mr_encode_labels.
Resize arithmetic follows cv2's float32 INTER_LINEAR path (csrc/image_sample.hip); cv2 itself is not available in the build
image, so that one piece is checked against the numpy restatement in oracle/pipeline.py ("parity unpinned").

`EncodedDevicePipeline` takes the step in front as well: it is handed the ENCODED files (what the reference's LMDB and msgpack
stores hold), the host reads only their JPEG headers, and the device decodes them (data/jpeg_decode.py, csrc/jpeg.hip) into the
buffer the resize kernel reads -- 5-10x fewer bytes over PCIe again, and no PIL call per sample.  Formats the device does not
decode (PNG, progressive JPEG, ...) still take the host path inside the same batch.
"""
import ctypes

import numpy as np
import torch

from .._lib import STRUCTS, call, load, ptr
from ..charsets import EnglishCharset
from .staging import Sections, Staging, check_images, upload

RGB_MEAN = (122.67891434, 116.66876762, 104.00698793)   # data/processes/normalize_image.py:9 (applied to BGR as is)


class ImgDesc(ctypes.Structure):
    """struct mr_img_desc of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_img_desc"]


_FOLDS_TO = None


def _folds_to():
    """{string u: [codepoints cp with chr(cp).upper() == u != chr(cp)]} over all of Unicode (surrogates excluded: they
    cannot be encoded as UTF-32 text).  One scan of the codepoints, about half a second, so once per process."""
    global _FOLDS_TO
    if _FOLDS_TO is None:
        inv = {}
        for cp in range(0x110000):
            if 0xD800 <= cp <= 0xDFFF:
                continue
            ch = chr(cp)
            up = ch.upper()
            if up != ch:
                inv.setdefault(up, []).append(cp)
        _FOLDS_TO = inv
    return _FOLDS_TO


def charset_table(charset):
    """Sorted (codepoint, id) arrays of a charset: exactly the codepoints cp with charset.index(chr(cp)) != unknown, and
    that id (concern/charsets.py:37-41).  Case sensitive: the single-character classes themselves.  Otherwise `index()`
    upper-cases the query, so cp maps to the class chr(cp).upper() when that is a class -- a class that is not its own
    upper case ('a' of EnglishPrintableCharset) is never a target and gets no entry under its own id.  None entries
    (blank, unknown) are skipped, and so are multi-character ones unless they are the upper case of a codepoint ('SS' in
    the alphabet ChineseCharset builds from a dictionary that holds 'ß')."""
    classes = {}
    for i in range(len(charset)):
        ch = charset[i]
        if isinstance(ch, str):
            classes[ch] = i                     # as the charset's own lookup table: the last of equal entries
    if getattr(charset, "case_sensitive", False):
        pairs = {ord(ch): i for ch, i in classes.items() if len(ch) == 1}
    else:
        folds_to = _folds_to()
        pairs = {}
        for ch, i in classes.items():
            if len(ch) == 1 and ch.upper() == ch:
                pairs[ord(ch)] = i
            for cp in folds_to.get(ch, ()):
                pairs[cp] = i
    cps = sorted(pairs)
    return np.array(cps, dtype=np.int32), np.array([pairs[c] for c in cps], dtype=np.int32)


def target_width(mode, image_size, shape):
    """_ResizeImage.get_image_size (resize_image.py:40-48)."""
    height, width = image_size
    if mode == 'keep_ratio':
        width = max(width, int(height / shape[0] * shape[1] / 32 + 0.5) * 32)
    if mode == 'pad':
        width = min(width, max(int(height / shape[0] * shape[1] / 32 + 0.5) * 32, 32))
    return width


class DevicePipeline(object):
    """augmenter: a `RecognitionAugmenter` (data/recognition_augment.py), or None: the batch is the bare resize.  With one,
    `pack` draws the batch's descriptor table (batch index: a counter of this pipeline, or `pack(..., index=)`) and stages it
    with an `mr_crop_image` table of the samples; `_kernels` runs mr_resize_normalize over the batch as before and then
    mr_rec_augment over the augmented rows, so the other rows keep their bits.  Labels and lengths are untouched."""

    def __init__(self, image_size=(32, 128), mode='resize', charset=None, max_size=32, device=None, augmenter=None):
        if mode not in ('resize', 'pad'):
            raise NotImplementedError("DevicePipeline supports the batched modes 'resize' and 'pad' "
                                      "(keep_size / keep_ratio produce per-sample shapes)")
        self.image_size = tuple(image_size)
        self.mode = mode
        self.charset = charset if charset is not None else EnglishCharset()
        self.max_size = max_size
        self.device = torch.device(device if device is not None else "cuda")
        load()
        cps, ids = charset_table(self.charset)
        self.tab_cp = torch.from_numpy(cps).to(self.device)
        self.tab_id = torch.from_numpy(ids).to(self.device)
        self.unknown = getattr(self.charset, "unknown", 1)
        self._staging = Staging()
        self.augmenter = augmenter
        self.index = 0                          # the next batch's number in the augmenter's stream
        self._copied = {}                       # slot -> the event behind the last H2D copy of its staging buffer

    def _describe(self, shapes):
        """The `ImgDesc` table of images of the given (h, w); the offsets are the caller's to fill."""
        H, W = self.image_size
        descs = (ImgDesc * len(shapes))()
        for d, shape in zip(descs, shapes):
            d.h, d.w, d.pitch = shape[0], shape[1], shape[1] * 3
            d.dst_w = W if self.mode == 'resize' else target_width('pad', self.image_size, shape)
            # cv2: inv_scale = (double)dsize / ssize; scale = 1. / inv_scale
            d.scale_x = 1.0 / (float(d.dst_w) / float(shape[1]))
            d.scale_y = 1.0 / (float(H) / float(shape[0]))
        return descs

    @staticmethod
    def _text(texts):
        """The two text sections: the UTF-32 codepoints of all strings back to back, and their int64 [n + 1] offsets."""
        cp = [np.frombuffer(t.encode('utf-32-le'), dtype=np.int32) for t in texts]
        offs = np.zeros(len(texts) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(c) for c in cp])
        return [np.concatenate(cp + [np.zeros(0, dtype=np.int32)]), offs]

    def _draw(self, shapes, slot, index):
        """With an augmenter: (the two further sections -- an `mr_crop_image` table, still to be filled from the `ImgDesc`
        entries, and the batch's descriptor table --, the rows it augments).  Also waits until the slot's last copy has run:
        the tables are drawn ahead of the device, and a slot must not be rewritten while its bytes are still to be copied."""
        from .quad_crop import CropImage
        if index is None:
            index, self.index = self.index, self.index + 1
        table, rows = self.augmenter.sample([s[:2] for s in shapes], self.image_size, self.mode, index)
        if self._copied.get(slot) is not None:
            self._copied[slot].synchronize()
        return [(CropImage * max(len(shapes), 1))(), table], rows

    @staticmethod
    def _fill_crop_images(table, descs):
        for t, d in zip(table, descs):
            t.offset, t.pitch, t.h, t.w, t.reserved = d.offset, d.pitch, d.h, d.w, 0

    def pack(self, images, texts, slot=0, index=None):
        """Host side: lay the decoded uint8 HWC images, their descriptors and the UTF-32 text out in ONE pinned
        staging buffer (per prefetch slot).  Returns (pinned uint8 tensor, layout tuple); element 4 of the layout is the
        `ImgDesc` array that was staged (`photos` reads it).  With an augmenter two further sections follow the text and the
        layout ends with (slot, M, offset of the crop-image table, offset of the descriptor table, rows)."""
        n = len(images)
        check_images(images)
        descs = self._describe([im.shape for im in images])
        if self.augmenter is None:
            lay = Sections(list(images) + [descs] + self._text(texts))
            for d, off in zip(descs, lay.offsets):
                d.offset = off
            staged, _ = self._staging.stage(slot, lay)
            return staged, (n,) + tuple(lay.offsets[n:]) + (descs,)
        extra, rows = self._draw([im.shape for im in images], slot, index)
        lay = Sections(list(images) + [descs] + self._text(texts) + extra)
        for d, off in zip(descs, lay.offsets):
            d.offset = off
        self._fill_crop_images(extra[0], descs)
        staged, _ = self._staging.stage(slot, lay)
        return staged, (n,) + tuple(lay.offsets[n:n + 3]) + (descs, (slot, len(rows)) + tuple(lay.offsets[n + 3:]) + (rows,))

    def upload(self, staged, layout):
        """One async H2D copy of the staging buffer, then the two kernels, on the CURRENT stream."""
        dbuf = upload(staged, self.device)
        self._mark_copied(layout)
        return self._kernels(dbuf, layout)

    def _mark_copied(self, layout):
        """With an augmenter: record the event `pack` waits for before it stages the same slot again."""
        if self.augmenter is not None:
            ev = self._copied[layout[-1][0]] = torch.cuda.Event()
            ev.record()

    def _kernels(self, dbuf, layout):
        """mr_resize_normalize and mr_encode_labels over the uploaded buffer."""
        n, desc_off, text_off, offs_off = layout[:4]
        H, W = self.image_size
        image = torch.empty((n, 3, H, W), dtype=torch.float32, device=self.device)
        call("mr_resize_normalize", ptr(dbuf), dbuf.data_ptr() + desc_off, n, H, W, RGB_MEAN[0], RGB_MEAN[1],
             RGB_MEAN[2], ptr(image))
        if self.augmenter is not None:
            _, M, table_off, aug_off, _ = layout[-1]
            call("mr_rec_augment", ptr(dbuf), dbuf.data_ptr() + table_off, n, dbuf.data_ptr() + aug_off, M, n, H, W,
                 RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(image))
        label = torch.empty((n, self.max_size), dtype=torch.int32, device=self.device)
        length = torch.empty((n,), dtype=torch.int32, device=self.device)
        call("mr_encode_labels", dbuf.data_ptr() + text_off, dbuf.data_ptr() + offs_off, n, self.max_size,
             ptr(self.tab_cp), ptr(self.tab_id), self.tab_cp.numel(), int(self.unknown), ptr(label), ptr(length))
        return {'image': image, 'label': label, 'length': length, '_keepalive': dbuf}

    @staticmethod
    def photos(batch, layout):
        """The uploaded photos as uint8 HWC views of the device buffer `upload` filled (batch: what it returned)."""
        dbuf = batch['_keepalive']
        return [dbuf[d.offset:d.offset + d.h * d.w * 3].view(d.h, d.w, 3) for d in layout[4]]

    def process(self, images, texts):
        staged, layout = self.pack(images, texts)
        return self.upload(staged, layout)


class EncodedDevicePipeline(DevicePipeline):
    """`DevicePipeline` fed with ENCODED image files: `pack(blobs, texts, slot=0)` / `upload` / `photos` / `process` have the
    same shape, so `Prefetcher` drives it unchanged.  The host reads only the JPEG headers (data/jpeg_decode.py: one C call per
    batch); the encoded bytes cross PCIe and the device decodes them (csrc/jpeg.hip) into the buffer that `mr_resize_normalize`
    reads.  What the device does not decode (PNG, progressive JPEG, ...; `JpegDecoder.plan`) is decoded on the host as before and
    staged as raw pixels beside the blobs.  The batch also carries 'jpeg_status', int32 [n] on the device: MR_JPEG_CORRUPT where
    an image's stream turned out to be damaged (nothing synchronises to look at it here).  Pixels are BGR, as the mean is.
    split_above: work items longer than that many bytes -- whole photos without restart markers -- are decoded by many lanes each
    (csrc/jpeg_split.hip) and `host_above` applies to the others only; None: every item is one wavefront's, as before."""

    def __init__(self, image_size=(32, 128), mode='resize', charset=None, max_size=32, device=None, host_above=None,
                 split_above=None, augmenter=None):
        super().__init__(image_size, mode, charset, max_size, device, augmenter)
        from .jpeg_decode import HOST_ABOVE, JpegDecoder
        self.decoder = JpegDecoder(self.device, 'BGR', HOST_ABOVE if host_above is None else host_above, split_above)

    def pack(self, blobs, texts, slot=0, index=None):
        """Host side: ONE staging buffer [blobs | plan | host-decoded pixels | descriptors | text], with an augmenter
        [... | crop-image table | augmentation descriptors] (the layout then ends as `DevicePipeline.pack`'s does).  The
        device buffer of `upload` is [staged bytes | workspace | decoded pixels]; the `ImgDesc` offsets point into its decoded region for the
        images the device decodes and at the staged pixels for the others.  Raises ValueError for blobs whose headers are
        corrupt."""
        from .jpeg_decode import plan_layout, stage_plan
        plan = self.decoder.plan(blobs)
        if plan.corrupt():
            raise ValueError("corrupt JPEG data at batch indices %s" % plan.corrupt())
        n = plan.n
        descs = self._describe([plan.shape(i) for i in range(n)])
        if self.augmenter is None:
            lay, jpeg = plan_layout(plan, [descs] + self._text(texts))
            at = dict(zip(sorted(plan.host), lay.offsets[lay.first:]))
            for i, d in enumerate(descs):
                d.offset = at[i] if i in at else jpeg[4] + plan.images[i].out_off
            staged, _ = stage_plan(plan, lay, self._staging, slot)
            return staged, (n,) + tuple(lay.offsets[-3:]) + (descs, jpeg)
        extra, rows = self._draw([plan.shape(i) for i in range(n)], slot, index)
        lay, jpeg = plan_layout(plan, [descs] + self._text(texts) + extra)
        at = dict(zip(sorted(plan.host), lay.offsets[lay.first:]))
        for i, d in enumerate(descs):
            d.offset = at[i] if i in at else jpeg[4] + plan.images[i].out_off
        self._fill_crop_images(extra[0], descs)
        staged, _ = stage_plan(plan, lay, self._staging, slot)
        return staged, (n,) + tuple(lay.offsets[-5:-2]) + (descs, jpeg, (slot, len(rows)) + tuple(lay.offsets[-2:]) + (rows,))

    def upload(self, staged, layout):
        """One device buffer, one async H2D copy of the staged part, then mr_jpeg_decode and the two kernels of
        `DevicePipeline`, on the CURRENT stream."""
        from .jpeg_decode import upload_and_launch
        dbuf, status = upload_and_launch(staged, layout[5], self.device)
        self._mark_copied(layout)
        batch = self._kernels(dbuf, layout)
        batch['jpeg_status'] = status
        return batch


class Prefetcher(object):
    """Iterates `(images, texts)` batches (DevicePipeline; `(images, polygons, ignore_tags)` for DetectionPipeline) from a
    host loader and yields device batches, keeping one batch in flight:
    the staging copy and the pipeline kernels of batch i+1 run on a side stream while the training step of batch i
    runs on the main stream (replaces the blocking `.to(device)` of structure/model.py:173)."""

    def __init__(self, loader, pipeline):
        self.loader = loader
        self.pipe = pipeline
        self.stream = torch.cuda.Stream(device=pipeline.device)

    def __iter__(self):
        it = iter(self.loader)
        slot = 0
        pending = None

        def launch(item, slot):
            staged, layout = self.pipe.pack(*item, slot=slot)   # (images, texts) / (images, polygons, ignore_tags)
            with torch.cuda.stream(self.stream):
                batch = self.pipe.upload(staged, layout)
                ev = torch.cuda.Event()
                ev.record(self.stream)
            return batch, ev

        for item in it:
            nxt = launch(item, slot)
            slot ^= 1
            if pending is not None:
                batch, ev = pending
                torch.cuda.current_stream().wait_event(ev)
                for t in batch.values():
                    t.record_stream(torch.cuda.current_stream())
                yield batch
                # the pinned slot of `pending` is reused two batches later: its H2D copy completed with `ev`
            pending = nxt
        if pending is not None:
            batch, ev = pending
            torch.cuda.current_stream().wait_event(ev)
            for t in batch.values():
                t.record_stream(torch.cuda.current_stream())
            yield batch
