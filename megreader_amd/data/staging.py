"""The one place a staging buffer is laid out: what `DevicePipeline`, `DetectionPipeline` and `QuadCropper` share on the host.

A batch goes to the device as ONE byte buffer -- pixels, descriptor tables, points, text -- in one async copy.  The pipelines
declare its sections in order; every section starts 16-byte aligned, and the bytes between two sections are never written:

    lay = Sections(images + [descs, n * 4])             # numpy arrays, ctypes arrays, or byte counts still to be filled
    for d, off in zip(descs, lay.offsets): d.offset = off
    staged, views = staging.stage(slot, lay)            # arrays are copied in; views[i]: the uint8 bytes of section i
    dbuf = upload(staged, device)
"""
import ctypes

import numpy as np
import torch


def align16(n):
    return (n + 15) // 16 * 16


def check_images(images, tensors=False):
    """Every image is uint8 HWC with 3 channels: a numpy array, or (tensors=True) also a torch tensor."""
    for im in images:
        dtype = torch.uint8 if tensors and isinstance(im, torch.Tensor) else np.uint8
        if im.dtype != dtype or im.ndim != 3 or im.shape[2] != 3:
            raise TypeError("images must be uint8 HWC with 3 channels (cv2.imread(..., IMREAD_COLOR))")


def as_array(items):
    """An array, list or tensor of numbers -> float64 numpy array."""
    if isinstance(items, torch.Tensor):
        items = items.detach().cpu().numpy()
    return np.asarray(items, dtype=np.float64)


def as_quads(items, who):
    """One image's quadrilaterals (K x 4 x 2 array, list or tensor; K may be 0) -> float64 array [K, 4, 2].  `who` opens the
    error text: "DetectionPipeline takes"."""
    a = as_array(items)
    if a.size == 0 and a.ndim < 3:
        return np.zeros((0, 4, 2), dtype=np.float64)
    if a.ndim != 3 or a.shape[1:] != (4, 2):
        raise ValueError("%s quadrilaterals: expected K x 4 x 2 points per image, got shape %s" % (who, a.shape))
    return a


class Sections(object):
    """The layout of `sections` (each a numpy array, a ctypes array or a byte count) in order: `offsets`, one per section and
    every one a multiple of 16, and `total`, the end of the last section (pad_end: rounded up to 16 as well)."""

    def __init__(self, sections, pad_end=False):
        self.sections = list(sections)
        self.offsets = []
        end = 0
        for s in self.sections:
            self.offsets.append(align16(end))
            end = self.offsets[-1] + (s if isinstance(s, int) else s.nbytes if isinstance(s, np.ndarray) else ctypes.sizeof(s))
        self.total = align16(end) if pad_end else end


class Staging(object):
    """The host buffers of one pipeline, one per prefetch slot: pinned when CUDA is available, pageable otherwise, and
    reallocated only when a batch needs more bytes than the slot has."""

    def __init__(self):
        self._slots = {}

    def buffer(self, slot, nbytes):
        buf = self._slots.get(slot)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty((max(nbytes, 1),), dtype=torch.uint8)
            buf = self._slots[slot] = buf.pin_memory() if torch.cuda.is_available() else buf
        return buf

    def stage(self, slot, lay):
        """(the slot's buffer cut to lay.total, [uint8 numpy view of each section]).  Array sections are copied in (any strides,
        without a temporary); sections given as byte counts are the caller's to fill."""
        staged = self.buffer(slot, lay.total)[:lay.total]
        host = staged.numpy()
        views = []
        for s, off in zip(lay.sections, lay.offsets):
            if isinstance(s, int):
                views.append(host[off:off + s])
                continue
            if not isinstance(s, np.ndarray):
                s = np.frombuffer(s, dtype=np.uint8)
            views.append(host[off:off + s.nbytes])
            views[-1].view(s.dtype).reshape(s.shape)[...] = s
        return staged, views


def upload(staged, device, patch=None):
    """One device byte buffer and one async H2D copy of `staged` into it on the CURRENT stream.  `patch(dbuf)` runs between
    the two: for staged fields that depend on the buffer's own address."""
    dbuf = torch.empty((staged.numel(),), dtype=torch.uint8, device=device)
    if patch is not None:
        patch(dbuf)
    dbuf.copy_(staged, non_blocking=True)
    return dbuf
