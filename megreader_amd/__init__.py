"""megreader_amd -- MI355X (gfx950) native training hot path for MegReader's recognition models.

Host-side mirror of the reference's plugin interface (``backbones``, ``decoders``, ``ops``, ``apex.parallel``)
on top of a C-ABI HIP library (``include/megreader_hip.h``).  PyTorch supplies device memory, streams,
autograd bookkeeping and ``torch.distributed`` (RCCL); every arithmetic kernel on the path is hand-written HIP.
"""
import os

import torch

_compute_dtype = torch.bfloat16 if os.environ.get("MEGREADER_DTYPE", "bf16").lower() in ("bf16", "bfloat16") \
    else torch.float32


def set_compute_dtype(dtype):
    """Storage type of activations / MFMA operands: torch.bfloat16 (default) or torch.float32 (parity mode)."""
    global _compute_dtype
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("compute dtype must be torch.bfloat16 or torch.float32")
    _compute_dtype = dtype


def get_compute_dtype():
    return _compute_dtype


def __getattr__(name):
    """`megreader_amd.TextReader` (reader.py), `megreader_amd.QuadCropper` (data/quad_crop.py), `megreader_amd.StripCropper`
    (data/strip_crop.py), `megreader_amd.Ribbon` (structure/ribbon.py), `megreader_amd.DetectionTiler` (data/detection_tiles.py)
    and `megreader_amd.Lexicon` (ops/lexicon.py), imported on first use: they load the HIP library, which `import megreader_amd`
    alone does not."""
    if name == "TextReader":
        from .reader import TextReader
        return TextReader
    if name == "QuadCropper":
        from .data.quad_crop import QuadCropper
        return QuadCropper
    if name == "StripCropper":
        from .data.strip_crop import StripCropper
        return StripCropper
    if name == "Ribbon":
        from .structure.ribbon import Ribbon
        return Ribbon
    if name == "DetectionTiler":
        from .data.detection_tiles import DetectionTiler
        return DetectionTiler
    if name == "Lexicon":
        from .ops.lexicon import Lexicon
        return Lexicon
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


__all__ = ["set_compute_dtype", "get_compute_dtype", "DetectionTiler", "Lexicon", "QuadCropper", "Ribbon", "StripCropper",
           "TextReader"]
