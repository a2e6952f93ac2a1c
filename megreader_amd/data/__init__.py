"""On-device input pipeline."""
from .device_pipeline import DevicePipeline, EncodedDevicePipeline, Prefetcher  # noqa: F401
from .jpeg_decode import JpegDecoder  # noqa: F401
from .detection_augment import AugmentPlan, DetectionAugmenter, WarpDesc  # noqa: F401
from .detection_pipeline import DetectionPipeline, EncodedDetectionPipeline  # noqa: F401
from .quad_crop import CropPlan, QuadCropper, plan_crop, rect_corners  # noqa: F401
from .detection_tiles import DetectionTiler, TilePlan, cover_1d, cover_owner  # noqa: F401
from .msgpack_records import UnpackMsgpackData, records_to_batch  # noqa: F401
from .synth_text import GlyphAtlas, SynthScenes, SynthStyle, SynthText  # noqa: F401
from .recognition_augment import RecognitionAugmenter, augment_crops  # noqa: F401
