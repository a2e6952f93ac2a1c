"""Mirror of structure/measurers/quad_measurer.py:8-64 (`QuadMeasurer`: `measure` / `validate_measure` /
`evaluate_measure` / `gather_measure`) with the evaluator it wraps -- concern/icdar2015_eval/detection/iou.py
(`DetectionIoUEvaluator.evaluate_image`, `combine_results`) -- on the GPU: megreader_amd.ops.detection_measure, two
launches for a whole validation batch instead of shapely calls in Python loops per (ground truth, detection) pair.
Precision / recall / F-measure of the boxes `SegDetectorRepresenter.represent` returns.

Parity unpinned: shapely / GEOS is not a dependency and cannot be run beside this code, so
  * the validity rule is a RESTATEMENT of `Polygon(points).is_valid and .is_simple` for a 4-gon: the shoelace area is
    non-zero and neither pair of opposite edges (0-1 / 2-3, 1-2 / 3-0) intersects or touches;
  * results at exact ties (an IoU or a covered fraction equal to its constraint to the last bit) are not pinned: GEOS
    rounds differently from the triangle clipping used here.  Away from ties the areas are exact to float64 rounding
    (tests/test_quad_measure_gpu.py: within 1e-6 px^2 of a float64 restatement at coordinates up to 2048).
Only quadrilaterals are measured here; polygons with more points (curved text: 14-point annotations, ribbon outlines) go
through `PolygonMeasurer` (structure/polygon_measurer.py), which has this class's contract.
`iouMat` of an image without valid ground truths or without valid detections is `[]`; the reference returns an
uninitialised 1 x 1 array there."""
import numpy as np
import torch

from ..data.staging import as_array, as_quads
from ..ops.detection_measure import quad_measure
from .measurers import AverageMeter


def _quads(items):
    """`as_quads`, except that an empty array of ANY shape is no quadrilaterals (the strict rule refuses an empty `(0, 5, 2)`)."""
    a = as_array(items)
    return as_quads(a if a.size else (), "QuadMeasurer measures")


def _pad(per_image, width):
    out = np.zeros((len(per_image), width, 4, 2), dtype=np.float64)
    for i, a in enumerate(per_image):
        out[i, :len(a)] = a
    return out


class QuadMeasurer(object):
    def __init__(self, iou_constraint=0.5, area_precision_constraint=0.5, **kwargs):
        self.iou_constraint = iou_constraint
        self.area_precision_constraint = area_precision_constraint

    def measure(self, batch, output, device=None):
        """batch['polygons'] / batch['ignore_tags']: per image K_i x 4 x 2 points and K_i flags; output[0]: per image the
        boxes of the representer (possibly none).  Returns one dict per image with the reference's keys."""
        gts = [_quads(p) for p in batch['polygons']]
        dets = [_quads(p) for p in output[0]]
        if len(gts) != len(dets):
            raise ValueError("QuadMeasurer: %d images of ground truths, %d of detections" % (len(gts), len(dets)))
        N = len(gts)
        if N == 0:
            return []
        G, D = max(1, max(len(a) for a in gts)), max(1, max(len(a) for a in dets))
        ignore = np.zeros((N, G), dtype=np.int32)
        for i, tags in enumerate(batch['ignore_tags']):
            if isinstance(tags, torch.Tensor):
                tags = tags.detach().cpu().numpy()
            tags = np.asarray(tags).reshape(-1)[:len(gts[i])]
            ignore[i, :len(tags)] = tags != 0
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise NotImplementedError("megreader_amd's QuadMeasurer runs only on an AMD GPU (HIP). There is no CPU fallback.")
        up = [torch.from_numpy(a).to(dev) for a in (
            _pad(gts, G), np.array([len(a) for a in gts], dtype=np.int32), ignore,
            _pad(dets, D), np.array([len(a) for a in dets], dtype=np.int32))]
        r = quad_measure(*up, iou_constraint=self.iou_constraint,
                         area_precision_constraint=self.area_precision_constraint).to_host()
        return self.per_image_results(r, gts, dets)

    @staticmethod
    def per_image_results(r, gts, dets):
        """The reference's per-image dicts from the host copies of `quad_measure`'s outputs; gts / dets: the float64
        arrays [K_i, 4, 2] that were measured."""
        results = []
        for i in range(len(gts)):
            gi, di = np.nonzero(r['gt_valid'][i])[0], np.nonzero(r['det_valid'][i])[0]     # compacted -> given index
            ng, nd = len(gi), len(di)
            match = r['match_det'][i, :ng]
            if ng > 0 and 0 < nd <= 100:
                iou_mat = r['iou'][i][np.ix_(gi, di)].tolist()
            else:
                iou_mat = []
            results.append({
                'precision': float(r['scores'][i, 0]), 'recall': float(r['scores'][i, 1]), 'hmean': float(r['scores'][i, 2]),
                'pairs': [{'gt': g, 'det': int(d)} for g, d in enumerate(match) if d >= 0],
                'iouMat': iou_mat,
                'gtPolPoints': [gts[i][g] for g in gi], 'detPolPoints': [dets[i][d] for d in di],
                'gtCare': int(r['counts'][i, 0]), 'detCare': int(r['counts'][i, 1]),
                'gtDontCare': np.nonzero(r['gt_dontcare'][i, :ng])[0].tolist(),
                'detDontCare': np.nonzero(r['det_dontcare'][i, :nd])[0].tolist(),
                'detMatched': int(r['counts'][i, 2]),
            })
        return results

    def validate_measure(self, batch, output):
        return self.measure(batch, output), [0]

    def evaluate_measure(self, batch, output):
        n = batch['image'].shape[0] if 'image' in batch else len(batch['polygons'])
        return self.measure(batch, output), np.linspace(0, n).tolist()

    def gather_measure(self, raw_metrics, logger=None):
        raw_metrics = [image_metrics for batch_metrics in raw_metrics for image_metrics in batch_metrics]
        gt_care = sum(m['gtCare'] for m in raw_metrics)
        det_care = sum(m['detCare'] for m in raw_metrics)
        matched = sum(m['detMatched'] for m in raw_metrics)
        precision, recall, fmeasure = AverageMeter(), AverageMeter(), AverageMeter()
        precision.update(0 if det_care == 0 else float(matched) / det_care, n=len(raw_metrics))
        recall.update(0 if gt_care == 0 else float(matched) / gt_care, n=len(raw_metrics))
        fmeasure.update(2 * precision.val * recall.val / (precision.val + recall.val + 1e-8))
        return {'precision': precision, 'recall': recall, 'fmeasure': fmeasure}
