"""`QuadMeasurer`'s contract (`measure` / `validate_measure` / `evaluate_measure` / `gather_measure`, the same per-image dicts)
for POLYGONS of any vertex count: what the reference's `DetectionIoUEvaluator.evaluate_image`
(concern/icdar2015_eval/detection/iou.py:13-179) does with one shapely call per (ground truth, detection) pair when it is handed
more than four points -- the annotations of CTW1500 (14 points) and Total-Text, and the ribbon outlines that
`SegDetectorRepresenter.represent_ribbons` and `TextReader(curved=True)` return.  On the GPU: megreader_amd.ops.detection_measure
`polygon_measure`, two launches for a whole validation batch (`mr_poly_iou`, then the `mr_quad_match` of the quads).

Parity unpinned, as for quads: shapely / GEOS is not a dependency, so
  * the validity rule is a RESTATEMENT of `Polygon(points).is_valid and .is_simple` for a ring (include/megreader_hip.h: a finite
    non-zero shoelace area, no repeated vertex, no two non-adjacent edges that share a point, no edge folding back onto the one
    before it);
  * results at exact ties (an IoU or a covered fraction equal to its constraint to the last bit) are not pinned.  Away from ties
    the areas are exact to float64 rounding: the sum of signed triangle overlaps is an identity for simple polygons, convex or
    not (tests/test_polygon_measure_cpu.py checks the restatement against exact rational arithmetic)."""
import numpy as np
import torch

from ..ops.detection_measure import MAX_POLYGON_VERTS, polygon_measure
from .quad_measurer import QuadMeasurer
from .ribbon import Ribbon


def _collect(item, out):
    """Append the outlines `item` stands for to `out` as float64 arrays [k, 2]: a `Ribbon`, points [k, 2], a block [K, k, 2]
    (quads: [K, 4, 2]) or a list of any of these."""
    if isinstance(item, Ribbon):
        out.append(item.polygon())
        return
    if isinstance(item, torch.Tensor):
        item = item.detach().cpu().numpy()
    if not isinstance(item, np.ndarray):
        try:
            a = np.array(item, dtype=np.float64)
        except (TypeError, ValueError):                      # ragged, or it holds ribbons
            a = None
        if a is None:
            for sub in item:
                _collect(sub, out)
            return
        item = a
    a = np.asarray(item, dtype=np.float64)
    if a.size == 0:
        return
    if a.ndim == 2 and a.shape[1] == 2:
        out.append(a)
    elif a.ndim == 3 and a.shape[2] == 2:
        out.extend(a)
    else:
        raise ValueError("PolygonMeasurer measures outlines [k, 2], blocks [K, k, 2] and Ribbons, got an array of shape %s"
                         % (a.shape,))


def _polygons(items):
    out = []
    _collect(items, out)
    for a in out:
        if len(a) > MAX_POLYGON_VERTS:
            raise ValueError("PolygonMeasurer: a polygon of %d vertices exceeds the %d that mr_poly_iou measures "
                             "(MR_POLY_MAX_VERTS)" % (len(a), MAX_POLYGON_VERTS))
    return out


def _pad(per_image, width, V):
    points = np.zeros((len(per_image), width, V, 2), dtype=np.float64)
    verts = np.zeros((len(per_image), width), dtype=np.int32)
    for i, polys in enumerate(per_image):
        for k, a in enumerate(polys):
            points[i, k, :len(a)] = a
            verts[i, k] = len(a)
    return points, verts


def outlines_of(represented):
    """The per-image outline lists of `SegDetectorRepresenter.represent_ribbons`'s (boxes, scores, ribbons): for every box its
    ribbon's outline (top forward, bottom backward), or the box's four corners where the box stands -- what `TextReader(curved=
    True)` reports as 'polygon'.  `PolygonMeasurer().measure(batch, (outlines_of(represented),))` measures them."""
    boxes, _, ribbons = represented
    return [[np.array(box, dtype=np.float64) if ribbon is None else ribbon.polygon() for box, ribbon in zip(found, curves)]
            for found, curves in zip(boxes, ribbons)]


class PolygonMeasurer(QuadMeasurer):
    def measure(self, batch, output, device=None):
        """batch['polygons'] / batch['ignore_tags']: per image a list of outlines with any mix of vertex counts (points [k, 2],
        a block of quads [K, 4, 2], `Ribbon`s) and one flag per outline; output[0]: per image the detected outlines alike
        (possibly none).  Returns one dict per image with the reference's keys."""
        gts = [_polygons(p) for p in batch['polygons']]
        dets = [_polygons(p) for p in output[0]]
        if len(gts) != len(dets):
            raise ValueError("PolygonMeasurer: %d images of ground truths, %d of detections" % (len(gts), len(dets)))
        N = len(gts)
        if N == 0:
            return []
        G, D = max(1, max(len(a) for a in gts)), max(1, max(len(a) for a in dets))
        V = max([3] + [len(a) for polys in gts + dets for a in polys])       # the batch's largest polygon
        ignore = np.zeros((N, G), dtype=np.int32)
        for i, tags in enumerate(batch['ignore_tags']):
            if isinstance(tags, torch.Tensor):
                tags = tags.detach().cpu().numpy()
            tags = np.asarray(tags).reshape(-1)[:len(gts[i])]
            ignore[i, :len(tags)] = tags != 0
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise NotImplementedError("megreader_amd's PolygonMeasurer runs only on an AMD GPU (HIP). There is no CPU fallback.")
        gt, gt_verts = _pad(gts, G, V)
        det, det_verts = _pad(dets, D, V)
        up = [torch.from_numpy(a).to(dev) for a in (
            gt, gt_verts, np.array([len(a) for a in gts], dtype=np.int32), ignore,
            det, det_verts, np.array([len(a) for a in dets], dtype=np.int32))]
        r = polygon_measure(*up, iou_constraint=self.iou_constraint,
                            area_precision_constraint=self.area_precision_constraint).to_host()
        return self.per_image_results(r, gts, dets)
