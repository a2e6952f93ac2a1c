"""Detection metrics of the DB detector on the GPU (csrc/quad_measure.hip): what the reference's
`DetectionIoUEvaluator.evaluate_image` (concern/icdar2015_eval/detection/iou.py:13-179) computes with one shapely call per
(ground truth, detection) pair, for quadrilaterals, as two launches for a whole batch -- `mr_quad_iou` (validity, areas,
pairwise intersection and IoU) and `mr_quad_match` (don't-care sets, greedy matching, precision / recall / hmean).
The class with the reference's measurer contract is megreader_amd.structure.QuadMeasurer.  `polygon_measure` is the same for
simple polygons of up to 64 vertices (curved text): `mr_poly_iou` fills the same tables, `mr_quad_match` reads them unchanged;
its class is megreader_amd.structure.PolygonMeasurer."""
import numpy as np
import torch

from .._lib import call, ptr, require_cuda


class QuadOutputs(dict):
    """The outputs of `quad_measure` as a dict of device tensors.  They are views of ONE byte buffer (`packed`), so that
    `to_host()` brings all of them back with a single device-to-host copy."""

    def __init__(self, N, G, D, device):
        super().__init__()
        layout = [('gt_area', torch.float64, (N, G)), ('det_area', torch.float64, (N, D)),
                  ('inter', torch.float64, (N, G, D)), ('iou', torch.float64, (N, G, D)), ('scores', torch.float64, (N, 3)),
                  ('gt_valid', torch.int32, (N, G)), ('det_valid', torch.int32, (N, D)), ('counts', torch.int32, (N, 4)),
                  ('match_det', torch.int32, (N, G)), ('gt_dontcare', torch.int32, (N, G)),
                  ('det_dontcare', torch.int32, (N, D))]
        self.sections = []
        offset = 0
        for name, dtype, shape in layout:          # the f64 sections come first: every section starts aligned
            nbytes = int(np.prod(shape)) * (8 if dtype == torch.float64 else 4)
            self.sections.append((name, dtype, shape, offset, nbytes))
            offset += nbytes
        self.packed = torch.empty((offset,), dtype=torch.uint8, device=device)
        for name, dtype, shape, start, nbytes in self.sections:
            self[name] = self.packed[start:start + nbytes].view(dtype).view(shape)

    def to_host(self):
        """dict of numpy arrays of the same names: one device-to-host copy (it synchronises with the launches)."""
        host = self.packed.cpu().numpy()
        return {name: host[start:start + nbytes].view(np.float64 if dtype == torch.float64 else np.int32).reshape(shape)
                for name, dtype, shape, start, nbytes in self.sections}


def quad_measure(gt, gt_count, gt_ignore, det, det_count, iou_constraint=0.5, area_precision_constraint=0.5, out=None):
    """gt f64 [N, G, 4, 2], gt_count i32 [N], gt_ignore i32 [N, G], det f64 [N, D, 4, 2], det_count i32 [N] on the GPU
    (slots at and beyond the count are padding).  Two launches on the current stream.  Returns a dict of device tensors
    (`QuadOutputs`; `out`: one to write into instead of a new one):
      gt_valid i32 [N, G], det_valid i32 [N, D], gt_area f64 [N, G], det_area f64 [N, D], inter / iou f64 [N, G, D],
      counts i32 [N, 4] = (gtCare, detCare, detMatched, valid gts), scores f64 [N, 3] = (precision, recall, hmean),
      match_det i32 [N, G], gt_dontcare i32 [N, G], det_dontcare i32 [N, D] -- the last three by position in the lists of
      VALID quads (the reference's gtPols / detPols), -1 / 0 in the unused slots.
    Both comparisons are strict (`>`), as in the reference."""
    require_cuda(gt, gt_count, gt_ignore, det, det_count)
    if gt.dim() != 4 or det.dim() != 4 or tuple(gt.shape[2:]) != (4, 2) or tuple(det.shape[2:]) != (4, 2):
        raise RuntimeError("quad_measure expects gt [N, G, 4, 2] and det [N, D, 4, 2]")
    N, G = gt.shape[:2]
    D = det.shape[1]
    if det.shape[0] != N or tuple(gt_count.shape) != (N,) or tuple(det_count.shape) != (N,) or \
            tuple(gt_ignore.shape) != (N, G):
        raise RuntimeError("quad_measure: gt_count / det_count must be [N], gt_ignore [N, G], det [N, D, 4, 2]")
    gt = gt.to(torch.float64).contiguous()
    det = det.to(torch.float64).contiguous()
    gt_count = gt_count.to(torch.int32).contiguous()
    det_count = det_count.to(torch.int32).contiguous()
    gt_ignore = gt_ignore.to(torch.int32).contiguous()
    if out is None:
        out = QuadOutputs(N, G, D, gt.device)
    elif tuple(out['inter'].shape) != (N, G, D) or out.packed.device != gt.device:
        raise RuntimeError("quad_measure: `out` was made for another shape or device")
    call("mr_quad_iou", ptr(gt), ptr(gt_count), ptr(det), ptr(det_count), N, G, D, ptr(out['gt_valid']),
         ptr(out['det_valid']), ptr(out['gt_area']), ptr(out['det_area']), ptr(out['inter']), ptr(out['iou']))
    call("mr_quad_match", ptr(out['gt_valid']), ptr(out['det_valid']), ptr(gt_ignore), ptr(out['det_area']),
         ptr(out['inter']), ptr(out['iou']), N, G, D, float(iou_constraint), float(area_precision_constraint),
         ptr(out['counts']), ptr(out['scores']), ptr(out['match_det']), ptr(out['gt_dontcare']), ptr(out['det_dontcare']))
    return out


MAX_POLYGON_VERTS = 64          # MR_POLY_MAX_VERTS of include/megreader_hip.h


def polygon_measure(gt, gt_verts, gt_count, gt_ignore, det, det_verts, det_count, iou_constraint=0.5,
                    area_precision_constraint=0.5, out=None):
    """`quad_measure` for simple polygons of 3 .. V vertices each (curved text): gt f64 [N, G, V, 2], gt_verts i32 [N, G] (the
    vertices of each polygon; those at and beyond it are padding), gt_count i32 [N], gt_ignore i32 [N, G], det f64 [N, D, V, 2],
    det_verts i32 [N, D], det_count i32 [N] on the GPU; V <= 64.  Two launches on the current stream, `mr_poly_iou` (validity,
    areas, pairwise intersection and IoU; the rule is written out in include/megreader_hip.h) and the `mr_quad_match` of
    `quad_measure`, which reads only those tables.  Returns the same `QuadOutputs`."""
    require_cuda(gt, gt_verts, gt_count, gt_ignore, det, det_verts, det_count)
    if gt.dim() != 4 or det.dim() != 4 or gt.shape[3] != 2 or det.shape[3] != 2 or gt.shape[2] != det.shape[2]:
        raise RuntimeError("polygon_measure expects gt [N, G, V, 2] and det [N, D, V, 2] with one V")
    N, G, V = gt.shape[:3]
    D = det.shape[1]
    if det.shape[0] != N or tuple(gt_count.shape) != (N,) or tuple(det_count.shape) != (N,) or \
            tuple(gt_ignore.shape) != (N, G) or tuple(gt_verts.shape) != (N, G) or tuple(det_verts.shape) != (N, D):
        raise RuntimeError("polygon_measure: gt_count / det_count must be [N], gt_verts / gt_ignore [N, G], det_verts [N, D], "
                           "det [N, D, V, 2]")
    gt = gt.to(torch.float64).contiguous()
    det = det.to(torch.float64).contiguous()
    gt_verts, gt_count, gt_ignore, det_verts, det_count = (t.to(torch.int32).contiguous()
                                                           for t in (gt_verts, gt_count, gt_ignore, det_verts, det_count))
    if out is None:
        out = QuadOutputs(N, G, D, gt.device)
    elif tuple(out['inter'].shape) != (N, G, D) or out.packed.device != gt.device:
        raise RuntimeError("polygon_measure: `out` was made for another shape or device")
    call("mr_poly_iou", ptr(gt), ptr(gt_verts), ptr(gt_count), ptr(det), ptr(det_verts), ptr(det_count), N, G, D, V,
         ptr(out['gt_valid']), ptr(out['det_valid']), ptr(out['gt_area']), ptr(out['det_area']), ptr(out['inter']),
         ptr(out['iou']))
    call("mr_quad_match", ptr(out['gt_valid']), ptr(out['det_valid']), ptr(gt_ignore), ptr(out['det_area']),
         ptr(out['inter']), ptr(out['iou']), N, G, D, float(iou_constraint), float(area_precision_constraint),
         ptr(out['counts']), ptr(out['scores']), ptr(out['match_det']), ptr(out['gt_dontcare']), ptr(out['det_dontcare']))
    return out
