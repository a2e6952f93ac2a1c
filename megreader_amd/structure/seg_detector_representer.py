"""DB detector post-processing -- mirror of structure/representers/seg_detector_representer.py:10-168
(`SegDetectorRepresenter`: `represent`, `binarize`, `boxes_from_bitmap`, `box_score_fast`, `unclip`, `get_mini_boxes`)
with the per-pixel stages on the GPU (csrc/db_post.hip: connected components + hull candidates, box scores) and the
per-box geometry on the host (db_geometry.py).  Same constructor states, `represent(batch, pred)` contract and box
format (a list per image of [[x, y] * 4] lists, corners ordered top-left, top-right, bottom-right, bottom-left).

`device_geometry=True` runs the per-box geometry on the GPU as well (`mr_db_boxes`: hull, calipers, score, unclip and scaling
in one chain of launches that restates db_geometry.py in float64) and copies the finished boxes back once; the lists are the
same.  `boxes_on_device` is that chain without any copy, `represent_scored` also returns each box's confidence.

Differences, all forced by the build image having neither cv2 nor pyclipper to run the reference against ("parity
unpinned"; the restatement in oracle/db_post.py is the checker):
  * cv2.findContours(RETR_LIST) also returns the contours of HOLES; here a candidate is an 8-connected component (its
    outer contour).  Candidates are taken in raster order of their first pixel, the reference in cv2's order -- it only
    matters when an image has more than `max_candidates` components.
  * rectangles come from exact float64 calipers (cv2 works in float32), box scores count pixels inside or on the border
    of the integer-truncated box (cv2.fillPoly's scan conversion), unclip is the closed form for rectangles."""
import ctypes

import numpy as np
import torch

from .._lib import call, load, ptr, require_cuda
from .db_geometry import mini_box, unclip


class SegDetectorRepresenter(object):
    def __init__(self, thresh=0.3, box_thresh=0.7, max_candidates=100, resize=False, dest='binary', cmd={},
                 device_geometry=False, **kwargs):
        self.thresh, self.box_thresh, self.max_candidates = thresh, box_thresh, max_candidates
        self.resize, self.dest = resize, dest
        self.device_geometry = bool(device_geometry)
        self.min_size = 3
        self.scale_ratio = 0.4
        self.debug = cmd.get('debug', False)
        for k in ('thresh', 'box_thresh', 'dest'):
            if k in cmd:
                setattr(self, k, cmd[k])

    def represent(self, batch, _pred):
        """batch['image'] (N,C,H,W), batch['shape'][i] = (height, width) of the original image; _pred[dest] (N,1,H,W).
        Returns (boxes_batch, _pred) like the reference."""
        pred = _pred[self.dest]
        shapes = [tuple(int(v) for v in s) for s in batch['shape']]
        boxes_batch = self.boxes_from_maps(_pred['binary'], pred, shapes)
        return boxes_batch, _pred

    def represent_scored(self, batch, _pred):
        """`represent` with the confidence of every box (the mean of `binary` inside the box before unclip, the number
        `box_thresh` is compared with): (boxes_batch, scores_batch, _pred).  Always the device path; ONE device-to-host copy
        of one packed buffer."""
        shapes = [tuple(int(v) for v in s) for s in batch['shape']]
        boxes, scores, _ = self._fetch(self.boxes_on_device(_pred['binary'], _pred[self.dest], shapes))
        return boxes, scores, _pred

    def binarize(self, pred):
        return pred > self.thresh

    def boxes_from_bitmap(self, pred, _bitmap, dest_width, dest_height):
        """Single map, reference signature: pred (1,H,W) probabilities, _bitmap (1,H,W) binarised map."""
        assert _bitmap.size(0) == 1
        boxes = self.boxes_from_maps(pred.reshape(1, 1, *pred.shape[-2:]), None, [(dest_height, dest_width)],
                                     bitmap=_bitmap.reshape(1, 1, *_bitmap.shape[-2:]))[0]
        return boxes, _bitmap[0]

    def _maps(self, binary, dest_map, bitmap):
        """(map that is scored, map that is thresholded, threshold) as contiguous f32 tensors."""
        prob = binary.detach().float().contiguous()
        if bitmap is not None:
            return prob, bitmap.detach().float().contiguous(), 0.5
        return prob, (prob if dest_map is None else dest_map.detach().float().contiguous()), float(self.thresh)

    def boxes_on_device(self, binary, dest_map, shapes, bitmap=None):
        """The arguments of `boxes_from_maps`; everything stays on the device and nothing waits for it.  Returns
        {'boxes': f64 [N, K, 4, 2] the boxes of image n in its first count[n] slots (zeros behind), 'scores': f32 [N, K],
        'count': i32 [N], 'components': i32 [N] connected components of the image (more than K = max_candidates: the rest was
        not looked at), 'packed': the uint8 buffer all four are views of}."""
        return self._boxes_launch(binary, dest_map, shapes, bitmap)[0]

    def _boxes_launch(self, binary, dest_map, shapes, bitmap, front=0):
        """`boxes_on_device` with `front` free bytes (a multiple of 8) in front of the packed results: (its dict, the workspace
        mr_db_boxes left its labels, extremes and candidates in, dest on the device, (N, H, W, K))."""
        require_cuda(binary)
        prob, seg, thr = self._maps(binary, dest_map, bitmap)
        N, H, W = prob.shape[0], prob.shape[2], prob.shape[3]
        K = int(self.max_candidates)
        nbytes = ctypes.c_longlong(0)
        if load().mr_db_boxes_ws_bytes(N, H, W, K, ctypes.byref(nbytes)) != 0:
            raise RuntimeError("mr_db_boxes_ws_bytes failed: %s" % load().mr_last_error().decode())
        dev = prob.device
        dest = [(shapes[n][1], shapes[n][0]) if self.resize else (W, H) for n in range(N)]
        dest = torch.tensor(dest, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
        packed = torch.empty((front + N * K * 68 + N * 8,), dtype=torch.uint8, device=dev)
        out = self._views(packed[front:], N, K)
        call("mr_db_boxes", ptr(prob), ptr(seg), thr, ptr(dest), N, H, W, K, float(self.box_thresh), float(self.min_size),
             ptr(ws), ptr(out['boxes']), ptr(out['scores']), ptr(out['count']), ptr(out['components']), 0, 0, 0)
        out['packed'] = packed
        return out, ws, dest, (N, H, W, K)

    def ribbons_on_device(self, binary, dest_map, shapes, slabs=8, bitmap=None):
        """`boxes_on_device`, then `mr_db_ribbons` on the same workspace and stream: beside every box the curve its component
        follows (structure/ribbon.py), nothing copied, nothing waited for.  Returns what `boxes_on_device` returns and 'ribbons':
        f64 [N, K, 18, 2, 2] (knot, top / bottom, x / y; zeros behind the used knots), 'knots': i32 [N, K] (0: no ribbon, the box
        stands), 'why': i32 [N, K] (0 ribbon, 1 short, 2 empty slab, 3 steep, 4 folded), all views of 'packed'.  The box score is
        the mean over the RECTANGLE, of which a curved word fills a part: read curved text with a lower `box_thresh`."""
        if not 3 <= int(slabs) <= 16:
            raise ValueError("slabs must be in [3, 16] (MR_RIBBON_MAX_SLABS), got %r" % (slabs,))
        N, K = binary.shape[0], int(self.max_candidates)
        front = N * K * (self.RIBBON_KNOTS * 32 + 8)             # ribbons | knots | why in front of the boxes' results
        out, ws, dest, (N, H, W, K) = self._boxes_launch(binary, dest_map, shapes, bitmap, front=front)
        rbytes = ctypes.c_longlong(0)
        if load().mr_db_ribbons_ws_bytes(N, K, ctypes.byref(rbytes)) != 0:
            raise RuntimeError("mr_db_ribbons_ws_bytes failed: %s" % load().mr_last_error().decode())
        rws = torch.empty((rbytes.value,), dtype=torch.uint8, device=ws.device)
        out.update(self._ribbon_views(out['packed'][:front], N, K))
        call("mr_db_ribbons", ptr(dest), N, H, W, K, int(slabs), 1.5, ptr(ws), ptr(rws), ptr(out['ribbons']), ptr(out['knots']),
             ptr(out['why']))
        return out

    RIBBON_KNOTS = 18            # MR_RIBBON_MAX_KNOTS

    @classmethod
    def _ribbon_views(cls, packed, N, K):
        """The three results of mr_db_ribbons as views of one byte buffer: ribbons | knots | why."""
        o1, o2 = N * K * cls.RIBBON_KNOTS * 32, N * K * (cls.RIBBON_KNOTS * 32 + 4)
        return {'ribbons': packed[:o1].view(torch.float64).view(N, K, cls.RIBBON_KNOTS, 2, 2),
                'knots': packed[o1:o2].view(torch.int32).view(N, K), 'why': packed[o2:].view(torch.int32).view(N, K)}

    def represent_ribbons(self, batch, _pred, slabs=8):
        """`represent_scored` with a ribbon beside every box: (boxes_batch, scores_batch, ribbons_batch), per image a `Ribbon` in
        photo coordinates or None (the box stands) for every box.  Always the device path, as `represent_scored`; ONE
        device-to-host copy of one packed buffer."""
        from .ribbon import Ribbon
        shapes = [tuple(int(v) for v in s) for s in batch['shape']]
        out = self.ribbons_on_device(_pred['binary'], _pred[self.dest], shapes, slabs=slabs)
        N, K = out['scores'].shape
        host = out['packed'].cpu()
        front = N * K * (self.RIBBON_KNOTS * 32 + 8)
        box, rib = self._views(host[front:], N, K), self._ribbon_views(host[:front], N, K)
        counts = box['count'].tolist()
        knots, curves = rib['knots'].tolist(), rib['ribbons'].numpy()
        ribbons = [[Ribbon(curves[n, j, :knots[n][j], 0], curves[n, j, :knots[n][j], 1]) if knots[n][j] else None
                    for j in range(counts[n])] for n in range(N)]
        return ([box['boxes'][n, :counts[n]].tolist() for n in range(N)],
                [box['scores'][n, :counts[n]].tolist() for n in range(N)], ribbons)

    @staticmethod
    def _views(packed, N, K):
        """The four results as views of one byte buffer: boxes | scores | count | components."""
        o1, o2, o3 = N * K * 64, N * K * 68, N * K * 68 + N * 4
        return {'boxes': packed[:o1].view(torch.float64).view(N, K, 4, 2), 'scores': packed[o1:o2].view(torch.float32).view(N, K),
                'count': packed[o2:o3].view(torch.int32), 'components': packed[o3:].view(torch.int32)}

    def _fetch(self, out):
        """One copy of the packed results to the host -> (boxes_batch, scores_batch, components per image)."""
        N, K = out['scores'].shape
        host = self._views(out['packed'].cpu(), N, K)
        counts = host['count'].tolist()
        return ([host['boxes'][n, :counts[n]].tolist() for n in range(N)],
                [host['scores'][n, :counts[n]].tolist() for n in range(N)], host['components'].tolist())

    def boxes_from_maps(self, binary, dest_map, shapes, bitmap=None):
        """binary: the probability map scored for box confidence (N,1,H,W); dest_map: the map that is thresholded into
        regions (defaults to `binary`); bitmap: an already binarised map instead of dest_map."""
        require_cuda(binary)
        if self.device_geometry:
            return self._fetch(self.boxes_on_device(binary, dest_map, shapes, bitmap=bitmap))[0]
        prob, seg, thr = self._maps(binary, dest_map, bitmap)
        N, H, W = prob.shape[0], prob.shape[2], prob.shape[3]
        dev = prob.device
        labels = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        cap = max(4096, N * H * W // 8)
        while True:
            points = torch.empty((cap, 4), dtype=torch.int32, device=dev)
            count = torch.zeros((1,), dtype=torch.int32, device=dev)
            call("mr_db_components", ptr(seg), thr, ptr(labels), ptr(points), ptr(count), cap, N, H, W)
            k = int(count.item())
            if k <= cap:
                break
            cap = k
        pts = points[:k].cpu().numpy()
        # group the hull candidates by (image, component root); raster order of the roots
        comps = {}
        for n, root, x, y in pts.tolist():
            comps.setdefault((n, root), []).append((x, y))
        per_image = [[] for _ in range(N)]
        for (n, root) in sorted(comps):
            per_image[n].append(comps[(n, root)])
        cand = []          # (image, ordered box)
        for n in range(N):
            for contour in per_image[n][:self.max_candidates]:
                box, sside = mini_box(contour)
                if sside < self.min_size:
                    continue
                cand.append((n, box))
        boxes_batch = [[] for _ in range(N)]
        if not cand:
            return boxes_batch
        rows = np.array([[n] + [float(int(v)) for p in box for v in p] for n, box in cand], dtype=np.float32)
        bx = torch.from_numpy(rows).to(dev)
        out = torch.empty((len(cand), 2), dtype=torch.float32, device=dev)
        call("mr_db_box_scores", ptr(prob), ptr(bx), ptr(out), len(cand), N, H, W)
        sc = out.cpu().numpy()
        for (n, box), (s, c) in zip(cand, sc.tolist()):
            score = s / c if c > 0 else 0.0
            if self.box_thresh > score:
                continue
            box2, sside = mini_box(unclip(box))
            if sside < self.min_size + 2:
                continue
            dest_height, dest_width = shapes[n] if self.resize else (H, W)
            b = np.array(box2, dtype=np.float64)
            b[:, 0] = np.clip(np.round(b[:, 0] / W * dest_width), 0, dest_width)
            b[:, 1] = np.clip(np.round(b[:, 1] / H * dest_height), 0, dest_height)
            boxes_batch[n].append(b.tolist())
        return boxes_batch
