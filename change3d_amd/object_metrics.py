"""Object-level scores of scene maps: how many objects of the ground truth were found, missed and invented, and how well the
found ones fit.  The reference has no counterpart; its scores are per pixel.

`ObjectEvaluator.update(objects, gt_mask, gt_cls)` takes the `SceneObjects` of `SceneInferencer.predict(objects=True)`, labels
the ground truth with the same entry (`c3d_scene_objects`, votes over `gt_cls`, `first_class = 1`) and joins the two labelings
with `c3d_objects_match`: a predicted object and a ground-truth object match iff their IoU is strictly above `iou_thr` (>=
0.5, so a match is unique on both sides).  Everything stays on the device and nothing synchronises until `scores()`, which
reads the accumulated integers and the summed IoU back once and does the arithmetic in float64 on the host.
`update_labeled(objects, labels_g, table_g, counts_g)` is the same join for a ground truth that is already objects, such as
polygon labels filled by `c3d_rings_fill`:

    precision = TP / (TP + FP)    recall = TP / (TP + FN)    f1 = 2 TP / (2 TP + FP + FN)
    sq = sum_iou / TP    rq = TP / (TP + FP / 2 + FN / 2)    pq = sq * rq          (the panoptic-quality triple)

each 0 where its denominator is 0; `conf[gt class, predicted class]` counts matched pairs, missed objects in column 0 and
false alarms in row 0, and `class_f1[c - 1]` is the object F1 of class c >= 1 from it."""
import numpy as np
import torch

from . import _lib as L
from . import ops


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def scores_from_totals(totals, sum_iou, n_cls):
    """The host arithmetic of `ObjectEvaluator.scores()`: `totals` = (TP, FP, FN, pairs, status, conf row-major ...) as
    integers, `sum_iou` a float.  float64 throughout."""
    totals = [int(v) for v in totals]
    tp, fp, fn, pairs, status = totals[:5]
    conf = np.asarray(totals[5:5 + n_cls * n_cls], dtype=np.int64).reshape(n_cls, n_cls)
    sq = _ratio(float(sum_iou), tp)
    rq = _ratio(tp, tp + 0.5 * fp + 0.5 * fn)
    class_f1 = [_ratio(2 * int(conf[c, c]), int(conf[:, c].sum()) + int(conf[c, :].sum())) for c in range(1, n_cls)]
    return dict(tp=tp, fp=fp, fn=fn, pairs=pairs, precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn),
                f1=_ratio(2 * tp, 2 * tp + fp + fn), sq=sq, rq=rq, pq=sq * rq, conf=conf, class_f1=class_f1, status=status)


class ObjectEvaluator:
    def __init__(self, n_cls=1, iou_thr=0.5, connectivity=8, gt_min_area=1, max_objects=65536, device=None, table_capacity=0):
        if not 1 <= int(n_cls) <= 16 or not 0.5 <= float(iou_thr) < 1.0 or connectivity not in (4, 8) or int(max_objects) < 1:
            raise ValueError(f"n_cls in [1, 16], iou_thr in [0.5, 1), connectivity 4 or 8, max_objects positive; got {n_cls}, "
                             f"{iou_thr}, {connectivity}, {max_objects}")
        self.n_cls, self.iou_thr, self.connectivity = int(n_cls), float(iou_thr), int(connectivity)
        self.gt_min_area, self.max_objects, self.table_capacity = int(gt_min_area), int(max_objects), int(table_capacity)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # one buffer, one read-back: totals i64 [5 + n_cls^2], then the f64 IoU sum in the last word
        self._buf = torch.zeros(6 + self.n_cls ** 2, dtype=torch.int64, device=self.device)
        self.totals = self._buf[:-1]
        self.total_iou = self._buf[-1:].view(torch.float64)
        self.scenes = 0
        self.last_gt_counts = None          # counts i32 [2] of the last scene's ground-truth objects, on the device

    def reset(self):
        self._buf.zero_()
        self.scenes = 0

    def update(self, objects, gt_mask_u8, gt_cls_u8=None):
        """Adds one scene; returns its `(match_p, match_g)` device tensors.  `objects`: a `SceneObjects` (labels, table,
        counts are used); `gt_mask_u8` u8 [Hs, Ws], nonzero = object; `gt_cls_u8` u8 [Hs, Ws] or None.  Does not synchronise."""
        for what, t in (("ground-truth mask", gt_mask_u8), ("ground-truth class map", gt_cls_u8), ("labels", objects.labels),
                        ("table", objects.table), ("counts", objects.counts)):
            if t is not None and t.device != self.device:
                raise ValueError(f"the {what} is on {t.device}, the evaluator's totals are on {self.device}")
        gt_mask_u8 = gt_mask_u8.contiguous()
        if gt_cls_u8 is not None:
            gt_cls_u8 = gt_cls_u8.contiguous()
        labels_g, table_g, _, _, counts_g = ops.scene_objects(
            gt_mask_u8, gt_cls_u8, None, connectivity=self.connectivity, min_area=self.gt_min_area, n_cls=self.n_cls,
            first_class=1, max_objects=self.max_objects, want_hist=False, want_object_cls=False)
        match_p, match_g, _, _, _ = ops.objects_match(
            objects.labels, objects.table, objects.counts, labels_g, table_g, counts_g, n_cls=self.n_cls, iou_thr=self.iou_thr,
            table_capacity=self.table_capacity, totals=self.totals, total_iou=self.total_iou)
        self.scenes += 1
        self.last_gt_counts = counts_g
        return match_p, match_g

    def update_labeled(self, objects, labels_g, table_g, counts_g):
        """Adds one scene whose ground truth is already objects: the join of `update` without the relabelling.  `labels_g` i32
        [Hs, Ws], `table_g` i32 [max_g, 8] and `counts_g` i32 [2] as `c3d_scene_objects` or `c3d_rings_fill` write them
        (`ops.rings_fill` on polygon labels: touching buildings stay two objects).  Returns `(match_p, match_g)`; does not
        synchronise."""
        for what, t in (("ground-truth labels", labels_g), ("ground-truth table", table_g), ("ground-truth counts", counts_g),
                        ("labels", objects.labels), ("table", objects.table), ("counts", objects.counts)):
            if t.device != self.device:
                raise ValueError(f"the {what} are on {t.device}, the evaluator's totals are on {self.device}")
        match_p, match_g, _, _, _ = ops.objects_match(
            objects.labels, objects.table, objects.counts, labels_g, table_g, counts_g, n_cls=self.n_cls, iou_thr=self.iou_thr,
            table_capacity=self.table_capacity, totals=self.totals, total_iou=self.total_iou)
        self.scenes += 1
        self.last_gt_counts = counts_g
        return match_p, match_g

    def scores(self):
        """The one synchronisation.  Raises `Change3DHipError` where a scene set a status bit (C3D_MATCH_ST_*)."""
        host = self._buf.cpu()
        out = scores_from_totals(host[:-1].tolist(), float(host[-1:].view(torch.float64)[0]), self.n_cls)
        if out["status"]:
            names = [n for bit, n in ((L.MATCH_ST_TABLE_FULL, "pair table full"), (L.MATCH_ST_TRUNCATED, "objects past max_objects"),
                                      (L.MATCH_ST_BAD_COUNTS, "c3d_scene_objects reported an error")) if out["status"] & bit]
            raise L.Change3DHipError(f"c3d_objects_match status {out['status']}: {', '.join(names)}; the object scores are incomplete")
        return out
