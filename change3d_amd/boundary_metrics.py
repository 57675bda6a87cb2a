"""Boundary scores of scene maps: how well the outlines of a predicted mask fit those of the ground truth, which neither the
per-pixel scores nor the object scores say.  The reference has no counterpart.

`BoundaryEvaluator.update(pred_mask, gt_mask)` adds the counts of one scene with `c3d_boundary_counts`, whose distances are the
exact squared Euclidean distance transform `c3d_scene_edt` of the masks in HBM:

    band       the pixels of a mask within `d` pixels of its background (Boundary IoU, Cheng et al., 2021)
    contour    the pixels of a mask that are 4-adjacent to background; a contour pixel is hit iff a contour pixel of the
               other mask lies within `tau` pixels (the boundary F-measure with a pixel tolerance)

With `border` (the default) the outside of the scene counts as background, so an object cut by the scene's edge has a boundary
there.  Everything stays on the device and nothing synchronises until `scores()`, which reads the accumulated integers back
once and does the arithmetic in float64 on the host:

    boundary_iou = inter / union    boundary_precision = hit_p / n_pc    boundary_recall = hit_g / n_gc
    boundary_f1 = 2 p r / (p + r)

each 0 where its denominator is 0.  The ratios are taken over the integers accumulated over ALL scenes, which is how the
reference accumulates its pixel scores; this is not the per-image mean that the Boundary IoU paper reports."""
import torch

from . import ops


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def scores_from_totals(totals):
    """The host arithmetic of `BoundaryEvaluator.scores()`: `totals` = (inter, union, n_pc, hit_p, n_gc, hit_g, scenes, 0) as
    integers.  float64 throughout."""
    inter, union, n_pc, hit_p, n_gc, hit_g, scenes = (int(v) for v in list(totals)[:7])
    p, r = _ratio(hit_p, n_pc), _ratio(hit_g, n_gc)
    return dict(inter=inter, union=union, n_pc=n_pc, hit_p=hit_p, n_gc=n_gc, hit_g=hit_g, scenes=scenes,
                boundary_iou=_ratio(inter, union), boundary_precision=p, boundary_recall=r, boundary_f1=_ratio(2.0 * p * r, p + r))


class BoundaryEvaluator:
    def __init__(self, d, tau=None, border=True, device=None):
        self.d, self.tau = float(d), float(d if tau is None else tau)
        if ops.boundary_radius2(self.d) < 1 or ops.boundary_radius2(self.tau) < 1:      # raises outside (0, 1024]
            raise ValueError(f"d and tau must be at least 1 pixel, got {d}, {tau}")
        self.border = bool(border)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.totals = torch.zeros(8, dtype=torch.int64, device=self.device)
        self.scenes = 0

    def reset(self):
        self.totals.zero_()
        self.scenes = 0

    def update(self, pred_mask_u8, gt_mask_u8):
        """Adds one scene; returns its `counts` i64 [8] on the device.  Both masks u8 [Hs, Ws], nonzero = object.  Does not
        synchronise."""
        for what, t in (("predicted mask", pred_mask_u8), ("ground-truth mask", gt_mask_u8)):
            if t.device != self.device:
                raise ValueError(f"the {what} is on {t.device}, the evaluator's totals are on {self.device}")
        pred_mask_u8, gt_mask_u8 = pred_mask_u8.contiguous(), gt_mask_u8.contiguous()
        counts = ops.boundary_counts(pred_mask_u8, gt_mask_u8, self.d, self.tau, border=self.border, totals=self.totals)
        self.scenes += 1
        return counts

    def scores(self):
        """The one synchronisation."""
        return scores_from_totals(self.totals.cpu().tolist())
