"""Polygon scores of scene maps: how far the predicted polygons lie from the labelled ones, pair by pair.  The reference has no
counterpart; its scores are per pixel.

`PolygonEvaluator.update(...)` takes what `ops.rings_polis` takes -- the ring table of the prediction, the ring table of the
ground truth, and the `match_p` of `ObjectEvaluator.update_labeled` -- and scores every matched pair with `c3d_rings_polis`:

    polis      the mean distance of the vertices of one polygon to the boundary of the other, averaged over the two
               directions (Avbelj et al., 2015), in pixels
    hausdorff  the largest of those vertex distances: the vertex-to-boundary form, NOT the Hausdorff distance of the two
               boundaries, whose maximum may fall inside an edge
    n_ratio    vertices of the prediction / vertices of the ground truth; 1 is best

Everything stays on the device and nothing synchronises until `scores()`, which reads the accumulated totals back once and
does the arithmetic in float64 on the host."""
import torch

from . import _lib as L
from . import ops


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def scores_from_totals(totals, total_sums):
    """The host arithmetic of `PolygonEvaluator.scores()`: `totals` = (scored, no partner, incomplete, over work, sum n_p,
    sum n_g, status, 0) as integers, `total_sums` = (sum polis, sum hausdorff, max hausdorff, sum n_p / n_g) as floats.
    float64 throughout; every mean is 0 without a scored pair."""
    pairs, no_partner, incomplete, over_work, n_p, n_g, status = (int(v) for v in list(totals)[:7])
    s = [float(v) for v in total_sums]
    return dict(pairs=pairs, polis=_ratio(s[0], pairs), hausdorff_mean=_ratio(s[1], pairs), hausdorff_max=s[2] if pairs else 0.0,
                n_ratio=_ratio(s[3], pairs), vertices=n_p, vertices_gt=n_g, no_partner=no_partner, incomplete=incomplete,
                over_work=over_work, status=status)


class PolygonEvaluator:
    def __init__(self, max_pair_work=2 ** 32, device=None):
        if not 0 <= int(max_pair_work) < 2 ** 63:
            raise ValueError(f"max_pair_work must lie in [0, 2^63), got {max_pair_work}")
        self.max_pair_work = int(max_pair_work)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # one buffer, one read-back: totals i64 [8], then the four f64 sums
        self._buf = torch.zeros(12, dtype=torch.int64, device=self.device)
        self.totals = self._buf[:8]
        self.total_sums = self._buf[8:].view(torch.float64)
        self.scenes = 0

    def reset(self):
        self._buf.zero_()
        self.scenes = 0

    def update(self, rings_p, vertices_p, counts_p, frac_bits_p, rings_g, vertices_g, counts_g, frac_bits_g, match_p, max_g):
        """Adds one scene; returns its `(pair, pair_n, counts, sums)` device tensors.  Does not synchronise."""
        for what, t in (("predicted rings", rings_p), ("ground-truth rings", rings_g), ("match", match_p)):
            if t.device != self.device:
                raise ValueError(f"the {what} are on {t.device}, the evaluator's totals are on {self.device}")
        out = ops.rings_polis(rings_p, vertices_p, counts_p, frac_bits_p, rings_g, vertices_g, counts_g, frac_bits_g, match_p, max_g,
                              max_pair_work=self.max_pair_work, totals=self.totals, total_sums=self.total_sums)
        self.scenes += 1
        return out

    def scores(self):
        """The one synchronisation.  Raises `Change3DHipError` where a scene set a status bit."""
        host = self._buf.cpu()
        out = scores_from_totals(host[:8].tolist(), host[8:].view(torch.float64).tolist())
        if out["status"]:
            raise L.Change3DHipError(f"c3d_rings_polis status {out['status']}: a ring table came with a status bit or match_p named a "
                                     f"partner outside the ground truth (bit {L.POLIS_ST_BAD_PARTNER}); the polygon scores are incomplete")
        return out
