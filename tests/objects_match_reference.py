"""Independent restatement of `c3d_objects_match` (include/change3d_hip.h) in numpy: `np.unique` over the pair keys of the two
label maps, the strict float64 comparison, the rows, the confusion matrix, the status rules and the host formulas of
`ObjectEvaluator.scores()`.  Nothing here shares code with the kernels: no hash table, no waves.  Also the mask pairs every
scene size is tested with (`mask_pairs`)."""
import numpy as np

ST_TABLE_FULL, ST_TRUNCATED, ST_BAD_COUNTS = 1, 2, 4


def _rows(counts, max_rows):
    return min(max(int(counts[1]), 0), int(max_rows))


def match(labels_p, table_p, counts_p, labels_g, table_g, counts_g, n_cls=1, iou_thr=0.5, strict=True, conf_gt_rows=True):
    """dict(match_p i32 [max_p, 4], match_g i32 [max_g, 4], conf i64 [n_cls, n_cls], counts i64 [6], sum_iou float, ious: list
    of the matched IoUs in ascending predicted id).  `strict=False` (>=) and `conf_gt_rows=False` (axes swapped) are the wrong
    rules, kept for the negative controls."""
    labels_p, labels_g = np.asarray(labels_p, dtype=np.int64), np.asarray(labels_g, dtype=np.int64)
    table_p, table_g = np.asarray(table_p), np.asarray(table_g)
    max_p, max_g = table_p.shape[0], table_g.shape[0]
    n_p, n_g = _rows(counts_p, max_p), _rows(counts_g, max_g)
    status = 0
    if counts_p[0] > counts_p[1] or counts_g[0] > counts_g[1] or counts_p[1] > max_p or counts_g[1] > max_g:
        status |= ST_TRUNCATED
    if counts_p[0] < 0 or counts_g[0] < 0:
        status |= ST_BAD_COUNTS
    both = (labels_p >= 1) & (labels_p <= n_p) & (labels_g >= 1) & (labels_g <= n_g)     # an id without a row is background
    keys, inters = np.unique((labels_p[both] << 32) | labels_g[both], return_counts=True)
    match_p, match_g = np.zeros((max_p, 4), dtype=np.int32), np.zeros((max_g, 4), dtype=np.int32)
    for key, inter in zip(keys.tolist(), inters.tolist()):
        p, g = key >> 32, key & 0xFFFFFFFF
        union = int(table_p[p - 1, 0]) + int(table_g[g - 1, 0]) - inter
        lhs, rhs = np.float64(inter), np.float64(iou_thr) * np.float64(union)
        if lhs > rhs or (not strict and lhs == rhs):
            match_p[p - 1, :3] = (g, inter, union)
            match_g[g - 1, :3] = (p, inter, union)
        match_p[p - 1, 3] += inter
        match_g[g - 1, 3] += inter

    def cls(table, k):
        c = int(table[k, 5])
        return c if 0 <= c < n_cls else 0

    conf = np.zeros((n_cls, n_cls), dtype=np.int64)
    ious = []
    for k in range(n_p):
        g = int(match_p[k, 0])
        if g:
            ious.append(np.float64(match_p[k, 1]) / np.float64(match_p[k, 2]))
            conf[cls(table_g, g - 1), cls(table_p, k)] += 1
        else:
            conf[0, cls(table_p, k)] += 1
    for k in range(n_g):
        if not match_g[k, 0]:
            conf[cls(table_g, k), 0] += 1
    if not conf_gt_rows:
        conf = conf.T.copy()
    tp = len(ious)
    counts = np.array([len(keys), tp, n_p - tp, n_g - tp, status, 0], dtype=np.int64)
    return dict(match_p=match_p, match_g=match_g, conf=conf, counts=counts, sum_iou=float(np.sum(np.array(ious, dtype=np.float64))),
                ious=ious)


def scores(results, n_cls):
    """The dict of `ObjectEvaluator.scores()` from a list of `match` results, written out once more."""
    tp = sum(int(r["counts"][1]) for r in results)
    fp = sum(int(r["counts"][2]) for r in results)
    fn = sum(int(r["counts"][3]) for r in results)
    pairs = sum(int(r["counts"][0]) for r in results)
    status = 0
    for r in results:
        status |= int(r["counts"][4])
    conf = np.zeros((n_cls, n_cls), dtype=np.int64)
    for r in results:
        conf += r["conf"]
    sum_iou = 0.0
    for r in results:
        sum_iou += r["sum_iou"]
    div = lambda a, b: a / b if b else 0.0  # noqa: E731
    sq, rq = div(sum_iou, tp), div(tp, tp + fp / 2 + fn / 2)
    class_f1 = [div(2.0 * conf[c, c], conf[:, c].sum() + conf[c, :].sum()) for c in range(1, n_cls)]
    return dict(tp=tp, fp=fp, fn=fn, pairs=pairs, precision=div(tp, tp + fp), recall=div(tp, tp + fn), f1=div(2.0 * tp, 2 * tp + fp + fn),
                sq=sq, rq=rq, pq=sq * rq, conf=conf, class_f1=class_f1, status=status)


def brute_force(labels_p, labels_g, n_p, n_g, iou_thr=0.5):
    """A double loop over object pairs on boolean masks: (matches [(p, g, inter, union)], covered_p, covered_g, pairs)."""
    labels_p, labels_g = np.asarray(labels_p), np.asarray(labels_g)
    masks_p = [labels_p == k for k in range(1, n_p + 1)]
    masks_g = [labels_g == k for k in range(1, n_g + 1)]
    any_p, any_g = (labels_p >= 1) & (labels_p <= n_p), (labels_g >= 1) & (labels_g <= n_g)
    matches, pairs = [], 0
    for p, mp in enumerate(masks_p):
        for g, mg in enumerate(masks_g):
            inter = int((mp & mg).sum())
            if not inter:
                continue
            pairs += 1
            union = int((mp | mg).sum())
            if inter / union > iou_thr:
                matches.append((p + 1, g + 1, inter, union))
    return matches, [int((m & any_g).sum()) for m in masks_p], [int((m & any_p).sum()) for m in masks_g], pairs


def _shift(mask, dy, dx):
    out = np.zeros_like(mask)
    H, W = mask.shape
    if dy < H and dx < W:
        out[dy:, dx:] = mask[:H - dy, :W - dx]
    return out


def _rectangles(H, W, rng):
    """Random 3..7 x 3..9 rectangles on a 9 x 11 pitch, clipped at the scene's edge: (mask, [(y, x, h, w)])."""
    mask, rects = np.zeros((H, W), np.uint8), []
    for y in range(0, H, 9):
        for x in range(0, W, 11):
            h, w = int(rng.integers(3, 8)), int(rng.integers(3, 10))
            mask[y:y + h, x:x + w] = 1
            rects.append((y, x, min(h, H - y), min(w, W - x)))
    return mask, rects


def mask_pairs(H, W, seed=0):
    """The mask pairs every scene size is tested with: list of (name, prediction u8 [H, W], ground truth u8 [H, W],
    connectivities the case is meant for)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base, rects = _rectangles(H, W, rng)
    cut = base.copy()                                      # a one-pixel column cut through every rectangle, off centre
    for y, x, h, w in rects:
        if w >= 3:
            cut[y:y + h, x + 1] = 0
    whole = (yy % 2 == 0) & (xx - xx % 6 + 4 <= W)                           # only where both runs fit into the scene
    runs_p = (whole & (xx % 6 < 3)).astype(np.uint8)                          # 3-pixel runs ..
    runs_g = (whole & (xx % 6 >= 1) & (xx % 6 < 4)).astype(np.uint8)          # .. overlapping in 2: IoU exactly 1/2
    empty = np.zeros((H, W), np.uint8)
    return [("identical", base, base.copy(), (4, 8)),
            ("shift1", base, _shift(base, 1, 1), (4, 8)),
            ("shift2", base, _shift(base, 2, 3), (4, 8)),
            ("split", cut, base, (4, 8)),
            ("merge", base, cut, (4, 8)),
            ("half", runs_p, runs_g, (4, 8)),
            ("checker_vs_full", ((yy + xx) % 2 == 0).astype(np.uint8), np.ones((H, W), np.uint8), (4,)),
            ("stripes", (yy % 2 == 0).astype(np.uint8) * np.ones((H, W), np.uint8), (xx % 2 == 0).astype(np.uint8), (4,)),
            ("random", (rng.random((H, W)) < 0.3).astype(np.uint8), (rng.random((H, W)) < 0.3).astype(np.uint8), (4, 8)),
            ("empty_prediction", empty, base, (4, 8)),
            ("empty_label", base, empty.copy(), (4, 8)),
            ("both_empty", empty, empty.copy(), (8,))]
