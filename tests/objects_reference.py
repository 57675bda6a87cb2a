"""Independent restatement of `c3d_scene_objects` (include/change3d_hip.h) in numpy and plain Python: a flood fill started
at every still unlabelled foreground pixel in raster order (which numbers components by their first pixel, as
`scipy.ndimage.label` does), the `min_area` filter before numbering, the table, the votes with their tie rule, `score_q`
with the kernel's f32 rounding, and the truncation at `max_objects`.  Nothing here shares code with the kernels: no
union-find, no tiles."""
import numpy as np

NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def components(mask, connectivity=8):
    """int32 [H, W]: 0 for background, components numbered 1.. in raster order of their first pixel."""
    fg = np.asarray(mask) != 0
    H, W = fg.shape
    steps = NEIGHBOURS[connectivity]
    out = np.zeros((H, W), dtype=np.int32)
    fg_l, out_l = fg.tolist(), out.tolist()
    n = 0
    for y0 in range(H):
        row = fg_l[y0]
        for x0 in range(W):
            if not row[x0] or out_l[y0][x0]:
                continue
            n += 1
            out_l[y0][x0] = n
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and fg_l[yy][xx] and not out_l[yy][xx]:
                        out_l[yy][xx] = n
                        stack.append((yy, xx))
    return np.asarray(out_l, dtype=np.int32).reshape(H, W)


def filter_small(labels, min_area):
    """Components with fewer than `min_area` pixels removed, the rest renumbered 1.. in the same (raster) order."""
    n = int(labels.max())
    area = np.bincount(labels.ravel(), minlength=n + 1)
    keep = area >= max(int(min_area), 1)
    keep[0] = False
    new = np.zeros(n + 1, dtype=np.int32)
    new[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return new[labels]


def score_fixed(score):
    """u32 [H, W] = round-to-nearest-even(clip(p, 0, 1) * 65535) in f32; NaN counts as 0."""
    p = np.asarray(score, dtype=np.float32)
    p = np.where(np.isnan(p), np.float32(0), p)
    p = np.minimum(np.maximum(p, np.float32(0)), np.float32(1)).astype(np.float32)
    return np.rint(p * np.float32(65535.0)).astype(np.int64)


def vote(counts, first_class, ties="low"):
    """Class in [first_class, n) with the most votes; the lowest index on a tie (`ties="high"` is the wrong rule, kept for
    the negative control); 0 when nobody votes."""
    best, arg = 0, 0
    for c in range(first_class, len(counts)):
        if counts[c] > best or (ties == "high" and counts[c] == best and best > 0):
            best, arg = int(counts[c]), c
    return arg


def objects(mask, cls_map=None, score=None, connectivity=8, min_area=1, n_cls=1, first_class=1, max_objects=65536, ties="low",
            labels0=None):
    """`labels0`: `components(mask, connectivity)` where the caller already has it.  Returns dict(labels i32 [H, W], table i32 [max_objects, 8], hist u32-as-int64 [max_objects, n_cls] or None, object_cls u8 [H, W],
    counts i32 [2]) as the kernel defines them."""
    labels = filter_small(components(mask, connectivity) if labels0 is None else labels0, min_area)
    H, W = labels.shape
    n = int(labels.max())
    rows = min(n, max_objects)
    table = np.zeros((max_objects, 8), dtype=np.int32)
    hist = np.zeros((max_objects, n_cls), dtype=np.int64) if cls_map is not None else None
    q = score_fixed(score) if score is not None else None
    ys, xs = np.nonzero(labels)
    ids = labels[ys, xs]
    order = np.argsort(ids, kind="stable")
    ys, xs, ids = ys[order], xs[order], ids[order]
    bounds = np.searchsorted(ids, np.arange(1, n + 2))
    for k in range(rows):
        y, x = ys[bounds[k]:bounds[k + 1]], xs[bounds[k]:bounds[k + 1]]
        area = len(y)
        cls = 0
        if cls_map is not None:
            c = np.asarray(cls_map)[y, x]
            hist[k] = np.bincount(c[c < n_cls], minlength=n_cls)
            cls = vote(hist[k], first_class, ties)
        sq = 0
        if q is not None:
            sq = (int(q[y, x].sum()) + area // 2) // area
        table[k] = (area, x.min(), y.min(), x.max(), y.max(), cls, int((y * W + x).min()), sq)
    paint = np.zeros(max(n, max_objects) + 1, dtype=np.uint8)
    paint[1:rows + 1] = table[:rows, 5]
    return dict(labels=labels, table=table, hist=hist, object_cls=paint[labels], counts=np.array([n, rows], dtype=np.int32))


def mask_list(H, W, th, tw, seed=0):
    """The masks every scene size is tested with: list of (name, u8 [H, W])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = [("background", np.zeros((H, W), np.uint8)), ("foreground", np.ones((H, W), np.uint8)),
           ("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8))]
    out += [(f"random{d}", (rng.random((H, W)) < d).astype(np.uint8)) for d in (0.3, 0.59, 0.8)]
    # even rows full, odd rows joined at alternating ends: one component, the longest parent chains, across every seam
    snake = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == W - 1)) | ((yy % 4 == 3) & (xx == 0))
    out.append(("serpentine", snake.astype(np.uint8)))
    # the right arm starts in row 0, the left one in row 1, they meet in the last row only: the left arm's tiles learn
    # the smaller root late
    u = ((xx == W - 1) | ((xx == 0) & (yy >= min(1, H - 1))) | (yy == H - 1))
    out.append(("u", u.astype(np.uint8)))
    # corner to corner across the tile corner (th, tw): 8-connected lines whose pixels are 4-connected to nothing
    out.append(("diagonal", ((yy - th) == (xx - tw)).astype(np.uint8)))
    out.append(("antidiagonal", ((yy - th) + (xx - tw) == -1).astype(np.uint8)))
    return out
