"""Independent restatement of `c3d_scene_regions` (include/change3d_hip.h) in numpy and plain Python: a flood fill over
pixels of EQUAL key, started at every still unlabelled nonzero pixel in raster order, which numbers the regions by their
first pixel over all keys together.  The filter, the table, `score_q` and the truncation are those of
tests/objects_reference.py (the rule says "exactly those of c3d_scene_objects"); column 5 is the key.  Nothing here shares
code with the kernels: no union-find, no tiles."""
import numpy as np

import objects_reference as oref


def regions(key, connectivity=8):
    """int32 [H, W]: 0 where key is 0, the regions of equal key numbered 1.. in raster order of their first pixel."""
    key = np.asarray(key)
    H, W = key.shape
    steps = oref.NEIGHBOURS[connectivity]
    key_l = key.tolist()
    out_l = [[0] * W for _ in range(H)]
    n = 0
    for y0 in range(H):
        for x0 in range(W):
            k = key_l[y0][x0]
            if not k or out_l[y0][x0]:
                continue
            n += 1
            out_l[y0][x0] = n
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and key_l[yy][xx] == k and not out_l[yy][xx]:
                        out_l[yy][xx] = n
                        stack.append((yy, xx))
    return np.asarray(out_l, dtype=np.int32).reshape(H, W)


def region_objects(key, score=None, connectivity=8, min_area=1, max_objects=65536, labels0=None):
    """dict(labels, table, object_key, counts) as `c3d_scene_regions` defines them."""
    key = np.asarray(key, dtype=np.uint8)
    labels0 = regions(key, connectivity) if labels0 is None else labels0
    out = oref.objects(key, score=score, connectivity=connectivity, min_area=min_area, max_objects=max_objects, labels0=labels0)
    table = out["table"]
    rows = int(out["counts"][1])
    table[:rows, 5] = key.ravel()[table[:rows, 6]]
    return dict(labels=out["labels"], table=table, object_key=np.where(out["labels"] > 0, key, 0).astype(np.uint8),
                counts=out["counts"])
