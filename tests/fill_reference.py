"""Independent restatement of `c3d_rings_fill` (include/change3d_hip.h): the per-pixel predicate -- active edge, strictly left
of the centre -- evaluated by brute force for every (edge, pixel) in numpy int64, counted per id, odd = inside, the largest
id wins.  No toggle columns and no prefix XOR: nothing here shares an idea with the kernels beyond the rule itself.
`inside_exact` is the same question asked of `fractions.Fraction`, for the CPU tests."""
from fractions import Fraction

import numpy as np

ST_BAD_COUNTS = 2                                        # C3D_OUTLINE_ST_BAD_COUNTS
ST_BAD_ID, ST_BAD_RING = 16, 32                          # C3D_FILL_ST_*
COORD_UNITS = 32768


def table(ring_lists, ids=None, max_rings=None, max_vertices=None, status=0):
    """(rings i32 [max_rings, 8], vertices i32 [max_vertices, 2], counts i32 [5]) holding the rings (lists of (vx, vy)) in
    order; ids default to 1, 2, ..."""
    ids = list(range(1, len(ring_lists) + 1)) if ids is None else list(ids)
    total = sum(len(v) for v in ring_lists)
    max_rings = len(ring_lists) + 1 if max_rings is None else max_rings
    max_vertices = total + 2 if max_vertices is None else max_vertices
    rings = np.zeros((max_rings, 8), dtype=np.int32)
    vertices = np.zeros((max_vertices, 2), dtype=np.int32)
    at = 0
    for r, v in enumerate(ring_lists):
        rings[r, :3] = (ids[r], at, len(v))
        if len(v):
            vertices[at:at + len(v)] = np.asarray(v, dtype=np.int64).reshape(-1, 2)
        at += len(v)
    counts = np.array([len(ring_lists), len(ring_lists), total, total, status], dtype=np.int32)
    return rings, vertices, counts


def ring_parity(verts, Hs, Ws, f, strict=True, winding=False, total=None):
    """i64 [Hs, Ws]: for every pixel the number of active edges of the ring left of its centre (with `winding` the signed
    number: +1 for an edge given downwards, -1 upwards), added into `total` where given."""
    s = 1 << f
    Cy = (2 * np.arange(Hs, dtype=np.int64) + 1) * s
    Cx = (2 * np.arange(Ws, dtype=np.int64) + 1) * s
    total = np.zeros((Hs, Ws), dtype=np.int64) if total is None else total
    n = len(verts)
    if n < 3:
        return total
    for k in range(n):
        (xa, ya), (xb, yb) = verts[k - 1], verts[k]
        sign = 1
        if ya > yb:
            xa, ya, xb, yb, sign = xb, yb, xa, ya, -1
        X0, Y0, X1, Y1 = 2 * int(xa), 2 * int(ya), 2 * int(xb), 2 * int(yb)
        if Y0 == Y1:
            continue
        rows = np.nonzero((Y0 <= Cy) & (Cy < Y1))[0]
        if rows.size == 0:
            continue
        lhs = (Cx[None, :] - X0) * (Y1 - Y0)
        rhs = (X1 - X0) * (Cy[rows, None] - Y0)
        left = lhs > rhs if strict else lhs >= rhs
        total[rows] += left.astype(np.int64) * (sign if winding else 1)
    return total


def classify(rings, vertices, counts, f, max_objects):
    """(used row indices, status bits added) by the header's rule."""
    max_rings, max_vertices = len(rings), len(vertices)
    rows = min(max(int(counts[1]), 0), max_rings)
    vlimit = min(max(int(counts[3]), 0), max_vertices)
    cmax = COORD_UNITS << f
    used, status = [], 0
    for r in range(rows):
        i, start, n = (int(v) for v in rings[r, :3])
        if start < 0:
            continue
        id_ok = 1 <= i <= max_objects
        ring_ok = n >= 0 and start + n <= vlimit
        if ring_ok and n:
            v = vertices[start:start + n].astype(np.int64)
            ring_ok = bool((np.abs(v) <= cmax).all())
        if id_ok and ring_ok:
            used.append(r)
        else:
            status |= (0 if id_ok else ST_BAD_ID) | (0 if ring_ok else ST_BAD_RING)
    return used, status


def fill(rings, vertices, counts, Hs, Ws, f=0, id_cls=None, max_objects=16, strict=True, winding=False):
    """dict(labels, table, counts_obj, mask, cls_map, info) as the call defines them."""
    rings, vertices, counts = np.asarray(rings), np.asarray(vertices), np.asarray(counts)
    labels = np.zeros((Hs, Ws), dtype=np.int32)
    tab = np.zeros((max_objects, 8), dtype=np.int32)
    if int(counts[4]) & ST_BAD_COUNTS:
        z = np.zeros((Hs, Ws), dtype=np.uint8)
        return dict(labels=labels, table=tab, counts_obj=np.array([-1, 0], dtype=np.int32), mask=z, cls_map=z.copy(),
                    info=np.array([int(counts[4]), 0, 0, 0], dtype=np.int32))
    used, status = classify(rings, vertices, counts, f, max_objects)
    per_id = {}
    for r in used:
        per_id.setdefault(int(rings[r, 0]), []).append(r)
    K = max(per_id) if per_id else 0
    for i in sorted(per_id):                             # ascending: the largest id paints last
        total = np.zeros((Hs, Ws), dtype=np.int64)
        for r in per_id[i]:
            start, n = int(rings[r, 1]), int(rings[r, 2])
            ring_parity([(int(x), int(y)) for x, y in vertices[start:start + n]], Hs, Ws, f, strict, winding, total)
        labels[total != 0 if winding else (total % 2) == 1] = i
    cls_map = np.zeros((Hs, Ws), dtype=np.uint8)
    for i in range(1, K + 1):
        cls = int(id_cls[i - 1]) if id_cls is not None else 0
        ys, xs = np.nonzero(labels == i)
        if len(ys):
            tab[i - 1] = (len(ys), xs.min(), ys.min(), xs.max(), ys.max(), cls, int((ys * Ws + xs).min()), 0)
            cls_map[ys, xs] = cls
        else:
            tab[i - 1, 5] = cls
    return dict(labels=labels, table=tab, counts_obj=np.array([K, K], dtype=np.int32), mask=(labels > 0).astype(np.uint8),
                cls_map=cls_map, info=np.array([int(counts[4]) | status, len(used), K, 0], dtype=np.int32))


def inside_exact(ring_lists, px, py, f):
    """Even-odd point-in-polygon of the pixel centre (px + 1/2, py + 1/2) in exact rationals: a crossing is an edge whose
    half-open y range [ya, yb) holds the centre's y and whose x at that y is strictly smaller than the centre's x."""
    s = 1 << f
    cx, cy = Fraction(2 * px + 1, 2), Fraction(2 * py + 1, 2)
    crossings = 0
    for verts in ring_lists:
        n = len(verts)
        if n < 3:
            continue
        for k in range(n):
            (xa, ya), (xb, yb) = (tuple(Fraction(int(c), s) for c in verts[k - 1]), tuple(Fraction(int(c), s) for c in verts[k]))
            if ya == yb:
                continue
            if ya > yb:
                xa, ya, xb, yb = xb, yb, xa, ya
            if ya <= cy < yb:
                x_at = xa + (xb - xa) * (cy - ya) / (yb - ya)
                crossings += x_at < cx
    return crossings % 2 == 1
