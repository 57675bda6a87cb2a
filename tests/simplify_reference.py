"""Independent restatement of `c3d_outlines_simplify` (include/change3d_hip.h) in plain Python integers: the segment distance
as a fraction, an explicit stack of chords, the two anchors, the third vertex of a collapsed ring, the table shapes and the
status rules.  Nothing here shares code with the kernels: no rounds, no reductions, no tiers.  `strict=False` and
`segment=False` are the two deliberately wrong variants of the negative controls."""
import numpy as np

ST_TRUNCATED, ST_BAD_COUNTS, ST_STEP_CAP, ST_BAD_INPUT = 1, 2, 4, 8
TOL2_Q_MAX = 16 * 1024 * 1024
COORD_MAX = 16384


def tol2_q(tol):
    q = int(round(16.0 * float(tol) * float(tol)))
    if not 0 <= q <= TOL2_Q_MAX:
        raise ValueError(f"tolerance {tol} outside [0, 1024]")
    return q


def distance(a, b, p, segment=True):
    """(num, den): the squared distance of p to the segment (a, b) -- to the line with segment=False -- is num / den."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    qx, qy = p[0] - a[0], p[1] - a[1]
    L2 = dx * dx + dy * dy
    if L2 == 0:
        return qx * qx + qy * qy, 1
    t = qx * dx + qy * dy
    if segment and t <= 0:
        return (qx * qx + qy * qy) * L2, L2
    if segment and t >= L2:
        return ((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2) * L2, L2
    c = dx * qy - dy * qx
    return c * c, L2


def simplify_ring(v, q, strict=True, segment=True, info=None):
    """Ascending indices of the kept vertices of the ring v = [(x, y), ...].  `info`, a dict, receives A, B, the depth and the
    list of (i, j, m, num, den) of every chord that was judged."""
    n = len(v)
    if n <= 3:
        return list(range(n))
    d = [(p[0] - v[0][0]) ** 2 + (p[1] - v[0][1]) ** 2 for p in v]
    B = d.index(max(d))                                  # the first of the largest
    w = list(v) + [v[0]]
    keep = {0, B}
    stack = [(B, n, 1), (0, B, 1)]
    depth, judged = 0, []
    while stack:
        i, j, level = stack.pop()
        if j <= i + 1:
            continue
        depth = max(depth, level)
        best, m, den = -1, -1, 1
        for k in range(i + 1, j):
            num, den = distance(w[i], w[j], w[k], segment)
            if num > best:                               # a tie keeps the smaller index
                best, m = num, k
        judged.append((i, j, m, best, den))
        far = 16 * best > q * den if strict else 16 * best >= q * den
        if far:
            keep.add(m)
            stack += [(m, j, level + 1), (i, m, level + 1)]
    if len(keep) <= 2:
        a, b = v[0], v[B]
        c = [abs((b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])) for p in v]
        keep.add(c.index(max(c)))
    if info is not None:
        info.update(A=0, B=B, depth=depth, judged=judged)
    return sorted(keep)


def shoelace2(v):
    """The shoelace sum as the call stores it: an i32, so modulo 2^32 for a ring that winds so often that the sum leaves it."""
    total = sum(v[k - 1][0] * v[k][1] - v[k][0] * v[k - 1][1] for k in range(len(v)))
    return (total + 2 ** 31) % 2 ** 32 - 2 ** 31


def simplify(rings, vertices, counts, q, strict=True, segment=True):
    """dict(rings i32 [max_rings, 8], vertices i32 [max_vertices, 2], counts i32 [5]) as the call defines them, from host
    arrays of the call's input shapes.  Vertex rows past counts[3] are zero here and left as they were there."""
    rings, vertices, counts = np.asarray(rings), np.asarray(vertices), np.asarray(counts)
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    assert 0 <= q <= TOL2_Q_MAX
    out_r = np.zeros((max_rings, 8), dtype=np.int32)
    out_v = np.zeros((max_vertices, 2), dtype=np.int32)
    found, rows_in, _, written_in, status = (int(c) for c in counts)
    if status & ST_BAD_COUNTS:
        return dict(rings=out_r, vertices=out_v, counts=np.array([0, 0, 0, 0, ST_BAD_COUNTS], dtype=np.int32))
    rows = min(max(rows_in, 0), max_rings)
    limit = min(max(written_in, 0), max_vertices)
    V = vertices.tolist()
    room = 0                                             # the n of the valid rows so far: their ranges must not overlap so
    at = 0                                               # far that they outgrow the vertex list
    for r, (rid, start, n, _, perimeter, x, y, _) in enumerate(rings[:rows].tolist()):
        kept = None
        if start >= 0:
            ok = n >= 0 and start + n <= limit
            if ok:
                ok = room + n <= max_vertices
                room += n
            ring = [tuple(p) for p in V[start:start + n]] if ok else []
            if ok and all(0 <= c <= COORD_MAX for p in ring for c in p):
                kept = [ring[k] for k in simplify_ring(ring, q, strict, segment)]
            else:
                status |= ST_BAD_INPUT
        if kept is None:
            out_r[r] = (rid, -1, 0, 0, perimeter, x, y, n)
            continue
        out_r[r] = (rid, at, len(kept), shoelace2(kept), perimeter, x, y, n)
        if kept:
            out_v[at:at + len(kept)] = kept
        at += len(kept)
    return dict(rings=out_r, vertices=out_v, counts=np.array([found, rows, at, at, status], dtype=np.int32))


def table(ring_lists, max_rings=None, max_vertices=None, ids=None):
    """(rings, vertices, counts) of the input shape from a list of rings [(x, y), ...]: what the outlines call would have
    written, with area = shoelace / 2 (floored) and perimeter = the ring's L1 length."""
    n_all = sum(len(v) for v in ring_lists)
    max_rings = max(1, len(ring_lists)) if max_rings is None else max_rings
    max_vertices = max(1, n_all) if max_vertices is None else max_vertices
    rings = np.zeros((max_rings, 8), dtype=np.int32)
    vertices = np.zeros((max_vertices, 2), dtype=np.int32)
    at = 0
    for r, v in enumerate(ring_lists):
        per = sum(abs(v[k][0] - v[k - 1][0]) + abs(v[k][1] - v[k - 1][1]) for k in range(len(v)))
        x, y = v[0] if v else (0, 0)
        rings[r] = (ids[r] if ids else r + 1, at, len(v), shoelace2(v) // 2, min(per, 2 ** 31 - 1), x, y, 0)
        if v:
            vertices[at:at + len(v)] = v
        at += len(v)
    counts = np.array([len(ring_lists), len(ring_lists), at, at, 0], dtype=np.int32)
    return rings, vertices, counts
