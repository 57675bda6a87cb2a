"""Independent restatement of `c3d_rings_hull` (include/change3d_hip.h) in plain Python integers: which rows are used, the
point set of an id, the walk from the smallest (y, x), the rectangle of every hull edge compared as exact fractions by
cross-multiplication, the tables and the counts.  Nothing here shares code with the kernels: no tiers, no reductions, no
prefilter.  `tie="largest"` and `collinear="nearest"` are the two deliberately wrong variants of the negative controls."""
import numpy as np

ST_TRUNCATED, ST_BAD_COUNTS = 1, 2
ST_BAD_ROW, ST_HULL_TRUNCATED = 64, 128
COORD_MAX = 16384
INT32_MAX = 2 ** 31 - 1


def cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def hull(points, collinear="farthest"):
    """h[0 .. m-1] of the header's walk over the point set `points` = [(x, y), ...], not empty."""
    pts = sorted(set(points))
    h = [min(pts, key=lambda p: (p[1], p[0]))]
    for _ in range(len(pts)):
        cur = h[-1]
        ok = [q for q in pts if q != cur and all(cross(cur, q, r) >= 0 for r in pts)]
        if not ok:
            break
        d2 = lambda q: (q[0] - cur[0]) ** 2 + (q[1] - cur[1]) ** 2  # noqa: E731
        q = max(ok, key=d2) if collinear == "farthest" else min(ok, key=d2)
        if q == h[0]:
            break
        h.append(q)
    return h


def hull_fast(points):
    """The same hull by a monotone chain, for inputs where the quadratic walk above would take minutes; tests check that
    the two agree wherever both are run."""
    pts = sorted(set(points))
    if len(pts) <= 2:
        out = pts
    else:
        def half(seq):
            s = []
            for p in seq:
                while len(s) >= 2 and cross(s[-2], s[-1], p) <= 0:
                    s.pop()
                s.append(p)
            return s
        lower, upper = half(pts), half(pts[::-1])
        out = lower[:-1] + upper[:-1]
    k = out.index(min(out, key=lambda p: (p[1], p[0])))
    out = out[k:] + out[:k]
    if len(out) >= 3 and cross(out[0], out[1], out[2]) < 0:
        out = [out[0]] + out[:0:-1]
    return out


def edge_rect(h, k):
    """(k, L, t_min, t_max, c_max, j_tmin, j_tmax, j_cmax) of hull edge k."""
    m = len(h)
    P, Q = h[k], h[(k + 1) % m]
    d = (Q[0] - P[0], Q[1] - P[1])
    L = d[0] * d[0] + d[1] * d[1]
    t = [(p[0] - P[0]) * d[0] + (p[1] - P[1]) * d[1] for p in h]
    c = [cross(P, Q, p) for p in h]
    assert min(c) >= 0
    return (k, L, min(t), max(t), max(c), t.index(min(t)), t.index(max(t)), c.index(max(c)))


def rect(h, tie="smallest"):
    """The header's rectangle row of the hull h; (-1, 0, ...) below three vertices."""
    if len(h) < 3:
        return (-1, 0, 0, 0, 0, 0, 0, 0)
    best = None
    for k in range(len(h)):
        r = edge_rect(h, k)
        if best is None:
            best = r
            continue
        lhs, rhs = (r[3] - r[2]) * r[4] * best[1], (best[3] - best[2]) * best[4] * r[1]   # area_r < area_best, exactly
        if lhs < rhs or (lhs == rhs and tie == "largest"):
            best = r
    return best


def shoelace2(v):
    return sum(v[k - 1][0] * v[k][1] - v[k][0] * v[k - 1][1] for k in range(len(v)))


def classify(rings, vertices, counts, max_objects):
    """(points of every id as a dict id -> list, status bits added, K)."""
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    rows = min(max(int(counts[1]), 0), max_rings)
    limit = min(max(int(counts[3]), 0), max_vertices)
    V = vertices.tolist()
    points, status, K = {}, 0, 0
    for rid, start, n in rings[:rows, :3].tolist():
        if start < 0:
            continue
        ok = n >= 0 and start + n <= limit and 1 <= rid <= max_objects
        ring = [tuple(p) for p in V[start:start + n]] if ok else []
        if not ok or not all(0 <= c <= COORD_MAX for p in ring for c in p):
            status |= ST_BAD_ROW
            continue
        points.setdefault(rid, []).extend(ring)
        K = max(K, rid)
    return points, status, K


def hulls(rings, vertices, counts, max_objects, max_hull_vertices, tie="smallest", collinear="farthest", fast=False):
    """dict(hulls i32 [max_objects, 8], vertices i32 [max_hull_vertices, 2], rects i64 [max_objects, 8], counts i32 [5]) as
    the call defines them.  Vertex rows past counts[3] are zero here and left as they were there."""
    rings, vertices, counts = np.asarray(rings), np.asarray(vertices), np.asarray(counts)
    out_h = np.zeros((max_objects, 8), dtype=np.int32)
    out_v = np.zeros((max_hull_vertices, 2), dtype=np.int32)
    out_r = np.zeros((max_objects, 8), dtype=np.int64)
    status = int(counts[4])
    if status & ST_BAD_COUNTS:
        return dict(hulls=out_h, vertices=out_v, rects=out_r, counts=np.array([0, 0, 0, 0, ST_BAD_COUNTS], dtype=np.int32))
    points, added, K = classify(rings, vertices, counts, max_objects)
    status |= added
    at, written, truncated, with_points = 0, 0, False, 0
    for rid in range(1, K + 1):
        pts = points.get(rid, [])
        if not pts:
            out_h[rid - 1] = (rid, -1, 0, 0, 0, 0, 0, 0)
            out_r[rid - 1] = (-1, 0, 0, 0, 0, 0, 0, 0)
            continue
        with_points += 1
        h = hull_fast(pts) if fast else hull(pts, collinear)
        truncated = truncated or at + len(h) > max_hull_vertices
        out_h[rid - 1] = (rid, -1 if truncated else at, len(h), shoelace2(h), 0, h[0][0], h[0][1], min(len(pts), INT32_MAX))
        out_r[rid - 1] = rect(h, tie)
        if not truncated:
            out_v[at:at + len(h)] = h
            written = at + len(h)
        at += len(h)
    if truncated:
        status |= ST_HULL_TRUNCATED
    return dict(hulls=out_h, vertices=out_v, rects=out_r, counts=np.array([with_points, K, at, written, status], dtype=np.int32))


def rect_corners(P, d, row):
    """float64 [4, 2] corners, long side, short side and angle of a rectangle row on the hull edge from P along d: the host
    helper `ops.rect_corners` restated with fractions."""
    from fractions import Fraction as F
    _, L, t0, t1, c = (int(v) for v in row[:5])
    n = (-d[1], d[0])
    cs = []
    for t, s in ((t0, 0), (t1, 0), (t1, c), (t0, c)):
        cs.append((float(P[0] + F(d[0] * t + n[0] * s, L)), float(P[1] + F(d[1] * t + n[1] * s, L))))
    return cs, (t1 - t0) / L ** 0.5, c / L ** 0.5
