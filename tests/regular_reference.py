"""Independent restatement of `c3d_rings_regularize` (include/change3d_hip.h) in plain Python integers: which rows are used,
the direction of an id, the frame, the edge classes, the runs, the levels as floor divisions of unbounded integers, the
vertices and the tables.  Nothing here shares code with the kernels: no tiers, no scans, no estimates.  `tie="strict"` (H iff
|dT| > |dC|) and `division="truncate"` are the two deliberately wrong variants of the negative controls."""
import math

import numpy as np

ST_TRUNCATED, ST_BAD_COUNTS = 1, 2
ST_BAD_ROW = 256
COORD_MAX = 16384


def _div(a, b, division):
    if division == "floor":
        return a // b
    q = abs(a) // b                                          # towards zero: the wrong variant
    return q if a >= 0 else -q


def direction(rid, hulls, hull_vertices, rects, counts_hull):
    """u = (u.x, u.y) of object `rid` (1 <= rid <= max_objects), or None."""
    max_objects, max_hull_vertices = hulls.shape[0], hull_vertices.shape[0]
    K = min(max(int(counts_hull[1]), 0), max_objects)
    limit = min(max(int(counts_hull[3]), 0), max_hull_vertices)
    if rid > K:
        return None
    k, start, m = int(rects[rid - 1, 0]), int(hulls[rid - 1, 1]), int(hulls[rid - 1, 2])
    if k < 0 or start < 0 or m < 3 or k >= m or start + m > limit:
        return None
    a, b = (tuple(int(c) for c in hull_vertices[start + j]) for j in (k, (k + 1) % m))
    if a == b or not all(0 <= c <= COORD_MAX for c in a + b):
        return None
    dx, dy = b[0] - a[0], b[1] - a[1]
    g = math.gcd(abs(dx), abs(dy))
    return dx // g, dy // g


def frame(p, u):
    return p[0] * u[0] + p[1] * u[1], p[1] * u[0] - p[0] * u[1]


def regular_ring(v, u, f, tie="ge", division="floor", info=None):
    """The regularised ring of v = [(x, y), ...] in units of 2^-f pixel, or None where the rule copies the ring.  `info`, a
    dict, receives the frame levels of the output vertices [(Tq, Cq), ...] and the runs [(class, W, A), ...]."""
    n = len(v)
    if n < 4 or any(v[k] == v[(k + 1) % n] for k in range(n)):
        return None
    S = 1 << f
    F = [frame(p, u) for p in v]
    dT = [F[(k + 1) % n][0] - F[k][0] for k in range(n)]
    dC = [F[(k + 1) % n][1] - F[k][1] for k in range(n)]
    H = [abs(dT[k]) >= abs(dC[k]) if tie == "ge" else abs(dT[k]) > abs(dC[k]) for k in range(n)]
    junctions = [k for k in range(n) if H[k - 1] != H[k]]
    R = len(junctions)
    if R < 4:
        return None
    levels, runs = [], []                                    # levels[j]: of the run that ends at junctions[j]
    for j in range(R):
        k, W, A = junctions[j - 1], 0, 0
        h = H[k]
        while k != junctions[j]:
            w = abs(dT[k]) if h else abs(dC[k])
            other = 1 if h else 0
            W += w
            A += w * (F[k][other] + F[(k + 1) % n][other])
            k = (k + 1) % n
        levels.append(_div(S * A + W, 2 * W, division))
        runs.append((h, W, A))
    N = u[0] * u[0] + u[1] * u[1]
    out, TC = [], []
    for j in range(R):
        behind, ahead = levels[j], levels[(j + 1) % R]
        Tq, Cq = (behind, ahead) if H[junctions[j]] else (ahead, behind)
        TC.append((Tq, Cq))
        out.append((_div(2 * (Tq * u[0] - Cq * u[1]) + N, 2 * N, division), _div(2 * (Tq * u[1] + Cq * u[0]) + N, 2 * N, division)))
    if info is not None:
        info.update(levels=TC, runs=runs, junctions=junctions)
    return out


def regularize(rings, vertices, counts, hulls, hull_vertices, rects, counts_hull, frac_bits, tie="ge", division="floor"):
    """dict(rings i32 [max_rings, 8], vertices i32 [max_vertices, 2], counts i32 [5]) as the call defines them.  Vertex rows
    past counts[3] are zero here and left as they were there."""
    rings, vertices, counts = np.asarray(rings), np.asarray(vertices), np.asarray(counts)
    hulls, hull_vertices, rects, counts_hull = (np.asarray(a) for a in (hulls, hull_vertices, rects, counts_hull))
    max_rings, max_vertices, max_objects = rings.shape[0], vertices.shape[0], hulls.shape[0]
    out_r = np.zeros((max_rings, 8), dtype=np.int32)
    out_v = np.zeros((max_vertices, 2), dtype=np.int32)
    status = int(counts[4]) | int(counts_hull[4])
    if status & ST_BAD_COUNTS:
        return dict(rings=out_r, vertices=out_v, counts=np.array([0, 0, 0, 0, status], dtype=np.int32))
    rows = min(max(int(counts[1]), 0), max_rings)
    limit = min(max(int(counts[3]), 0), max_vertices)
    S = 1 << frac_bits
    V = vertices.tolist()
    results = []                                             # per row: None (skipped) or (flag, vertices)
    for r in range(rows):
        rid, start, n = (int(c) for c in rings[r, :3])
        if start < 0:
            results.append(None)
            continue
        ok = n >= 0 and start + n <= limit and 1 <= rid <= max_objects
        ring = [tuple(p) for p in V[start:start + n]] if ok else []
        if not ok or not all(0 <= c <= COORD_MAX for p in ring for c in p):
            status |= ST_BAD_ROW
            results.append(None)
            continue
        u = direction(rid, hulls, hull_vertices, rects, counts_hull)
        new = regular_ring(ring, u, frac_bits, tie, division) if u is not None else None
        results.append((1, new) if new is not None else (0, [(x * S, y * S) for x, y in ring]))
    at, written, cut = 0, 0, False                           # rows that share vertices may not fit: skipped rows from there on
    for r in range(rows):
        row = rings[r]
        res = results[r]
        if res is not None and at + len(res[1]) > max_vertices:
            status |= ST_BAD_ROW
            cut = True
            at += len(res[1])
            res = None
        if res is None:
            out_r[r] = (row[0], -1, 0, 0, row[4], row[5], row[6], row[2])
            continue
        flag, new = res
        out_r[r] = (row[0], at, len(new), flag, row[4], row[5], row[6], row[2])
        out_v[at:at + len(new)] = np.array(new, dtype=np.int64).reshape(-1, 2)
        at += len(new)
        if not cut:
            written = at
    return dict(rings=out_r, vertices=out_v, counts=np.array([int(counts[0]), rows, written, written, status], dtype=np.int32))
