"""Independent restatement of `c3d_outlines_simplify_shared` (include/change3d_hip.h) in plain Python: the four labels round a
lattice point, a walk along every stored edge, an explicit stack of chords per arc, the closed-arc guard, and the table and
status rules.  The distances of one chord are taken for all its vertices at once in numpy int64 (`distances`, held against the
scalar `simplify_reference.distance` by tests/test_shared_cpu.py), so that a comb of 5800 vertices and 2900 levels takes a second.
Nothing here shares code with the kernels: no bitmaps, no scans, no rounds, no tiers.  `tie="index"` and `insert_nodes=False` are
the two deliberately wrong variants of the negative controls."""
import numpy as np

from simplify_reference import COORD_MAX, ST_BAD_COUNTS, ST_BAD_INPUT, ST_TRUNCATED, TOL2_Q_MAX, distance, shoelace2, tol2_q  # noqa: F401


class Labels:
    """l(y, x) of the rule: the label if the pixel is in the scene and 1 <= value <= rows, else 0."""

    def __init__(self, labels, counts_obj, max_objects):
        lab = np.asarray(labels)
        self.H, self.W = lab.shape
        self.L = lab.tolist()
        self.rows = min(max(int(counts_obj[1]), 0), int(max_objects))

    def at(self, y, x):
        if 0 <= y < self.H and 0 <= x < self.W:
            v = self.L[y][x]
            return v if 1 <= v <= self.rows else 0
        return 0

    def is_node(self, vx, vy):
        a, b, c, d = self.at(vy - 1, vx - 1), self.at(vy - 1, vx), self.at(vy, vx - 1), self.at(vy, vx)
        return (a != b) + (c != d) + (a != c) + (b != d) >= 3

    def left(self, vx, vy, dx, dy):
        """The label left of the unit edge that leaves (vx, vy) in direction (dx, dy), the object on the right, y down."""
        if dx > 0:
            return self.at(vy - 1, vx)
        if dy > 0:
            return self.at(vy, vx)
        if dx < 0:
            return self.at(vy, vx - 1)
        return self.at(vy - 1, vx - 1)


def augment(ring, lab, insert_nodes=True):
    """[(x, y, node, left, inserted)] of the ring [(x, y), ...] in stored order, or None for bad input."""
    n = len(ring)
    if n < 4:
        return None
    for x, y in ring:
        if not (0 <= x <= lab.W and 0 <= y <= lab.H and x <= COORD_MAX and y <= COORD_MAX):
            return None
    out = []
    for k in range(n):
        (x0, y0), (x1, y1) = ring[k], ring[(k + 1) % n]
        if (x0 != x1) == (y0 != y1):                     # zero, or not parallel to an axis
            return None
        dx, dy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
        out.append((x0, y0, lab.is_node(x0, y0), lab.left(x0, y0, dx, dy), False))
        x, y = x0 + dx, y0 + dy
        while (x, y) != (x1, y1):
            if insert_nodes and lab.is_node(x, y):
                out.append((x, y, True, lab.left(x, y, dx, dy), True))
            x, y = x + dx, y + dy
    return out


def rotate(aug):
    nodes = [k for k, a in enumerate(aug) if a[2]]
    s = nodes[0] if nodes else min(range(len(aug)), key=lambda k: (aug[k][1], aug[k][0]))
    return aug[s:] + aug[:s]


def _farthest(values, keys, order):
    """The position of the largest of `values` (an int64 array); ties to the smallest of `keys` = vy * 16385 + vx, or to the first
    position with order="index"."""
    cand = np.flatnonzero(values == values.max())
    return int(cand[0]) if order == "index" else int(cand[np.argmin(keys[cand])])


def distances(a, b, X, Y):
    """(num i64 [len(X)], den): `distance` for all the points (X, Y) at once; every product stays below 2^60."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    qx, qy = X - a[0], Y - a[1]
    L2 = dx * dx + dy * dy
    pa2 = qx * qx + qy * qy
    if L2 == 0:
        return pa2, 1
    t = qx * dx + qy * dy
    c = dx * qy - dy * qx
    pb2 = (X - b[0]) ** 2 + (Y - b[1]) ** 2
    return np.where(t <= 0, pa2 * L2, np.where(t >= L2, pb2 * L2, c * c)), L2


def simplify_arc(P, q, tie="position", stats=None):
    """Ascending interior indices kept of the arc P[0] .. P[m] (points, ends included).  stats["depth"] = the deepest chord."""
    m = len(P) - 1
    X, Y = np.array([p[0] for p in P], dtype=np.int64), np.array([p[1] for p in P], dtype=np.int64)
    keys = Y * (COORD_MAX + 1) + X
    keep, stack = set(), [(0, m, 1)]
    closed = P[0] == P[m] and m >= 2
    while stack:
        i, j, level = stack.pop()
        if j <= i + 1:
            continue
        if stats is not None:
            stats["depth"] = max(stats.get("depth", 0), level)
        nums, den = distances(P[i], P[j], X[i + 1:j], Y[i + 1:j])   # ends that coincide: |p - N|^2 over 1, so the split vertex is M
        k = _farthest(nums, keys[i + 1:j], tie)
        if P[i] == P[j] or 16 * int(nums[k]) > q * den:   # a closed arc always keeps M
            keep.add(i + 1 + k)
            stack += [(i + 1 + k, j, level + 1), (i, i + 1 + k, level + 1)]
    if closed and len(keep) == 1:
        a, b = P[0], P[min(keep)]
        cr = np.abs((b[0] - a[0]) * (Y[1:m] - a[1]) - (b[1] - a[1]) * (X[1:m] - a[0]))
        t = _farthest(cr, keys[1:m], tie)
        if cr[t] != 0:
            keep.add(1 + t)
    return sorted(keep)


def simplify_ring(aug, q, tie="position", stats=None):
    """Indices kept of the rotated augmented ring: its nodes, and what Douglas-Peucker keeps of every arc between them."""
    n = len(aug)
    pts = [(a[0], a[1]) for a in aug] + [(aug[0][0], aug[0][1])]
    ends = [k for k in range(n) if aug[k][2]] or [0]
    keep = set(ends)
    ends = ends + [n]
    for i, j in zip(ends[:-1], ends[1:]):
        keep.update(i + k for k in simplify_arc(pts[i:j + 1], q, tie, stats))
        if stats is not None:
            stats["arcs"] += 1
            stats["closed"] += pts[i] == pts[j]
            stats["shared"] += aug[i][3] > 0
    return sorted(keep)


def simplify_shared(labels, counts_obj, rings, vertices, counts, q, max_objects=65536, max_vertices_out=None, tie="position",
                    insert_nodes=True):
    """dict(rings i32 [max_rings, 8], vertices i32 [max_vertices_out, 2], left i32 [max_vertices_out], counts i32 [5], info i32
    [8]) as the call defines them.  Vertex and left rows past counts[3] are zero here and left as they were there."""
    rings, vertices, counts = np.asarray(rings), np.asarray(vertices), np.asarray(counts)
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    max_out = 2 * max_vertices if max_vertices_out is None else int(max_vertices_out)
    assert 0 <= q <= TOL2_Q_MAX
    out_r = np.zeros((max_rings, 8), dtype=np.int32)
    out_v = np.zeros((max_out, 2), dtype=np.int32)
    out_l = np.zeros(max_out, dtype=np.int32)
    info = np.zeros(8, dtype=np.int32)
    found, rows_in, _, written_in, status = (int(c) for c in counts)
    if status & ST_BAD_COUNTS:
        return dict(rings=out_r, vertices=out_v, left=out_l, counts=np.array([0, 0, 0, 0, ST_BAD_COUNTS], dtype=np.int32), info=info)
    lab = Labels(labels, counts_obj, max_objects)
    rows = min(max(rows_in, 0), max_rings)
    limit = min(max(written_in, 0), max_vertices)
    V = vertices.tolist()
    room = at = written = 0
    stats = dict(arcs=0, closed=0, shared=0)
    for r, (rid, start, n, _, perimeter, x, y, _) in enumerate(rings[:rows].tolist()):
        kept = None
        if start >= 0:
            aug = None
            if n >= 4 and start + n <= limit:
                aug = augment([tuple(p) for p in V[start:start + n]], lab, insert_nodes)
            if aug is not None:                          # the augmented rings of the valid rows share a workspace of 2 max_vertices
                fits = room + len(aug) <= 2 * max_vertices
                room += len(aug)
                aug = aug if fits else None
            if aug is None:
                status |= ST_BAD_INPUT
            else:
                aug = rotate(aug)
                info[0] += sum(a[4] for a in aug)
                info[1] += sum(a[2] for a in aug)
                kept = [aug[k] for k in simplify_ring(aug, q, tie, stats)]
        if kept is None:
            out_r[r] = (rid, -1, 0, 0, perimeter, x, y, n)
            continue
        if at + len(kept) <= max_out:
            pts = [(a[0], a[1]) for a in kept]
            area2 = shoelace2(pts)
            out_r[r] = (rid, at, len(kept), area2, perimeter, pts[0][0], pts[0][1], n)
            out_v[at:at + len(kept)] = pts
            out_l[at:at + len(kept)] = [a[3] for a in kept]
            written = at + len(kept)
            info[5] += len(kept) < 3 or area2 == 0
        else:
            out_r[r] = (rid, -1, 0, 0, perimeter, x, y, n)
        at += len(kept)
    info[2:5] = stats["arcs"], stats["closed"], stats["shared"]
    if at > written:
        status |= ST_TRUNCATED
    return dict(rings=out_r, vertices=out_v, left=out_l, counts=np.array([found, rows, at, written, status], dtype=np.int32), info=info,
                depth=stats.get("depth", 0))


def geometry(out):
    """{id: [ring, ...]} and {id: [lefts, ...]} of the written rows of a result."""
    geo, lefts = {}, {}
    V, Lf = out["vertices"].tolist(), out["left"].tolist()
    for rid, start, n, *_ in out["rings"][:int(out["counts"][1])].tolist():
        if start >= 0:
            geo.setdefault(rid, []).append([tuple(p) for p in V[start:start + n]])
            lefts.setdefault(rid, []).append(Lf[start:start + n])
    return geo, lefts


def twin_failures(out):
    """The output edges p -> q of id i with left = j > 0 for which the table does not hold q -> p of id j with left = i equally
    often."""
    geo, lefts = geometry(out)
    have = {}
    for i, ring_list in geo.items():
        for ring, lf in zip(ring_list, lefts[i]):
            for k in range(len(ring)):
                e = (ring[k], ring[(k + 1) % len(ring)], i, lf[k])
                have[e] = have.get(e, 0) + 1
    return [e for e, c in have.items() if e[3] > 0 and have.get((e[1], e[0], e[3], e[2]), 0) != c]
