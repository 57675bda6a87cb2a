"""Independent restatement of `c3d_scene_outlines` (include/change3d_hip.h) in plain Python: a dict of directed boundary
edges, a walk from edge to edge with the turn priority of the connectivity, the corner / start / order rules, shoelace
areas and the prefix-shaped truncation.  Nothing here shares code with the kernels: no compaction, no pointer doubling.
`rasterise` fills rings back into pixels by the even-odd rule, for the round trip."""
import numpy as np

ST_TRUNCATED, ST_BAD_COUNTS, ST_STEP_CAP = 1, 2, 4

# side 0 top, 1 right, 2 bottom, 3 left; (dy, dx) of travel with the object on the right (y down), and of the outside
TRAVEL = ((0, 1), (1, 0), (0, -1), (-1, 0))
OUTSIDE = ((-1, 0), (0, 1), (1, 0), (0, -1))
# start vertex of side s of pixel (y, x), as an offset (dx, dy) from (x, y)
START = ((0, 0), (1, 0), (1, 1), (0, 1))


def boundary_edges(labels, rows):
    """{(y, x, side): id} over the pixels with 1 <= id <= rows."""
    lab = np.asarray(labels)
    H, W = lab.shape
    L = lab.tolist()
    edges = {}
    for y in range(H):
        for x in range(W):
            i = L[y][x]
            if i < 1 or i > rows:
                continue
            for s, (dy, dx) in enumerate(OUTSIDE):
                yy, xx = y + dy, x + dx
                if not (0 <= yy < H and 0 <= xx < W) or L[yy][xx] != i:
                    edges[(y, x, s)] = i
    return edges


def successor(edges, e, connectivity, flip=False):
    y, x, s = e
    i = edges[e]
    ty, tx = TRAVEL[s]
    oy, ox = OUTSIDE[s]
    right = (y, x, (s + 1) % 4)
    straight = (y + ty, x + tx, s)
    left = (y + ty + oy, x + tx + ox, (s + 3) % 4)
    order = (right, straight, left) if (connectivity == 4) != flip else (left, straight, right)
    for c in order:
        if edges.get(c) == i:
            return c
    raise AssertionError(f"edge {e} has no successor")


def trace(labels, rows, connectivity=8, flip=False):
    """Every ring of the ids 1 .. rows, in the order of the call: list of dict(id, key, vertices [(vx, vy)], area, perimeter)."""
    lab = np.asarray(labels)
    H, W = lab.shape
    edges = boundary_edges(lab, rows)
    seen, rings = set(), []
    for e0 in sorted(edges):
        if e0 in seen:
            continue
        ring, e = [], e0
        while e not in seen:
            seen.add(e)
            ring.append(e)
            e = successor(edges, e, connectivity, flip)
        assert e == e0, "the successor relation is a permutation: a walk ends where it began"
        corners = [k for k in range(len(ring)) if ring[k][2] != ring[k - 1][2]]
        key = lambda k: 4 * (ring[k][0] * W + ring[k][1]) + ring[k][2]  # noqa: E731
        first = min(corners, key=key)
        at = corners.index(first)
        corners = corners[at:] + corners[:at]
        verts = [(ring[k][1] + START[ring[k][2]][0], ring[k][0] + START[ring[k][2]][1]) for k in corners]
        twice = sum(verts[k - 1][0] * verts[k][1] - verts[k][0] * verts[k - 1][1] for k in range(len(verts)))
        assert twice % 2 == 0
        rings.append(dict(id=edges[e0], key=key(first), vertices=verts, area=twice // 2, perimeter=len(ring)))
    rings.sort(key=lambda r: r["key"])
    return rings


def outlines(labels, counts_obj, connectivity=8, max_objects=65536, max_rings=65536, max_vertices=1 << 20, flip=False):
    """dict(rings i32 [max_rings, 8], vertices i32 [max_vertices, 2], counts i32 [5], traced) as the call defines them;
    vertex rows past counts[3] are zero here and unspecified there."""
    found_obj, rows_obj = int(counts_obj[0]), int(counts_obj[1])
    out_r = np.zeros((max_rings, 8), dtype=np.int32)
    out_v = np.zeros((max_vertices, 2), dtype=np.int32)
    if found_obj < 0:
        return dict(rings=out_r, vertices=out_v, counts=np.array([0, 0, 0, 0, ST_BAD_COUNTS], dtype=np.int32), traced=[])
    rows = min(max(rows_obj, 0), max_objects)
    traced = trace(labels, rows, connectivity, flip)
    start = written = 0
    for r, ring in enumerate(traced):
        n = len(ring["vertices"])
        if r < max_rings:
            fits = start + n <= max_vertices
            x, y = ring["vertices"][0]
            out_r[r] = (ring["id"], start if fits else -1, n, ring["area"], ring["perimeter"], x, y, 0)
            if fits:
                out_v[start:start + n] = ring["vertices"]
                written = start + n
        start += n
    status = ST_TRUNCATED if (len(traced) > max_rings or start > written or found_obj > rows_obj) else 0
    counts = np.array([len(traced), min(len(traced), max_rings), start, written, status], dtype=np.int32)
    return dict(rings=out_r, vertices=out_v, counts=counts, traced=traced)


def rasterise(rings, H, W):
    """bool [H, W]: the pixels whose centre lies inside an odd number of the rings (lists of (vx, vy), open or closed)."""
    cross = np.zeros((H, W + 1), dtype=np.int64)         # vertical unit edges at (row y, lattice column vx)
    for ring in rings:
        v = [tuple(p) for p in ring]
        for k in range(len(v)):
            (x0, y0), (x1, y1) = v[k - 1], v[k]
            if x0 == x1 and y0 != y1:
                cross[min(y0, y1):max(y0, y1), x0] += 1
    return (np.cumsum(cross, axis=1)[:, :W] % 2) == 1
