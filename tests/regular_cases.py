"""Inputs shared by tests/test_regular_cpu.py and tests/test_regular_gpu.py: ring lists written down by hand with the
direction of every id, hull tables that carry such directions, staircase rings of a given edge count, tables of many small
rings, and rasterised rotated rectangles.  Rings are lists of (x, y)."""
import numpy as np

M = 16384
NO_HULL_START, SHORT_HULL, PAST_K = "start", "short", "past_k"   # the three ways an id has no direction


def hull_tables(dirs, max_objects, spare_vertices=3):
    """(hulls i32 [max_objects, 8], hull_vertices i32 [.., 2], rects i64 [max_objects, 8], counts_hull i32 [5]) in which id
    (1-based) has the direction dirs[id]: a vector d = (dx, dy), not necessarily primitive, stored as a hull edge k = 1 of a
    triangle.  dirs[id] may also be one of the three markers above; an id that is missing gets an empty hull row."""
    hulls = np.zeros((max_objects, 8), dtype=np.int32)
    rects = np.zeros((max_objects, 8), dtype=np.int64)
    verts = []
    K = max((i for i, d in dirs.items() if d != PAST_K), default=0)
    for rid in range(1, K + 1):
        d = dirs.get(rid)
        if d is None or d == PAST_K:
            hulls[rid - 1] = (rid, -1, 0, 0, 0, 0, 0, 0)
            rects[rid - 1, 0] = -1
            continue
        if d == SHORT_HULL:
            hulls[rid - 1] = (rid, len(verts), 2, 0, 0, 3, 3, 2)
            verts += [(3, 3), (9, 5)]
            rects[rid - 1, 0] = -1
            continue
        dx, dy = (3, 1) if d == NO_HULL_START else d
        a = (max(0, -dx), max(0, -dy))
        tri = [(M - a[0], M - a[1]), a, (a[0] + dx, a[1] + dy)]   # the edge k = 1 runs from a along d
        hulls[rid - 1] = (rid, -1 if d == NO_HULL_START else len(verts), 3, 1, 0, a[0], a[1], 3)
        if d != NO_HULL_START:
            verts += tri
        rects[rid - 1] = (1, dx * dx + dy * dy, 0, 1, 1, 0, 1, 2)
    for rid, d in dirs.items():                              # rows past K that look usable but are not to be looked at
        if d == PAST_K:
            hulls[rid - 1] = (rid, 0, 3, 1, 0, 0, 0, 3)
            rects[rid - 1] = (1, 10, 0, 1, 1, 0, 1, 2)
    hv = np.zeros((max(1, len(verts)) + spare_vertices, 2), dtype=np.int32)
    if verts:
        hv[:len(verts)] = verts
    ids = sum(1 for d in dirs.values() if d not in (None, PAST_K))
    return hulls, hv, rects, np.array([ids, K, len(verts), len(verts), 0], dtype=np.int32)


WOBBLY = [(20, 10), (35, 16), (50, 20), (46, 33), (42, 44), (27, 38), (12, 34), (16, 21)]   # a rectangle along (3, 1), bent


def hand_made():
    """name -> (list of rings, list of ids, {id: direction})."""
    rect = [(1, 1), (9, 1), (9, 5), (1, 5)]
    hole = [(3, 2), (3, 4), (7, 4), (7, 2)]
    return {
        "n3": ([[(1, 1), (9, 1), (9, 5)]], [1], {1: (1, 0)}),
        "n4_junction_at_0": ([rect], [1], {1: (1, 0)}),
        "R0": ([[(0, 5), (10, 6), (20, 5), (10, 4)]], [1], {1: (1, 0)}),
        "R2": ([[(0, 0), (10, 1), (20, 0), (18, 10)]], [1], {1: (1, 0)}),
        "zero_edge": ([[(1, 1), (9, 1), (9, 1), (9, 5), (1, 5)]], [1], {1: (1, 0)}),
        "run_wraps_0": ([[(5, 2), (9, 1), (9, 5), (1, 5), (1, 1)]], [1], {1: (1, 0)}),
        "tie45": ([[(0, 0), (10, 0), (14, 4), (14, 12), (0, 12)]], [1], {1: (1, 0)}),
        "gcd": ([WOBBLY], [1], {1: (6, 2)}),
        "negative_u": ([WOBBLY, [(x + 100, y + 7) for x, y in WOBBLY]], [1, 2], {1: (-3, -1), 2: (1, -3)}),
        "holes": ([[(0, 0), (12, 1), (12, 9), (0, 9)], hole, [(x + 20, y) for x, y in WOBBLY]], [1, 1, 2], {1: (1, 0), 2: (3, 1)}),
        "not_contiguous": ([WOBBLY, rect, [(x + 60, y + 60) for x, y in WOBBLY], [(x + 30, y) for x, y in rect]], [1, 2, 1, 2],
                           {1: (3, 1), 2: (0, 5)}),
        "no_direction": ([WOBBLY, WOBBLY, WOBBLY, WOBBLY, rect], [1, 2, 3, 4, 5],
                         {1: SHORT_HULL, 2: NO_HULL_START, 3: (3, 1), 4: None, 5: PAST_K}),
        "empty_ring": ([[], rect, []], [2, 1, 1], {1: (1, 0), 2: (1, 1)}),
    }


FULL_RANGE = ([[(1, 0), (M, 1), (M - 1, M), (0, M - 1)], [(0, 0), (M, 0), (M, M), (M // 2, M - 1), (0, M)]], [1, 1],
              {1: (M, -(M - 1))})


def stair_ring(n, seed):
    """A staircase of n vertices (n >= 6) from (100, 100) down to the right and back round the corner, every vertex moved by
    0 or 1 px: about n junctions along (1, 0), runs of several edges along other directions."""
    rng = np.random.default_rng(seed)
    steps = (n - 2) // 2
    x, y, pts = 100, 100, [(100, 100)]
    for a, b in rng.integers(3, 5, (steps, 2)).tolist():
        x += a
        pts.append((x, y))
        y += b
        pts.append((x, y))
    pts.append((100, y))
    if len(pts) < n:
        pts.append((101, (y + 100) // 2))
    assert len(pts) == n and x < M and y < M
    jitter = rng.integers(0, 2, (n, 2)).tolist()
    return [(px + jx, py + jy) for (px, py), (jx, jy) in zip(pts, jitter)]


DIRECTIONS = [(1, 0), (3, 1), (2, 5), (1, 1), (-3, -1), (1, -3), (0, 7), (-5, 2), (12, 4), (M, -(M - 1))]


def many_small(count, seed, objects=40):
    """`count` rings of 4 to 8 vertices, bent rectangles on a grid, their ids cycling over `objects` ids with the directions
    of DIRECTIONS; every fifth id has none."""
    rng = np.random.default_rng(seed)
    lists, ids = [], []
    for i in range(count):
        x0, y0 = 10 + 40 * (i % 300), 10 + 40 * (i // 300)
        w, h = (int(c) for c in rng.integers(6, 30, 2))
        ring = [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)]
        for side in rng.permutation(4)[:int(rng.integers(0, 5))].tolist():   # a bent side: one more vertex
            a, b = ring[side], ring[(side + 1) % len(ring)]
            ring.insert(side + 1, ((a[0] + b[0]) // 2 + int(rng.integers(0, 2)), (a[1] + b[1]) // 2 + int(rng.integers(0, 2))))
        k = int(rng.integers(0, len(ring)))
        lists.append(ring[k:] + ring[:k])
        ids.append(1 + i % objects)
    dirs = {rid: DIRECTIONS[rid % len(DIRECTIONS)] for rid in range(1, objects + 1) if rid % 5}
    return lists, ids, dirs


def rotated_rectangle(d, long_px=40, short_px=25, size=96):
    """u8 [size, size]: the pixels whose centres lie in a long_px x short_px rectangle along the integer direction d."""
    yy, xx = np.mgrid[:size, :size]
    n = float(np.hypot(*d))
    ux, uy = d[0] / n, d[1] / n
    px, py = xx + 0.5 - size / 2, yy + 0.5 - size / 2
    return ((np.abs(px * ux + py * uy) <= long_px / 2) & (np.abs(py * ux - px * uy) <= short_px / 2)).astype(np.uint8)
