"""Inputs of the hull tests: hand-made ring lists with their ids, lattice point clouds, and convex lattice polygons with more
vertices than a workgroup is wide."""
import math

import numpy as np

M = 16384


def hand_made():
    """name -> (list of rings [(x, y), ...], list of ids)."""
    square = [(2, 2), (6, 2), (10, 2), (10, 6), (10, 10), (6, 10), (2, 10), (2, 6)]   # a point in the middle of every side
    plus = [(2, 0), (4, 0), (4, 2), (6, 2), (6, 4), (4, 4), (4, 6), (2, 6), (2, 4), (0, 4), (0, 2), (2, 2)]
    outer, hole = [(3, 2), (21, 2), (21, 18), (3, 18)], [(8, 6), (8, 12), (14, 12), (14, 6)]
    corners = [(1, 0), (M, 1), (M - 1, M), (0, M - 1)]       # the corners of [0, 16384]^2 moved by one: the largest products
    return {
        "single_point": ([[(5, 7)]], [1]),
        "two_points": ([[(9, 3), (2, 8)]], [1]),
        "collinear": ([[(1, 1), (3, 2), (7, 4), (5, 3), (9, 5)]], [1]),
        "duplicates": ([[(4, 4), (9, 4), (9, 9), (4, 4), (9, 9), (4, 9), (9, 4)], [(4, 9), (4, 4)]], [1, 1]),
        "side_points": ([square], [1]),
        "plus": ([plus], [1]),
        "holed": ([outer, hole], [1, 1]),
        "interleaved": ([[(0, 0), (5, 0), (5, 3)], [(10, 10), (14, 10)], [(0, 3), (2, 7)], [(14, 16), (10, 16), (12, 19)]], [1, 2, 1, 2]),
        "gap": ([[(1, 1), (4, 1), (4, 5), (1, 5)], [(7, 7), (12, 8), (9, 13)]], [1, 3]),   # id 2 owns no row
        "empty_ring": ([[], [(3, 3), (8, 4), (5, 9)], []], [2, 1, 1]),
        "full_range": ([corners], [1]),
        "axis_rectangle": ([[(3, 2), (12, 2), (12, 7), (3, 7)]], [1]),                   # four equal areas: k = 0
        "diamond": ([[(6, 0), (12, 6), (6, 12), (0, 6)]], [1]),
        "thin_diagonal": ([[(0, 0), (1, 0), (11, 10), (10, 10)]], [1]),                  # the smallest rectangle is not on edge 0
    }


def cloud(n, seed, lo=100, hi=4000):
    """n lattice points, duplicates possible, in one ring."""
    rng = np.random.default_rng(seed)
    return [tuple(int(c) for c in p) for p in rng.integers(lo, hi, (n, 2))]


def convex_polygon(n):
    """A strictly convex lattice polygon of n vertices (n divisible by 4) from the shortest primitive vectors by angle, moved
    to touch both axes; the walk's order (cross > 0), starting anywhere."""
    assert n % 4 == 0
    q, r = [], 1
    while len(q) < n // 4:                                   # primitive (a, b), a > 0, b >= 0, by length
        q = sorted(((a, b) for a in range(1, r + 1) for b in range(0, r + 1) if math.gcd(a, b) == 1 and a * a + b * b <= r * r),
                   key=lambda v: (v[0] * v[0] + v[1] * v[1], v))
        r += 1
    q = q[:n // 4]
    vecs = q + [(-b, a) for a, b in q] + [(-a, -b) for a, b in q] + [(b, -a) for a, b in q]
    vecs.sort(key=lambda v: math.atan2(v[1], v[0]) % (2 * math.pi))
    pts, x, y = [], 0, 0
    for dx, dy in vecs:
        pts.append((x, y))
        x, y = x + dx, y + dy
    assert (x, y) == (0, 0)
    x0, y0 = min(p[0] for p in pts), min(p[1] for p in pts)
    pts = [(px - x0, py - y0) for px, py in pts]
    assert max(max(p) for p in pts) <= M
    return pts


def square_sides(per_side, size=12000, at=50):
    """4 * per_side lattice points on the sides of a square, none of them strictly inside the octagon of its extremes."""
    step = size // per_side
    pts = []
    for k in range(per_side):
        pts += [(at + k * step, at), (at + size, at + k * step), (at + size - k * step, at + size), (at, at + size - k * step)]
    return pts


def chunks(points, size):
    return [points[i:i + size] for i in range(0, len(points), size)]


def rect_mask(H=96, W=96):
    m = np.zeros((H, W), np.uint8)
    for y0, x0, h, w in ((2, 3, 10, 20), (20, 5, 30, 8), (20, 30, 1, 1), (40, 40, 50, 50), (0, 60, 5, 36), (60, 0, 36, 30)):
        m[y0:y0 + h, x0:x0 + w] = 1
    return m
