"""The restatement of `c3d_rings_hull` (tests/hull_reference.py) against independent witnesses, without a GPU: scipy's convex
hull, a minimum over all hull edges in exact fractions, the traced ring an object's hull must be a subsequence of, the bound
on the vertices of a lattice hull that the kernel's cap relies on, and the argument checks of the `ops` wrappers."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_cases as K  # noqa: E402
import hull_reference as R  # noqa: E402
import objects_reference as O  # noqa: E402
import outlines_reference as T  # noqa: E402
import simplify_cases as SK  # noqa: E402
from simplify_reference import table as make_table  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402


def _objects(mask, connectivity=8):
    """id -> (all ring vertices, the positive ring) of a traced mask."""
    labels = O.components(np.asarray(mask, np.uint8), connectivity)
    out = {}
    for ring in T.trace(labels, int(labels.max()), connectivity):
        pts, pos = out.setdefault(ring["id"], ([], []))
        pts.extend(tuple(v) for v in ring["vertices"])
        if ring["area"] > 0:
            pos.extend(tuple(v) for v in ring["vertices"])
    return out


MASKS = {"disc120": lambda: SK.disc(260, 120), "disc7": lambda: SK.disc(20, 7), "blobs": lambda: SK.blobs(96, 96, 12, 7, seed=1),
         "rectangle": lambda: np.pad(np.ones((5, 9), np.uint8), 2)}


def _scipy_hull(points):
    pts = np.array(sorted(set(points)))
    return {tuple(int(c) for c in pts[k]) for k in ConvexHull(pts).vertices}


@pytest.mark.parametrize("name", list(MASKS))
def test_walk_against_scipy_and_the_traced_ring(name):
    for rid, (pts, ring) in _objects(MASKS[name]()).items():
        h = R.hull(pts) if len(pts) <= 600 else R.hull_fast(pts)
        assert R.hull_fast(pts) == h
        assert set(h) == _scipy_hull(pts), (name, rid)       # qhull reports no collinear point as a vertex
        assert all(R.cross(h[k - 1], h[k], h[(k + 1) % len(h)]) > 0 for k in range(len(h))) and R.shoelace2(h) > 0
        assert h[0] == ring[0], "the hull begins where the object's outline does"
        at = 0
        for p in h:                                          # the hull is a subsequence of the outline: both go the same way
            at = ring.index(p, at) + 1
    if name == "disc120":
        (pts, _), = _objects(MASKS[name]()).values()
        assert len(pts) == 556 and len(R.hull_fast(pts)) == 80
    if name == "rectangle":
        (pts, _), = _objects(MASKS[name]()).values()
        h = R.hull(pts)
        assert R.rect(h) == (0, 81, 0, 81, 45, 0, 1, 2) and R.shoelace2(h) == 90


@pytest.mark.parametrize("seed", range(6))
def test_walk_against_scipy_on_lattice_clouds(seed):
    pts = K.cloud(40 + 60 * seed, seed, 0, 12 + 30 * seed)   # dense: many duplicates and collinear triples
    h = R.hull(pts)
    assert set(h) == _scipy_hull(pts) and R.hull_fast(pts) == h
    assert h[0] == min(pts, key=lambda p: (p[1], p[0]))


def test_walk_on_degenerate_sets_and_the_wrong_variants():
    assert R.hull([(5, 7)]) == [(5, 7)] == R.hull_fast([(5, 7), (5, 7)])
    assert R.hull([(9, 3), (2, 8)]) == [(9, 3), (2, 8)] == R.hull_fast([(2, 8), (9, 3)])
    line = [(1, 1), (3, 2), (7, 4), (5, 3), (9, 5)]
    assert R.hull(line) == [(1, 1), (9, 5)] == R.hull_fast(line) and R.rect(R.hull(line))[0] == -1
    side = K.hand_made()["side_points"][0][0]
    assert R.hull(side) == [(2, 2), (10, 2), (10, 10), (2, 10)] and len(R.hull(side, collinear="nearest")) == 8
    axis = R.hull(K.hand_made()["axis_rectangle"][0][0])
    assert R.rect(axis)[0] == 0 and R.rect(axis, tie="largest")[0] == 3


def _fraction_minimum(h):
    best = None
    for k in range(len(h)):
        _, L2, t0, t1, c = R.edge_rect(h, k)[:5]
        area = Fraction((t1 - t0) * c, L2)
        if best is None or area < best[0]:
            best = (area, k)
    return best


@pytest.mark.parametrize("seed", range(5))
def test_rectangle_against_a_minimum_in_fractions(seed):
    shapes = [R.hull(K.cloud(30 + 40 * seed, 20 + seed, 0, 50 + 3000 * seed)), K.convex_polygon(4 * (seed + 2))]
    shapes += [R.hull(ring[0]) for ring, _ in K.hand_made().values() if len(set(ring[0])) >= 3 and len(R.hull(ring[0])) >= 3]
    for h in shapes:
        h = R.hull(h)
        row = R.rect(h)
        area, k = _fraction_minimum(h)
        assert row[0] == k and Fraction((row[3] - row[2]) * row[4], row[1]) == area
        assert (row[3] - row[2]) * row[4] * row[1] < 2 ** 88
        P, Q = h[k], h[(k + 1) % len(h)]
        corners, long_side, short_side, angle = ops.rect_corners(P, (Q[0] - P[0], Q[1] - P[1]), row)
        want, a, b = R.rect_corners(P, (Q[0] - P[0], Q[1] - P[1]), row)
        assert np.allclose(corners, want, rtol=0, atol=1e-9) and 0.0 <= angle < 180.0
        assert math.isclose(long_side * short_side, float(area), rel_tol=1e-12) and long_side >= short_side
        assert {round(long_side, 9), round(short_side, 9)} == {round(a, 9), round(b, 9)}
        for p in h:                                          # every hull vertex lies inside the rectangle
            for i in range(4):
                (ax, ay), (bx, by) = corners[i], corners[(i + 1) % 4]
                assert (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax) >= -1e-6


def test_rect_corners_angles():
    h = [(3, 2), (12, 2), (12, 7), (3, 7)]
    corners, a, b, angle = ops.rect_corners(h[0], (9, 0), R.rect(h))
    assert corners.tolist() == [[3, 2], [12, 2], [12, 7], [3, 7]] and (a, b, angle) == (9.0, 5.0, 0.0)
    tall = [(0, 0), (2, 0), (2, 6), (0, 6)]
    assert ops.rect_corners(tall[0], (2, 0), R.rect(tall))[1:] == (6.0, 2.0, 90.0)
    square = [(6, 0), (12, 6), (6, 12), (0, 6)]
    _, a, b, angle = ops.rect_corners(square[0], (6, 6), R.rect(square))
    assert math.isclose(a, b) and math.isclose(angle, 45.0), "the first of two equal sides wins"
    with pytest.raises(ValueError):
        ops.rect_corners((0, 0), (1, 0), (-1, 0, 0, 0, 0, 0, 0, 0))
    with pytest.raises(ValueError):
        ops.rect_corners((0, 0), (1, 1), R.rect(h))


def test_no_lattice_hull_reaches_the_cap_of_the_walk():
    """Edge directions of a strictly convex lattice polygon are distinct, and inside [0, 16384]^2 the |dx| + |dy| of the edges
    add up to at most 4 * 16384.  Count the primitive vectors by |dx| + |dy| until the budget is spent."""
    budget, count, s = 4 * K.M, 0, 1
    while True:
        n = 4 * sum(1 for a in range(1, s + 1) if math.gcd(a, s - a) == 1) if s > 1 else 4   # (a, s - a) in four quadrants
        if n * s > budget:
            count += budget // s
            break
        budget -= n * s
        count += n
        s += 1
    assert count < 4096, count
    assert len(K.convex_polygon(2048)) == 2048 and len(R.hull_fast(K.convex_polygon(1040))) == 1040


def test_tables_of_the_restatement():
    ring_lists, ids = K.hand_made()["gap"]
    rings, vertices, counts = make_table(ring_lists, max_rings=4, max_vertices=9, ids=ids)
    out = R.hulls(rings, vertices, counts, 5, 9)
    assert out["counts"].tolist() == [2, 3, 7, 7, 0] and out["hulls"][1].tolist() == [2, -1, 0, 0, 0, 0, 0, 0]
    assert out["hulls"][:, 1].tolist() == [0, -1, 4, 0, 0] and out["rects"][:, 0].tolist() == [0, -1, out["rects"][2, 0], 0, 0]
    cut = R.hulls(rings, vertices, counts, 5, 6)
    assert cut["counts"].tolist() == [2, 3, 7, 4, R.ST_HULL_TRUNCATED] and cut["hulls"][2, 1] == -1 and np.array_equal(cut["rects"], out["rects"])
    rings[0, 0] = 9
    assert R.hulls(rings, vertices, counts, 5, 9)["counts"].tolist() == [1, 3, 3, 3, R.ST_BAD_ROW]


def test_ops_argument_checks_refuse_without_a_gpu():
    rings, vertices, counts = (torch.zeros((4, 8), dtype=torch.int32), torch.zeros((9, 2), dtype=torch.int32), torch.zeros(5, dtype=torch.int32))
    with pytest.raises(Exception):
        ops.rings_hull(rings, vertices, counts)              # host tensors
    assert L.HULL_ST_BAD_ROW == R.ST_BAD_ROW == 64 and L.HULL_ST_TRUNCATED == R.ST_HULL_TRUNCATED == 128
    assert hasattr(ops, "rings_hull_limits")
