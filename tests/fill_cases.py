"""Inputs shared by tests/test_fill_cpu.py and tests/test_fill_gpu.py: masks for the round trips and ring tables built by
hand.  Coordinates of the hand-built cases are given in pixels as exact multiples of 1/2 and scaled to units of 2^-f."""
import math

import numpy as np


def masks(H, W, seed=0):
    """name -> u8 [H, W]."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {}
    blobs = np.zeros((H, W), dtype=bool)
    for _ in range(max(3, H * W // 600)):
        cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(2, 9), rng.integers(2, 13)
        blobs |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    out["blobs"] = blobs
    ring = np.zeros((H, W), dtype=bool)
    ring[1:H - 1, 1:W - 1] = True                         # one object across the whole scene with a lattice of holes
    ring[3:H - 3:4, 3:W - 3:5] = False
    ring[H // 2 - 4:H // 2 + 4, W // 3:W // 3 + 9] = False
    out["ring_with_holes"] = ring
    out["checkerboard"] = (yy + xx) % 2 == 0
    snake = np.zeros((H, W), dtype=bool)
    snake[::2] = True
    snake[1::4, W - 1] = True
    snake[3::4, 0] = True
    out["serpentine"] = snake
    diag = np.zeros((H, W), dtype=bool)
    d = np.arange(min(H, W))
    diag[d, d] = True
    diag[d[:-2], d[:-2] + 2] = True
    out["diagonal"] = diag
    out["full"] = np.ones((H, W), dtype=bool)
    out["empty"] = np.zeros((H, W), dtype=bool)
    return {k: v.astype(np.uint8) for k, v in out.items()}


def wide_mask(H, W):
    """One object as wide as the scene with holes, and small ones inside the holes: the widest band of the workgroup tier."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[2:H - 2, :] = 1
    m[6:H - 6:9, 5:W - 5:37] = 0
    m[10:H - 10, 100:W - 100:997] = 0
    m[20:30, 40:W - 40] = 0
    m[23:27, 60:W - 60:3] = 1
    return m


def touching_mask(H, W):
    """Two discs joined by a neck, and two squares joined by a thin bridge: `scene_split` cuts both."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy - H // 3) ** 2 + (xx - W // 4) ** 2 <= (H // 5) ** 2) | ((yy - H // 3) ** 2 + (xx - W // 4 - H // 3) ** 2 <= (H // 5) ** 2)
    m[H - 14:H - 2, 2:14] = True
    m[H - 14:H - 2, 18:30] = True
    m[H - 9:H - 7, 14:18] = True
    return m.astype(np.uint8)


def _scale(rings, f):
    """Pixel coordinates given as multiples of 1/2 to integers in units of 2^-f.  At f = 0 the halves are rounded down."""
    s = 1 << f
    return [[(math.floor(x * s), math.floor(y * s)) for x, y in ring] for ring in rings]


def rect(x0, y0, x1, y1, ccw=False):
    r = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return r[::-1] if ccw else r


def star(cx, cy, r, points=5, step=2):
    """A star polygon that crosses itself: every `step`-th of `points` points on a circle, on the half-pixel lattice."""
    out = []
    for k in range(points):
        a = 2 * math.pi * ((k * step) % points) / points - math.pi / 2
        out.append((round(2 * (cx + r * math.cos(a))) / 2, round(2 * (cy + r * math.sin(a))) / 2))
    return out


HS, WS = 96, 80                                           # the scene of the hand-built cases: taller than one band


def hand_built(f):
    """name -> (ring lists in units of 2^-f, ids, max_objects)."""
    big = 32768
    cases = {
        "stars_and_triangles": ([star(30, 30, 24), star(60, 70, 17.5, 7, 3), [(2, 2), (20, 5), (7, 30)], [(40, 2), (70, 20), (40, 20), (70, 2)],
                                 [(5.5, 60.5), (25.5, 60.5), (15.5, 90)]], [1, 2, 3, 4, 5], 6),
        "cw_and_ccw": ([rect(3, 3, 30, 40), rect(35, 3, 62, 40, ccw=True), rect(3.5, 50.5, 70, 90), rect(10, 55, 60.5, 85.5, ccw=True)],
                       [1, 2, 3, 3], 4),
        "hole_and_twice": ([rect(4, 4, 70, 90), rect(10, 10, 30, 30), rect(12, 12, 20, 20), rect(40, 40, 60, 60.5), rect(40, 40, 60, 60.5),
                            rect(42, 70, 50, 80), rect(42, 70, 50, 80, ccw=True), rect(42, 70, 50, 80)], [1, 1, 1, 2, 2, 3, 3, 3], 5),
        "scattered": ([rect(1, 1, 9, 9), rect(20, 1, 29, 9), rect(3, 3, 6, 6), rect(40, 1, 49, 9), rect(1, 20, 70, 95), [(22, 3), (27, 3), (25, 7)],
                       rect(5, 25, 60, 90)], [1, 2, 1, 3, 1, 2, 1], 3),
        "degenerate": ([[], [(5, 5)], [(5, 5), (30, 30)], [(3, 3), (3, 3), (3, 3)], [(10, 10), (40, 10), (70, 10)],
                        [(10, 20), (10, 20), (40, 20), (40, 20), (40, 50), (40, 50), (10, 50)], [(50, 60), (70, 60), (70, 60), (60, 60), (60, 80)],
                        [(5, 60), (5, 90), (5, 75), (30, 75)]], [1, 2, 3, 4, 5, 6, 7, 8], 9),
        # centres lie at k + 1/2: vertices on them, edges through them (a diagonal of the lattice passes through every centre
        # it meets), a vertical edge along a column of centres, a horizontal one along a row of them
        "strictness": ([[(0, 0), (20, 20), (0, 20)], [(30, 0), (50, 0), (30, 20)], [(10.5, 30.5), (40.5, 30.5), (40.5, 50.5), (10.5, 50.5)],
                        [(50.5, 30.5), (70.5, 50.5), (50.5, 70.5), (30.5, 50.5)], [(0, 60), (20, 80), (0, 95)], [(60, 70), (79, 89), (60, 89)]],
                       [1, 2, 3, 4, 5, 6], 6),
        "outside": ([rect(-20, -20, 10, 10), rect(70, 85, 120, 130), rect(-30, 40, -5, 60), rect(100, 10, 130, 30), rect(20, -50, 40, -10),
                     rect(20, 100, 40, 140), [(-big, -big), (big, -big), (big, big)], [(-big, 50), (big, 40.5), (big, 60), (-big, 70.5)],
                     [(40, -big), (50, -big), (60.5, big), (45, big)], rect(-big, -big, big, big), rect(-big, 20, -big + 5, 30)],
                    [2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 11], 12),     # the square that covers everything paints first
        "overlap": ([rect(5, 5, 60, 60), rect(15, 15, 40, 40), rect(20, 20, 30, 30), rect(50, 50, 75, 90), rect(50, 50, 75, 90),
                     [(10, 70), (45, 65), (40, 92), (5, 88)], [(30, 60), (48, 75), (20, 95)]], [1, 2, 3, 4, 5, 7, 6], 7),
    }
    return {name: (_scale(rings, f), ids, max_objects) for name, (rings, ids, max_objects) in cases.items()}
