"""Inputs shared by tests/test_simplify_cpu.py and tests/test_simplify_gpu.py: small masks to trace on the CPU, rings written
down by hand, and synthetic lattice rings of a given vertex count or recursion depth.  Rings are lists of (x, y)."""
import math

import numpy as np

TOLERANCES = (0.0, 0.5, 1.0, 2.0, 1024.0)


def blobs(H, W, n, r, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), bool)
    yy, xx = np.mgrid[:H, :W]
    for _ in range(n):
        cy, cx, a, b = rng.integers(0, H), rng.integers(0, W), rng.integers(3, r), rng.integers(3, r)
        th = rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        w = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        m |= (np.abs(u) < a) & (np.abs(w) < b)
    return m.astype(np.uint8)


def serpentine(H, W):
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def disc(size, radius):
    yy, xx = np.mgrid[:size, :size]
    return (((xx - size // 2) ** 2 + (yy - size // 2) ** 2) < radius * radius).astype(np.uint8)


def masks():
    """name -> mask, none above 96 x 96."""
    holed = np.zeros((20, 24), np.uint8)
    holed[2:18, 3:21] = 1
    holed[5:9, 6:12] = 0
    holed[11:15, 9:18] = 0
    holed[10, 4] = 0
    return {"blobs": blobs(96, 96, 12, 16), "random": (np.random.default_rng(3).random((48, 64)) < 0.59).astype(np.uint8),
            "serpentine": serpentine(33, 32), "disc": disc(96, 40), "holed": holed,
            "diagonal_pair": np.array([[1, 0], [0, 1]], np.uint8)}


def hand_made():
    """name -> list of rings."""
    plus = [(2, 0), (4, 0), (4, 2), (6, 2), (6, 4), (4, 4), (4, 6), (2, 6), (2, 4), (0, 4), (0, 2), (2, 2)]
    stairs = [(0, 0)]
    for k in range(9):
        stairs += [(k + 1, k), (k + 1, k + 1)]
    stairs += [(0, 9)]
    return {
        "pixel": [[(3, 2), (4, 2), (4, 3), (3, 3)]],
        "rectangle": [[(1, 1), (9, 1), (9, 5), (1, 5)]],
        "L": [[(0, 0), (3, 0), (3, 7), (8, 7), (8, 10), (0, 10)]],
        "plus": [plus],
        "staircase": [stairs],
        "holed": [[(0, 0), (12, 0), (12, 9), (0, 9)], [(5, 3), (3, 3), (3, 4), (2, 4), (2, 6), (5, 6)]],
        "repeated_vertex": [[(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]],
        # (1, 3) lies exactly 1 px off the chord (0, 0) -> (6000, 8000): cross^2 = L2 = 1e8; (0, 3) lies 1.8 px off it
        "strictness": [[(0, 0), (1, 3), (6000, 8000), (6000, 0)], [(0, 0), (0, 3), (6000, 8000), (6000, 0)]],
        # the diagonal of the whole coordinate range as a chord: 8 (py - px)^2 against tol2_q, on the threshold at tol = 1024
        # between |py - px| = 1448 and 1449; 16 * num reaches 2^60 at the corner (16384, 0)
        "full_range": [[(0, 0), (7468, 8916), (16384, 16384), (16384, 0)], [(0, 0), (7468, 8917), (16384, 16384), (16384, 0)],
                       [(0, 16384), (16384, 16384), (16384, 0), (3, 4), (0, 0)]],
        "hook": [[(10, 10), (4, 11), (30, 10), (30, 30)]],
        # five turns round the whole coordinate range: the shoelace sum, 5 * 2^29, leaves i32 and is stored modulo 2^32
        "winding": [[(0, 0), (16384, 0), (16384, 16384), (0, 16384)] * 5],
        "degenerate": [[(5, 5), (5, 5), (5, 5), (5, 5), (5, 5)], [(0, 0), (4, 0), (8, 0), (4, 0), (2, 0)], [(1, 1), (2, 2), (3, 3)],
                       [(7, 7)], []],
    }


def lattice_ring(n, seed, radius=6000, noise=400, centre=8192):
    """n lattice points round a noisy circle: neither rectilinear nor necessarily simple, inside [0, 16384]."""
    rng = np.random.default_rng(seed)
    r = radius + rng.integers(-noise, noise + 1, n)
    a = 2 * math.pi * np.arange(n) / max(n, 1)
    x = np.rint(centre + r * np.cos(a)).astype(np.int64)
    y = np.rint(centre + r * np.sin(a)).astype(np.int64)
    return list(zip(x.tolist(), y.tolist()))


def zigzag_ring(teeth, filler=0, height=50):
    """A comb of `teeth` equal teeth under a tall box: every tooth ties with the rest, the first one wins, and the recursion
    goes one level deeper per tooth.  `filler` collinear vertices along the top edge add vertices without depth."""
    v = [(0, 0)] + [(2 * k, height if k % 2 else 0) for k in range(1, teeth + 1)]
    right = 2 * teeth + 2 + filler
    assert right <= 16384
    v += [(right, 0), (right, 16000)]
    v += [(right - k, 16000) for k in range(1, filler + 1)]
    return v + [(0, 16000)]
