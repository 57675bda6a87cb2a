"""Inputs shared by tests/test_polis_cpu.py, tests/test_polis_gpu.py and tests/test_polis_scene_gpu.py: polygons of a given
vertex count, tables written down by hand, and the scene of rotated rectangles.  Rings are lists of (x, y); a case is
dict(P=(rings, ids, frac_bits), G=(rings, ids, frac_bits), match={p: g}, max_p, max_g)."""
import math

import numpy as np

from fill_reference import table as make_table

M = 32768


def polygon(n, seed=0, radius=6000, centre=(0, 0), wobble=0.1):
    """n distinct lattice points round `centre`, in order of angle: a star-shaped ring."""
    rng = np.random.default_rng(seed)
    r = radius * (1.0 + wobble * (rng.random(n) - 0.5))
    a = 2.0 * math.pi * (np.arange(n) + 0.3 * rng.random(n)) / n
    pts = [(int(round(centre[0] + r[k] * math.cos(a[k]))), int(round(centre[1] + r[k] * math.sin(a[k])))) for k in range(n)]
    assert len(set(pts)) == n
    return pts


def square(x0, y0, side):
    return [(x0, y0), (x0 + side, y0), (x0 + side, y0 + side), (x0, y0 + side)]


def case(P, G, match, f_p=0, f_g=0, ids_p=None, ids_g=None, max_p=None, max_g=None):
    ids_p = list(range(1, len(P) + 1)) if ids_p is None else ids_p
    ids_g = list(range(1, len(G) + 1)) if ids_g is None else ids_g
    return dict(P=(P, ids_p, f_p), G=(G, ids_g, f_g), match=match, max_p=max(ids_p) + 2 if max_p is None else max_p,
                max_g=max(ids_g) + 1 if max_g is None else max_g)


def tables(c, spare_rings=2, spare_vertices=3):
    """((rings, vertices, counts) of P, the same of G, match_p i32 [max_p, 4]) of a case."""
    out = []
    for rings, ids, _ in (c["P"], c["G"]):
        out.append(make_table(rings, ids=ids, max_rings=len(rings) + spare_rings, max_vertices=sum(len(r) for r in rings) + spare_vertices))
    match = np.zeros((c["max_p"], 4), dtype=np.int32)
    for p, g in c["match"].items():
        match[p - 1] = (g, 1, 1, 1)
    return out[0], out[1], match


def sized(n_p, n_g, seed=0):
    """One pair of polygons with n_p and n_g vertices, 150 units apart."""
    return case([polygon(n_p, seed)], [polygon(n_g, seed + 100, centre=(150, -90))], {1: 1})


def hand_made():
    outer, hole_a, hole_b = square(0, 0, 100), square(10, 10, 20)[::-1], square(60, 60, 20)[::-1]
    other = [(200, 0), (260, 5), (230, 70)]
    return {
        "triangles": case([[(0, 0), (40, 0), (0, 30)]], [[(3, 2), (45, 1), (1, 33)]], {1: 1}),
        "n64": sized(64, 64, seed=1),
        "squares_apart": case([square(20, 0, 10)], [square(0, 0, 10)], {1: 1}),
        # id 1 of P is a small ring inside hole_a of G's id 2: the nearest boundary is the hole ring.  G's id 2 has three rings,
        # interleaved with the rows of ids 1 and 3
        "holes_interleaved": case([square(12, 14, 10), other], [other, outer, [(300, 300), (310, 300), (305, 320)], hole_a, other[::-1],
                                                                hole_b], {1: 2, 2: 1}, ids_g=[1, 2, 3, 2, 3, 2]),
        "frac_0_against_4": case([[(-M, -M), (M, -M), (M, M), (-M, M)]], [[(-16 * M, -16 * M + 5), (16 * M, -16 * M), (16 * M - 7, 16 * M),
                                                                          (-16 * M, 16 * M - 3)]], {1: 1}, f_p=0, f_g=4),
        "frac_8_against_0": case([[(-256 * M, -256 * M), (256 * M, 256 * M - 1), (-256 * M + 1, 256 * M)]],
                                 [[(-M, M), (M, -M), (M, M)]], {1: 1}, f_p=8, f_g=0),
        "zero_and_collinear": case([[(0, 0), (10, 0), (10, 0), (20, 0), (20, 10), (20, 10), (0, 10)]],
                                   [[(1, 1), (1, 1), (1, 1)], [(0, -2), (5, -2), (10, -2), (22, -2), (22, 12), (11, 12), (0, 12)]], {1: 1},
                                   ids_g=[1, 1]),
        # partner 0, a start < 0 row (patched in by the test), only short rings, an id without rows
        "flags": case([square(0, 0, 10), square(20, 0, 10), [(40, 0), (50, 0)], square(60, 0, 10), square(80, 0, 10)],
                      [square(1, 1, 10), square(21, 1, 10), square(41, 1, 10), square(61, 1, 10)], {1: 1, 2: 0, 3: 3, 4: 4, 5: 2},
                      ids_p=[1, 2, 3, 4, 6], max_p=8, max_g=4),
    }


DIRECTIONS = [(3, 1), (2, 5), (5, -2), (1, 1)]


def true_rectangle(d, long_px=40, short_px=25, size=96, f=4, centre=None):
    """The corners of the rectangle that regular_cases.rotated_rectangle rasterises, at 2^-f px (rounded to that grid)."""
    n = math.hypot(*d)
    ux, uy = d[0] / n, d[1] / n
    cx, cy = (size / 2, size / 2) if centre is None else centre
    out = []
    for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        x = cx + a * long_px / 2 * ux - b * short_px / 2 * uy
        y = cy + a * long_px / 2 * uy + b * short_px / 2 * ux
        out.append((int(round(x * (1 << f))), int(round(y * (1 << f)))))
    return out
