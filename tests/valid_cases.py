"""Inputs shared by tests/test_valid_cpu.py, tests/test_valid_gpu.py and tests/test_valid_infer_gpu.py: star polygons {n/k}
on the lattice, one table per pair class written down by hand, and the survey of noisy masks traced and simplified by the
restatements (tests/outlines_reference.py, tests/simplify_reference.py).  A case is dict(rings, ids, frac_bits, max_ids);
`want` holds (cross, overlap, touch_vv, touch_ve) of id 1 where they were counted by hand."""
import functools
import math

import numpy as np

import objects_reference as O
import outlines_reference as T
import polis_cases as P
import simplify_reference as S
from fill_reference import table as make_table

M = 32768


def star(n, k, seed=0, radius=30000, centre=(0, 0)):
    """The star polygon {n/k}: the n lattice points of polis_cases.polygon (in order of angle, no wobble, so in convex
    position up to the rounding) visited k apart.  gcd(n, k) = 1 makes it one ring of n edges with n (k - 1) crossings."""
    assert math.gcd(n, k) == 1 and 2 * k < n
    pts = P.polygon(n, seed, radius=radius, centre=centre, wobble=0.0)
    return [pts[(i * k) % n] for i in range(n)]


def case(rings, ids=None, frac_bits=0, max_ids=None, want=None):
    ids = [1] * len(rings) if ids is None else list(ids)
    return dict(rings=rings, ids=ids, frac_bits=frac_bits, max_ids=max(ids) + 2 if max_ids is None else max_ids, want=want)


def tables(c, spare_rings=2, spare_vertices=3):
    """(rings i32 [max_rings, 8], vertices i32 [max_vertices, 2], counts i32 [5]) of a case."""
    return make_table(c["rings"], ids=c["ids"], max_rings=len(c["rings"]) + spare_rings,
                      max_vertices=sum(len(r) for r in c["rings"]) + spare_vertices)


def hand_made():
    sq = P.square
    corner = lambda f: M << f                                # noqa: E731  the corner of the coordinate range
    out = {
        "square": case([sq(0, 0, 10)], want=(0, 0, 0, 0)),
        "triangle": case([[(0, 0), (40, 0), (0, 30)]], want=(0, 0, 0, 0)),
        "bow_tie": case([[(0, 0), (10, 10), (10, 0), (0, 10)]], want=(1, 0, 0, 0)),
        # p -> q -> p': the edges (0,0)-(10,0) and (10,0)-(4,0) are adjacent and fold back on each other
        "spike": case([[(0, 0), (10, 0), (4, 0), (4, 8), (0, 8)]], want=(0, 1, 0, 1)),
        # two squares of one id sharing the corner (10, 10): each of the two edges that end there meets each of the other two
        "corner_shared": case([sq(0, 0, 10), sq(10, 10, 10)], want=(0, 0, 4, 0)),
        # the apex (5, 0) of the triangle lies strictly inside the lower edge of the other ring: both edges ending there touch it
        "t_contact": case([[(0, 0), (10, 0), (10, -10), (0, -10)], [(5, 0), (9, 6), (1, 6)]], want=(0, 0, 0, 2)),
        "collinear_disjoint": case([[(0, 0), (10, 0), (5, -5)], [(20, 0), (30, 0), (25, 5)]], want=(0, 0, 0, 0)),
        # (0,0)-(10,0) of one ring and (10,0)-(20,0) of the other: collinear, end to end, not adjacent; the other edges that
        # end in (10, 0) meet there too: (10,0)-(5,-5) with (10,0)-(20,0) and with (15,5)-(10,0); (0,0)-(10,0) with (15,5)-(10,0)
        "collinear_end_to_end": case([[(0, 0), (10, 0), (5, -5)], [(10, 0), (20, 0), (15, 5)]], want=(0, 0, 4, 0)),
        "collinear_overlap": case([[(0, 0), (10, 0), (5, -5)], [(6, 0), (20, 0), (15, 5)]], want=(0, 1, 0, 2)),
        # the hole pokes through the right side of its shell
        "hole_through_shell": case([sq(0, 0, 20), [(5, 5), (5, 15), (30, 15), (30, 5)]], want=(2, 0, 0, 0)),
        # (10, 0) twice: one degenerate edge, which takes part in no pair; its neighbours are no longer adjacent and touch
        "degenerate": case([[(0, 0), (10, 0), (10, 0), (10, 10), (0, 10)]], want=(0, 0, 1, 0)),
        # one id of three rings whose rows interleave with two other ids; the hole crosses the shell
        "interleaved": case([sq(0, 0, 40), sq(100, 0, 5), [(10, 10), (10, 30), (50, 30), (50, 10)], sq(200, 0, 7), sq(20, 15, 5)[::-1],
                             [(300, 0), (310, 10), (310, 0), (300, 10)]], ids=[1, 2, 1, 3, 1, 2], want=(2, 0, 0, 0)),
        # flags: id 1 checked, id 2 only a 2-gon (empty), id 3 a start < 0 row patched in by the test, id 4 all vertices equal
        # (empty, 3 degenerate), id 5 no row, id 6 checked
        "flags": case([sq(0, 0, 10), [(40, 0), (50, 0)], sq(60, 0, 10), [(7, 7), (7, 7), (7, 7)], sq(80, 0, 10)], ids=[1, 2, 3, 4, 6],
                      max_ids=8, want=(0, 0, 0, 0)),
    }
    for f in (0, 4, 8):                                      # the corners of the range: products reach 2^(30 + 2 f + 2)
        c = corner(f)
        out[f"frac_{f}"] = case([[(-c, -c), (c, c), (c, -c), (-c, c)], [(-c, -c + 1), (c - 1, c), (-c, c)]], frac_bits=f,
                                want=None)
    return out


# --------------------------------------------------------------------------------------------------------------- the survey
SEEDS, SIZE, DENSITY, MOST_VERTICES = range(40), 20, 0.62, 400


def survey_mask(seed):
    return (np.random.default_rng(seed).random((SIZE, SIZE)) < DENSITY).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def traced(seed, connectivity):
    """{id: [ring, ...]} of the raw rings of one labeling, the ids of at most MOST_VERTICES vertices."""
    mask = survey_mask(seed)
    obj = O.objects(mask, connectivity=connectivity, max_objects=SIZE * SIZE)
    geo = {}
    for ring in T.trace(obj["labels"], int(obj["counts"][1]), connectivity):
        geo.setdefault(ring["id"], []).append(ring["vertices"])
    return {i: rings for i, rings in geo.items() if sum(len(r) for r in rings) <= MOST_VERTICES}


def simplified(rings, tol):
    """The rings of one id after the restatement of c3d_outlines_simplify at `tol` pixels."""
    q = S.tol2_q(tol)
    return [[ring[k] for k in S.simplify_ring(ring, q)] for ring in rings]
