"""Inputs shared by tests/test_conflicts_cpu.py, tests/test_conflicts_gpu.py and tests/test_conflicts_infer_gpu.py: one table
per pair class between two ids written down by hand, triangles of different ids inscribed in one circle, the survey masks of
tests/valid_cases.py labelled as components and as split pieces, a restatement of the header's grid rule (which shift the
device must choose, what `entries` and `work` then are), and an all-pairs count in numpy for the survey, which
tests/test_conflicts_cpu.py checks against tests/conflicts_reference.py.  A case is dict(rings, ids, frac_bits, max_ids);
`want` holds {id: (cross, same, opposite, touch_vv, touch_ve)} where the counts were taken by hand."""
import functools

import numpy as np

import objects_reference as O
import outlines_reference as T
import polis_cases as P
import simplify_reference as S
import split_reference as SP
import valid_cases as K
from polis_reference import geometry

case, tables, M = K.case, K.tables, K.M
sq = P.square


def filler(n, x0, y0, first_id):
    """n unit squares of n different ids, 3 apart: short edges that let the budget afford a fine grid."""
    return [sq(x0 + 3 * k, y0, 1) for k in range(n)], list(range(first_id, first_id + n))


def hand_made():
    out = {
        # the right wall of 1 crosses the lower edge of 2, the upper edge of 1 its left wall
        "cross": case([sq(0, 0, 10), sq(5, 5, 10)], ids=[1, 2], want={1: (2, 0, 0, 0, 0), 2: (2, 0, 0, 0, 0)}),
        # (0,0)->(10,0) and (6,0)->(20,0) run the same way over (6..10, 0); (10,0) lies inside the edge of 2, (6,0) inside that of 1
        "same": case([[(0, 0), (10, 0), (5, -5)], [(6, 0), (20, 0), (15, 5)]], ids=[1, 2], want={1: (0, 1, 0, 0, 2), 2: (0, 1, 0, 0, 2)}),
        # two squares sharing the wall x = 10, which they walk in opposite directions; at each end of the wall the two edges of
        # the one meet the two of the other: four pairs, one of them the wall itself
        "opposite": case([sq(0, 0, 10), sq(10, 0, 10)], ids=[1, 2], want={1: (0, 0, 1, 6, 0), 2: (0, 0, 1, 6, 0)}),
        "touch_vv": case([sq(0, 0, 10), sq(10, 10, 10)], ids=[1, 2], want={1: (0, 0, 0, 4, 0), 2: (0, 0, 0, 4, 0)}),
        # the apex (5, 0) of the triangle lies strictly inside the upper edge of the square
        "touch_ve": case([[(0, 0), (10, 0), (10, -10), (0, -10)], [(5, 0), (9, 6), (1, 6)]], ids=[1, 2],
                         want={1: (0, 0, 0, 0, 2), 2: (0, 0, 0, 0, 2)}),
        # the small triangle lies below the diagonal of the large one: the boxes overlap, the edges never meet
        "boxes_only": case([[(0, 0), (10, 10), (0, 10)], [(4, 1), (9, 1), (9, 6)]], ids=[1, 2], want={1: (0,) * 5, 2: (0,) * 5}),
        # one id that crosses itself: nothing is said about an id against itself
        "bow_tie_alone": case([[(0, 0), (10, 10), (10, 0), (0, 10)]], ids=[1], want={1: (0,) * 5}),
        # three triangles with their apex in (0, 0): each of the two edges that end there meets the two of each other id
        "three_in_a_point": case([[(0, 0), (10, 2), (10, -2)], [(0, 0), (-2, 10), (2, 10)], [(0, 0), (-10, -2), (-10, 2)]], ids=[1, 2, 3],
                                 want={1: (0, 0, 0, 8, 0), 2: (0, 0, 0, 8, 0), 3: (0, 0, 0, 8, 0)}),
        # the bar 3 pokes through the right wall of 1 and the left wall of 2: its partner is the smaller of the two
        "two_neighbours": case([sq(0, 0, 10), sq(20, 0, 10), [(5, 3), (25, 3), (25, 7), (5, 7)]], ids=[1, 2, 3],
                               want={1: (2, 0, 0, 0, 0), 2: (2, 0, 0, 0, 0), 3: (4, 0, 0, 0, 0)}),
        # one id of two rings whose rows interleave with the other id's
        "interleaved": case([sq(0, 0, 10), sq(5, 5, 10), sq(100, 0, 10), sq(105, 5, 10)], ids=[1, 2, 1, 2],
                            want={1: (4, 0, 0, 0, 0), 2: (4, 0, 0, 0, 0)}),
    }
    # two slivers along the two diagonals of a 4000 x 4000 box: the four long edges cross pair by pair, each pair once; 60 unit
    # squares elsewhere let the budget afford a grid of many cells, all of which the long edges' boxes cover
    rings, ids = filler(60, 5000, 5000, 3)
    out["diagonals"] = case([[(0, 0), (4000, 4000), (1, 0)], [(0, 4000), (4000, 0), (0, 3999)]] + rings, ids=[1, 2] + ids,
                            want={1: (4, 0, 0, 0, 0), 2: (4, 0, 0, 0, 0)})
    # 8 x 8 squares of side 16 that share their walls: every vertex lies on a multiple of 16, so on the border of a cell for
    # every shift up to 4, and the outer ones in the corners of the box
    out["borders"] = case([sq(16 * i, 16 * j, 16) for j in range(8) for i in range(8)], ids=list(range(1, 65)))
    for f in (0, 4, 8):                                      # the corners of the range: products reach 2^(30 + 2 f + 2)
        c = M << f
        out[f"frac_{f}"] = case([[(-c, -c), (c, c), (c, -c)], [(-c, c), (c, -c), (-c, c - 1)], [(c, c), (c - 1, c), (c, c - 1)]],
                                ids=[1, 2, 3], frac_bits=f)
    return out


@functools.lru_cache(maxsize=None)
def crowded(t, seed=3):
    """t triangles of t different ids inscribed in one circle and rotated against each other: all 3 t edges are long, so no grid
    within the budget separates them."""
    pts = P.polygon(3 * t, seed, radius=30000, wobble=0.0)
    return case([[pts[k], pts[k + t], pts[k + 2 * t]] for k in range(t)], ids=list(range(1, t + 1)))


# ------------------------------------------------------------------------------------------------------------ the grid rule
def grid(table, frac_bits, max_ids, limits):
    """dict(shift, cells_x, cells_y, entries, work, cells = {(x, y): n_c}) by the header's rule: cells of 2^s units from the lower
    corner of the box of all live edges of complete ids, an edge in every cell its box covers, the smallest s in [0, 25] within
    the two budgets, which are taken per live edge."""
    geo, incomplete, _ = geometry(*table, frac_bits, max_ids, limits[3])
    boxes = []
    for i, ring_list in geo.items():
        if i in incomplete:
            continue
        for ring in ring_list:
            for k in range(len(ring)):
                a, b = ring[k], ring[(k + 1) % len(ring)]
                if a != b:
                    boxes.append((min(a[0], b[0]), max(a[0], b[0]), min(a[1], b[1]), max(a[1], b[1])))
    if not boxes:
        return dict(shift=0, cells_x=1, cells_y=1, entries=0, work=0, cells={})
    bx = np.array(boxes, dtype=np.int64)
    x0, y0 = bx[:, 0].min(), bx[:, 2].min()
    wx, wy = bx[:, 1].max() - x0, bx[:, 3].max() - y0
    for s in range(26):
        lo_x, hi_x, lo_y, hi_y = (bx[:, 0] - x0) >> s, (bx[:, 1] - x0) >> s, (bx[:, 2] - y0) >> s, (bx[:, 3] - y0) >> s
        entries = int(((hi_x - lo_x + 1) * (hi_y - lo_y + 1)).sum())
        cells_x, cells_y = int(wx >> s) + 1, int(wy >> s) + 1
        if entries <= limits[4] * len(boxes) and cells_x * cells_y <= limits[5] * len(boxes):
            break
    cells = {}
    for ax, bx_, ay, by in zip(lo_x.tolist(), hi_x.tolist(), lo_y.tolist(), hi_y.tolist()):
        for y in range(ay, by + 1):
            for x in range(ax, bx_ + 1):
                cells[(x, y)] = cells.get((x, y), 0) + 1
    return dict(shift=s, cells_x=cells_x, cells_y=cells_y, entries=entries, work=sum(n * (n - 1) // 2 for n in cells.values()),
                cells=cells)


# --------------------------------------------------------------------------------------------------------------- the survey
SEEDS, TOLERANCES, SPLIT_R2 = K.SEEDS, (1.0, 1.5, 2.0), 1
LABELLINGS = (("components", 4), ("components", 8), ("split", 4), ("split", 8))


@functools.lru_cache(maxsize=None)
def scene(seed, labelling, connectivity):
    """{id: [ring, ...]} of the raw rings of every object of one survey mask, labelled as components or as the pieces of
    `split_reference.split` at r2 = 1.  No vertex filter."""
    mask = K.survey_mask(seed)
    if labelling == "components":
        obj = O.objects(mask, connectivity=connectivity, max_objects=K.SIZE * K.SIZE)
    else:
        obj = SP.split(mask, SPLIT_R2, connectivity=connectivity, max_objects=K.SIZE * K.SIZE)
    geo = {}
    for ring in T.trace(obj["labels"], int(obj["counts"][1]), connectivity):
        geo.setdefault(ring["id"], []).append(ring["vertices"])
    return geo


@functools.lru_cache(maxsize=None)
def simplified_scene(seed, labelling, connectivity, tol):
    return {i: K.simplified(rings, tol) for i, rings in scene(seed, labelling, connectivity).items()}


def scene_case(geo):
    """The case of a {id: rings} scene, rows in ascending id."""
    ids = [i for i in sorted(geo) for _ in geo[i]]
    return case([ring for i in sorted(geo) for ring in geo[i]], ids=ids, max_ids=max(geo) + 2)


def fast_counts(geo):
    """({id: (cross, same, opposite, touch_vv, touch_ve)}, the five sums with every pair once) of a {id: rings} scene whose ids
    are all complete: the rule over all pairs of live edges at once in numpy int64.  The survey's tool;
    tests/test_conflicts_cpu.py holds it against tests/conflicts_reference.py."""
    ids, a, b = [], [], []
    for i in sorted(geo):
        for ring in geo[i]:
            for k in range(len(ring)):
                p, q = ring[k], ring[(k + 1) % len(ring)]
                if p != q and len(ring) >= 3:
                    ids.append(i), a.append(p), b.append(q)
    ids, a, b = np.array(ids, dtype=np.int64), np.array(a, dtype=np.int64).reshape(-1, 2), np.array(b, dtype=np.int64).reshape(-1, 2)
    n = len(ids)
    e = b - a
    A, B, C, D, E, F = a[:, None, :], b[:, None, :], a[None, :, :], b[None, :, :], e[:, None, :], e[None, :, :]
    cr = lambda u, v: u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]  # noqa: E731
    o1, o2, o3, o4 = np.sign(cr(E, C - A)), np.sign(cr(E, D - A)), np.sign(cr(F, A - C)), np.sign(cr(F, B - C))
    pair = (ids[:, None] != ids[None, :]) & (np.arange(n)[:, None] < np.arange(n)[None, :])
    cross = (o1 * o2 < 0) & (o3 * o4 < 0)
    coll = (o1 == 0) & (o2 == 0) & (o3 == 0) & (o4 == 0)
    tc, td, L = ((C - A) * E).sum(-1), ((D - A) * E).sum(-1), (E * E).sum(-1)
    lo, hi = np.maximum(np.minimum(tc, td), 0), np.minimum(np.maximum(tc, td), L)
    over = coll & (lo < hi)
    dot = (E * F).sum(-1)
    same, opposite = over & (dot > 0), over & (dot < 0)
    contact = ~cross & ~coll & ~(o1 * o2 > 0) & ~(o3 * o4 > 0)
    ends = (A == C).all(-1) | (A == D).all(-1) | (B == C).all(-1) | (B == D).all(-1)
    vv, ve = (coll & (lo == hi)) | (contact & ends), contact & ~ends
    rows = {int(i): [0] * 5 for i in geo}
    sums = []
    for col, what in enumerate((cross, same, opposite, vv, ve)):
        hit = what & pair
        sums.append(int(hit.sum()))
        per = np.bincount(ids, weights=hit.sum(1) + hit.sum(0), minlength=int(ids.max()) + 1 if n else 1)
        for i in rows:
            rows[i][col] = int(per[i]) if i < len(per) else 0
    return {i: tuple(v) for i, v in rows.items()}, tuple(sums)


def in_conflict(rows):
    return sorted(i for i, v in rows.items() if v[0] + v[1] > 0)


def fall_back(raw, simple, most=16):
    """The loop "put every object in conflict back on its raw vertices, check again" on a scene: (rounds, the mixed scene).  A
    round is one check that found something; the loop can only end when every remaining conflict-free pair stands."""
    mixed = dict(simple)
    for rounds in range(most + 1):
        bad = in_conflict(fast_counts(mixed)[0])
        if not bad:
            return rounds, mixed
        for i in bad:
            mixed[i] = raw[i]
    raise AssertionError("the fall-back loop did not end")
