"""Independent restatement of `c3d_rings_valid` (include/change3d_hip.h) in plain Python: integers, every unordered pair of an
id's live edges by `itertools.combinations`, no numpy in the predicate, no bounding boxes, no tiers, no chunks.  The rows used
and the incomplete ids are those of `c3d_rings_polis` for one side, taken from tests/polis_reference.py.  The three keyword
switches turn the rule into the wrong ones of the negative controls."""
import itertools

import numpy as np

from polis_reference import geometry

CROSS, OVERLAP, VV, VE = "cross", "overlap", "touch_vv", "touch_ve"
COLUMNS = {CROSS: 4, OVERLAP: 5, VV: 6, VE: 7}


def _sign(v):
    return (v > 0) - (v < 0)


def _cross(o, p, q):
    return (p[0] - o[0]) * (q[1] - o[1]) - (p[1] - o[1]) * (q[0] - o[0])


def _on(p, a, b):
    """p lies on the closed segment (a, b)."""
    return _cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def classify(a, b, c, d, adjacent=False, strict=True, adjacent_overlap=True):
    """The class of the live edges (a, b) and (c, d): CROSS, OVERLAP, VV, VE or None."""
    o1, o2, o3, o4 = _sign(_cross(a, b, c)), _sign(_cross(a, b, d)), _sign(_cross(c, d, a)), _sign(_cross(c, d, b))
    if strict:
        if o1 * o2 < 0 and o3 * o4 < 0:
            return CROSS
    elif o1 * o2 <= 0 and o3 * o4 <= 0:                    # the wrong rule: touches and collinear pairs become crossings
        return CROSS
    if o1 == 0 and o2 == 0 and o3 == 0 and o4 == 0:
        if adjacent and not adjacent_overlap:              # the wrong rule: a folded spike goes unseen
            return None
        ex, ey = b[0] - a[0], b[1] - a[1]
        tc, td, L = (c[0] - a[0]) * ex + (c[1] - a[1]) * ey, (d[0] - a[0]) * ex + (d[1] - a[1]) * ey, ex * ex + ey * ey
        lo, hi = max(min(tc, td), 0), min(max(tc, td), L)
        if lo < hi:
            return OVERLAP
        return VV if lo == hi and not adjacent else None
    shared = {p for p in (c, d) if _on(p, a, b)} | {p for p in (a, b) if _on(p, c, d)}
    if not shared or adjacent:
        return None
    assert len(shared) == 1
    p = next(iter(shared))
    return VV if p in (a, b) and p in (c, d) else VE


def edges_of(ring_list):
    """[(a, b, ring index, index within the ring, n)] of an id's rings, the closing edges included."""
    out = []
    for r, ring in enumerate(ring_list):
        n = len(ring)
        out += [(ring[k], ring[(k + 1) % n], r, k, n) for k in range(n)]
    return out


def count_pairs(ring_list, strict=True, adjacent_overlap=True, ring_adjacency=True):
    """(m, degenerate, {class: pairs}) of one id."""
    edges = edges_of(ring_list)
    live = [(pos, e) for pos, e in enumerate(edges) if e[0] != e[1]]
    total = len(edges)
    got = {CROSS: 0, OVERLAP: 0, VV: 0, VE: 0}
    for (pi, (a, b, ri, ki, ni)), (pj, (c, d, rj, kj, _)) in itertools.combinations(live, 2):
        if ring_adjacency:
            adjacent = ri == rj and (ki - kj) % ni in (1, ni - 1)
        else:                                              # the wrong rule: neighbours in the id's list, across rings too
            adjacent = (pi - pj) % total in (1, total - 1)
        what = classify(a, b, c, d, adjacent, strict, adjacent_overlap)
        if what:
            got[what] += 1
    return len(live), total - len(live), got


def valid(table, frac_bits, max_ids, max_id_work=2 ** 32, ring_limit=16384, **wrong):
    """dict(valid i64 [max_ids, 8], counts i64 [8]) as the call defines them."""
    geo, incomplete, top = geometry(*table, frac_bits, max_ids, ring_limit)
    rows = np.zeros((max_ids, 8), dtype=np.int64)
    counts = np.zeros(8, dtype=np.int64)
    for i in range(1, top + 1):
        if i in incomplete:
            rows[i - 1, 0] = 2
            counts[3] += 1
            continue
        rings = geo.get(i, [])
        edges = edges_of(rings)
        m = sum(1 for e in edges if e[0] != e[1])
        rows[i - 1, 1:4] = (len(rings), m, len(edges) - m)
        if m == 0:
            rows[i - 1, 0] = 1
            counts[2] += 1
        elif m * (m - 1) // 2 > max_id_work:
            rows[i - 1, 0] = 3
            counts[4] += 1
        else:
            _, _, got = count_pairs(rings, **wrong)
            for what, col in COLUMNS.items():
                rows[i - 1, col] = got[what]
            counts[0] += 1
            counts[1] += bool(got[CROSS] or got[OVERLAP])
            counts[5] += got[CROSS]
            counts[6] += got[OVERLAP]
    counts[7] = int(table[2][4])
    return dict(valid=rows, counts=counts)
