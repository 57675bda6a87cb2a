"""Independent restatement of `c3d_rings_conflicts` (include/change3d_hip.h) in plain Python: integers, every unordered pair of
live edges of all complete ids by `itertools.combinations`, the class of a pair by `valid_reference.classify(...,
adjacent=False)` and the sign of the dot product for overlaps.  No grid, no cells, no bounding boxes, no tiers.  The rows used
and the incomplete ids are those of `c3d_rings_polis` for one side (tests/polis_reference.py).  The three keyword switches turn
the rule into the wrong ones of the negative controls.  The columns of `info` that describe the grid (1 .. 5) are the
implementation's and are not restated; `info` here carries elements 0, 6 and 7 and zeros elsewhere."""
import itertools

import numpy as np

import valid_reference as V
from polis_reference import geometry

CROSS, SAME, OPPOSITE, VV, VE = "cross", "same", "opposite", "touch_vv", "touch_ve"
COLUMNS = {CROSS: 3, SAME: 4, OPPOSITE: 5, VV: 6, VE: 7}
FIXED_INFO = (0, 6, 7)                                       # the elements of info that the rule fixes


def pair_class(a, b, c, d, direction=True, strict=True):
    """The class of two live edges of different ids, or None."""
    what = V.classify(a, b, c, d, adjacent=False, strict=strict)
    if what == V.OVERLAP:
        if not direction:                                    # the wrong rule: every overlap is `same`
            return SAME
        dot = (b[0] - a[0]) * (d[0] - c[0]) + (b[1] - a[1]) * (d[1] - c[1])
        return SAME if dot > 0 else OPPOSITE
    return {V.CROSS: CROSS, V.VV: VV, V.VE: VE, None: None}[what]


def live_edges(geo, incomplete):
    """[(id, a, b)] of the live edges of the complete ids."""
    out = []
    for i in sorted(geo):
        if i in incomplete:
            continue
        for ring in geo[i]:
            n = len(ring)
            out += [(i, ring[k], ring[(k + 1) % n]) for k in range(n) if ring[k] != ring[(k + 1) % n]]
    return out


def conflicts(table, frac_bits, max_ids, over_work=False, ring_limit=16384, same_id=False, direction=True, strict=True):
    """dict(conflict i64 [max_ids, 8], counts i64 [8], info i64 [8]) as the call defines them.  `over_work` states that the
    implementation's work exceeds the cap: the grid is not restated here, so the caller says which side of the cap it is on."""
    geo, incomplete, top = geometry(*table, frac_bits, max_ids, ring_limit)
    rows = np.zeros((max_ids, 8), dtype=np.int64)
    counts = np.zeros(8, dtype=np.int64)
    info = np.zeros(8, dtype=np.int64)
    edges = live_edges(geo, incomplete)
    info[0] = len(edges)
    m = {}
    for i, _, _ in edges:
        m[i] = m.get(i, 0) + 1
    checked = set()
    for i in range(1, top + 1):
        if i in incomplete:
            rows[i - 1, 0] = 2
            counts[3] += 1
        elif m.get(i, 0) == 0:
            rows[i - 1, 0] = 1
            counts[2] += 1
        else:
            rows[i - 1, 2] = m[i]
            if over_work:
                rows[i - 1, 0] = 3
                counts[4] += 1
            else:
                checked.add(i)
                counts[0] += 1
    if not over_work:
        once = {CROSS: 0, SAME: 0, OPPOSITE: 0, VV: 0, VE: 0}
        partner = {}
        for (i, a, b), (j, c, d) in itertools.combinations(edges, 2):
            if i == j and not same_id:
                continue
            what = pair_class(a, b, c, d, direction, strict)
            if what is None:
                continue
            once[what] += 1
            rows[i - 1, COLUMNS[what]] += 1
            if i != j:
                rows[j - 1, COLUMNS[what]] += 1
            if what in (CROSS, SAME) and i != j:
                partner[i] = min(partner.get(i, j), j)
                partner[j] = min(partner.get(j, i), i)
        for i, j in partner.items():
            rows[i - 1, 1] = j
        counts[1] = sum(1 for i in checked if rows[i - 1, 3] + rows[i - 1, 4] > 0)
        counts[5], counts[6] = once[CROSS], once[SAME]
        info[6], info[7] = once[OPPOSITE], once[VV] + once[VE]
    counts[7] = int(table[2][4])
    return dict(conflict=rows, counts=counts, info=info)
