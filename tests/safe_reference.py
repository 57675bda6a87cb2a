"""Independent restatement of `c3d_outlines_simplify_safe` (include/change3d_hip.h) in plain Python, over the restatements it
builds on: the labels, the augmented ring, its start and the per-arc Douglas-Peucker are `shared_reference`'s, the class of a
pair of edges is `valid_reference.classify`.  Levels live in a dict by arc key, the defective pairs are found over all
unordered pairs of live edges by `itertools.combinations`: no grid, no cells, no bounding boxes, no tiers, no launches.
`detect_numpy` is a second, independent count of the same pairs over all pairs at once in numpy int64, which the survey uses
for speed and which tests/test_safe_cpu.py holds against the plain one.  `grid_work` restates the work of the detector's grid,
which is the rule of c3d_rings_conflicts over the live output edges.  `per_ring=True` and `touch_ve=False` are the two
deliberately wrong variants of the negative controls."""
import itertools

import numpy as np

import shared_reference as R
import valid_reference as V
from simplify_reference import ST_BAD_COUNTS, ST_BAD_INPUT, ST_TRUNCATED, shoelace2

ST_CONVERGED, ST_NOT_CONVERGED, ST_DEFECTS_LEFT, ST_OVER_WORK = 0, 1, 2, 3
DIRS = {(1, 0): 0, (0, 1): 1, (-1, 0): 2, (0, -1): 3}        # as the tracer numbers sides: top +x, right +y, bottom -x, left -y
INT_MAX = 2 ** 31 - 1


def level_cap(q):
    """The smallest L with q >> 2 L == 0."""
    L = 0
    while q >> (2 * L):
        L += 1
    return L


def _step(p, q):
    return DIRS[((q[0] > p[0]) - (q[0] < p[0]), (q[1] > p[1]) - (q[1] < p[1]))]


def arc_key(pts, i, j, Ws):
    """The key of the arc pts[i] .. pts[j] of a rotated augmented ring with its closing repeat: the smaller of (start, first unit
    step) and (end, reverse of the last unit step)."""
    key = lambda v, d: 4 * (v[1] * (Ws + 1) + v[0]) + d  # noqa: E731
    return min(key(pts[i], _step(pts[i], pts[i + 1])), key(pts[j], (_step(pts[j - 1], pts[j]) + 2) % 4))


def prepare(labels, counts_obj, rings, vertices, counts, max_objects=65536):
    """What does not depend on the levels: per ring row either None (not simplified) or dict(aug = the rotated augmented ring,
    pts with the closing repeat, arcs = [(i, j, key)]), and the counts, status and first five info elements."""
    rings, vertices, counts = np.asarray(rings), np.asarray(vertices), np.asarray(counts)
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    found, rows_in, _, written_in, status = (int(c) for c in counts)
    prep = dict(max_rings=max_rings, max_vertices=max_vertices, found=found, bad_counts=bool(status & ST_BAD_COUNTS), rows=[], head=[],
                info=[0] * 5)
    if prep["bad_counts"]:
        return prep
    lab = R.Labels(labels, counts_obj, max_objects)
    n_rows, limit = min(max(rows_in, 0), max_rings), min(max(written_in, 0), max_vertices)
    V_, room = vertices.tolist(), 0
    for rid, start, n, area, perimeter, x, y, _ in rings[:n_rows].tolist():
        prep["head"].append((rid, area, perimeter, x, y, n))
        ring = None
        if start >= 0:
            aug = None
            if n >= 4 and start + n <= limit:
                aug = R.augment([tuple(p) for p in V_[start:start + n]], lab)
            if aug is not None:
                fits = room + len(aug) <= 2 * max_vertices
                room += len(aug)
                aug = aug if fits else None
            if aug is None:
                status |= ST_BAD_INPUT
            else:
                aug = R.rotate(aug)
                m = len(aug)
                pts = [(a[0], a[1]) for a in aug] + [(aug[0][0], aug[0][1])]
                ends = ([k for k in range(m) if aug[k][2]] or [0]) + [m]
                arcs = [(i, j, arc_key(pts, i, j, lab.W)) for i, j in zip(ends[:-1], ends[1:])]
                prep["info"][0] += sum(a[4] for a in aug)
                prep["info"][1] += sum(a[2] for a in aug)
                prep["info"][2] += len(arcs)
                prep["info"][3] += sum(pts[i] == pts[j] for i, j, _ in arcs)
                prep["info"][4] += sum(aug[i][3] > 0 for i, _, _ in arcs)
                ring = dict(aug=aug, pts=pts, arcs=arcs)
        prep["rows"].append(ring)
    prep["status"] = status
    return prep


def _slot(r, key, per_ring):
    return (r, key) if per_ring else key                      # the wrong rule: every ring keeps levels of its own


def simplify_round(prep, q, levels, max_out, per_ring=False):
    """One simplify step with the current levels: the shared call's outputs, `level` beside `left`, and per written row the
    arc slot of every output edge."""
    out_r = np.zeros((prep["max_rings"], 8), dtype=np.int32)
    out_v = np.zeros((max_out, 2), dtype=np.int32)
    out_l = np.zeros(max_out, dtype=np.int32)
    out_lv = np.zeros(max_out, dtype=np.int32)
    info = np.zeros(8, dtype=np.int32)
    if prep["bad_counts"]:
        return dict(rings=out_r, vertices=out_v, left=out_l, level=out_lv, counts=np.array([0, 0, 0, 0, ST_BAD_COUNTS], dtype=np.int32),
                    info=info, slots={})
    at = written = 0
    slots = {}
    for r, (ring, (rid, _, perimeter, x, y, n)) in enumerate(zip(prep["rows"], prep["head"])):
        if ring is None:
            out_r[r] = (rid, -1, 0, 0, perimeter, x, y, n)
            continue
        aug, pts = ring["aug"], ring["pts"]
        kept = []
        for i, j, key in ring["arcs"]:
            L = levels.get(_slot(r, key, per_ring), 0)
            inner = R.simplify_arc(pts[i:j + 1], q >> (2 * L))
            kept += [(k, L, _slot(r, key, per_ring)) for k in [i] + [i + t for t in inner]]
        if at + len(kept) <= max_out:
            p = [pts[k] for k, _, _ in kept]
            area2 = shoelace2(p)
            out_r[r] = (rid, at, len(kept), area2, perimeter, p[0][0], p[0][1], n)
            out_v[at:at + len(kept)] = p
            out_l[at:at + len(kept)] = [aug[k][3] for k, _, _ in kept]
            out_lv[at:at + len(kept)] = [L for _, L, _ in kept]
            slots[r] = [s for _, _, s in kept]
            written = at + len(kept)
            info[5] += len(kept) < 3 or area2 == 0
        else:
            out_r[r] = (rid, -1, 0, 0, perimeter, x, y, n)
        at += len(kept)
    info[:5] = prep["info"]
    status = prep["status"] | (ST_TRUNCATED if at > written else 0)
    return dict(rings=out_r, vertices=out_v, left=out_l, level=out_lv, counts=np.array([prep["found"], len(prep["rows"]), at, written, status],
                                                                                      dtype=np.int32), info=info, slots=slots)


def edges_of(out):
    """[(id, ring row, k, n', slot, a, b)] of the live edges of every written ring, whatever its n'."""
    V_, edges = out["vertices"].tolist(), []
    for r, slot in sorted(out["slots"].items()):
        rid, start, n = (int(v) for v in out["rings"][r, :3])
        ring = [tuple(p) for p in V_[start:start + n]]
        edges += [(rid, r, k, n, slot[k], ring[k], ring[(k + 1) % n]) for k in range(n) if ring[k] != ring[(k + 1) % n]]
    return edges


def defective(e, f, touch_ve=True):
    """Is the unordered pair of distinct live edges defective."""
    (i, ri, ki, ni, _, a, b), (j, rj, kj, _, _, c, d) = e, f
    adjacent = ri == rj and (ki - kj) % ni in (1, ni - 1)
    what = V.classify(a, b, c, d, adjacent=adjacent)
    if what == V.CROSS:
        return True
    if what == V.OVERLAP:
        return not (i != j and (b[0] - a[0]) * (d[0] - c[0]) + (b[1] - a[1]) * (d[1] - c[1]) < 0)   # a shared wall
    return what == V.VE and touch_ve


def detect(edges, touch_ve=True):
    """(the slots marked, defective pairs) over every unordered pair of live edges."""
    marks, pairs = set(), 0
    for e, f in itertools.combinations(edges, 2):
        if defective(e, f, touch_ve):
            pairs += 1
            marks.update((e[4], f[4]))
    return marks, pairs


def detect_numpy(edges, touch_ve=True):
    """The same over all pairs at once in numpy int64; written from the rule, not from `defective`."""
    if len(edges) < 2:
        return set(), 0
    ids = np.array([e[0] for e in edges], dtype=np.int64)
    row = np.array([e[1] for e in edges], dtype=np.int64)
    k = np.array([e[2] for e in edges], dtype=np.int64)
    n = np.array([e[3] for e in edges], dtype=np.int64)
    a = np.array([e[5] for e in edges], dtype=np.int64)
    b = np.array([e[6] for e in edges], dtype=np.int64)
    m = len(edges)
    ev = b - a
    A, B, C, D, E, F = a[:, None, :], b[:, None, :], a[None, :, :], b[None, :, :], ev[:, None, :], ev[None, :, :]
    cr = lambda u, v: u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]  # noqa: E731
    o1, o2, o3, o4 = np.sign(cr(E, C - A)), np.sign(cr(E, D - A)), np.sign(cr(F, A - C)), np.sign(cr(F, B - C))
    once = np.arange(m)[:, None] < np.arange(m)[None, :]
    diff = (k[:, None] - k[None, :]) % n[:, None]
    adjacent = (row[:, None] == row[None, :]) & ((diff == 1) | (diff == n[:, None] - 1))
    cross = (o1 * o2 < 0) & (o3 * o4 < 0)
    coll = (o1 == 0) & (o2 == 0) & (o3 == 0) & (o4 == 0)
    tc, td, L = ((C - A) * E).sum(-1), ((D - A) * E).sum(-1), (E * E).sum(-1)
    lo, hi = np.maximum(np.minimum(tc, td), 0), np.minimum(np.maximum(tc, td), L)
    wall = (ids[:, None] != ids[None, :]) & ((E * F).sum(-1) < 0)
    overlap = coll & (lo < hi) & ~wall
    contact = ~cross & ~coll & ~(o1 * o2 > 0) & ~(o3 * o4 > 0)
    ends = (A == C).all(-1) | (A == D).all(-1) | (B == C).all(-1) | (B == D).all(-1)
    bad = cross | overlap
    if touch_ve:
        bad = bad | (contact & ~ends & ~adjacent)
    bad &= once
    hit = np.flatnonzero(bad.any(1) | bad.any(0))
    return {edges[t][4] for t in hit.tolist()}, int(bad.sum())


def defective_rings(prep, out):
    """The written rows whose ring is defective: n' < 3, or an area whose sign is not that of the input row."""
    sign = lambda v: (v > 0) - (v < 0)  # noqa: E731
    return [r for r in sorted(out["slots"]) if int(out["rings"][r, 2]) < 3 or sign(int(out["rings"][r, 3])) != sign(prep["head"][r][1])]


def grid_work(edges, limits):
    """(shift, work, the most entries of a cell) of the detector's grid: the rule of c3d_rings_conflicts with n = the live output
    edges; limits[0], [1] = the entry and cell budgets per live edge."""
    if not edges:
        return 0, 0, 0
    bx = np.array([(min(a[0], b[0]), max(a[0], b[0]), min(a[1], b[1]), max(a[1], b[1])) for *_, a, b in edges], dtype=np.int64)
    x0, y0 = bx[:, 0].min(), bx[:, 2].min()
    wx, wy = bx[:, 1].max() - x0, bx[:, 3].max() - y0
    for s in range(26):
        lo_x, hi_x, lo_y, hi_y = (bx[:, 0] - x0) >> s, (bx[:, 1] - x0) >> s, (bx[:, 2] - y0) >> s, (bx[:, 3] - y0) >> s
        entries = int(((hi_x - lo_x + 1) * (hi_y - lo_y + 1)).sum())
        if entries <= limits[0] * len(bx) and (int(wx >> s) + 1) * (int(wy >> s) + 1) <= limits[1] * len(bx):
            break
    cells = {}
    for ax, bx_, ay, by in zip(lo_x.tolist(), hi_x.tolist(), lo_y.tolist(), hi_y.tolist()):
        for y in range(ay, by + 1):
            for x in range(ax, bx_ + 1):
                cells[(x, y)] = cells.get((x, y), 0) + 1
    return s, sum(c * (c - 1) // 2 for c in cells.values()), max(cells.values())


def simplify_safe(labels, counts_obj, rings, vertices, counts, q, max_rounds=8, max_work=2 ** 32, limits=(2, 4), max_objects=65536,
                  max_vertices_out=None, per_ring=False, touch_ve=True, fast=False, start_levels=None, history=None, prep=None):
    """dict(rings, vertices, left, level, counts, info, safe i64 [8], work) as the call defines them; info[6], [7] = the shift and
    the work (saturated) of the last round's grid.  `history` collects (output, marks, pairs, defective rows) of every round."""
    assert 0 <= q <= R.TOL2_Q_MAX and 1 <= max_rounds <= 64
    prep = prepare(labels, counts_obj, rings, vertices, counts, max_objects) if prep is None else prep
    max_out = 2 * prep["max_vertices"] if max_vertices_out is None else int(max_vertices_out)
    cap = level_cap(q)
    levels = dict(start_levels or {})
    all_slots = {_slot(r, key, per_ring) for r, ring in enumerate(prep["rows"]) if ring is not None for _, _, key in ring["arcs"]}
    safe = np.zeros(8, dtype=np.int64)
    find = detect_numpy if fast else detect
    out = None
    for rnd in range(max_rounds):
        out = simplify_round(prep, q, levels, max_out, per_ring)
        safe[0] += 1
        safe[2] = sum(1 for s in all_slots if levels.get(s, 0) > 0)
        safe[3] = sum(1 for s in all_slots if levels.get(s, 0) == cap)
        edges = edges_of(out)
        bad_rows = defective_rings(prep, out)
        shift, work, most = grid_work(edges, limits)
        out["info"][6], out["info"][7], out["work"], out["most"] = shift, min(work, INT_MAX), work, most
        if rnd == 0:
            safe[6] = len(bad_rows)
        if work > max_work:
            safe[5], safe[7] = 0, ST_OVER_WORK
            break
        marks, pairs = find(edges, touch_ve)
        for r in bad_rows:
            marks.update(out["slots"][r])
        if history is not None:
            history.append((out, set(marks), pairs, bad_rows))
        if rnd == 0:
            safe[4] = pairs
        safe[5] = pairs
        if not marks:
            safe[7] = ST_CONVERGED
            break
        up = [s for s in marks if levels.get(s, 0) < cap]
        if not up:
            safe[7] = ST_DEFECTS_LEFT
            break
        for s in up:
            levels[s] = levels.get(s, 0) + 1
        safe[1] += 1
        if rnd == max_rounds - 1:
            safe[7] = ST_NOT_CONVERGED
    out["safe"] = safe
    out["levels"] = levels
    return out
