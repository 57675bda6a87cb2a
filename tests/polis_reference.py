"""Independent restatement of `c3d_rings_polis` (include/change3d_hip.h) in plain Python: integers up to the one quotient and
the square root of a distance, sequential sums.  No tiers, no jobs, no grouping step: nothing here shares an idea with the
kernels beyond the rule itself.  The three keyword switches turn the rule into the wrong ones of the negative controls."""
import math

import numpy as np

ST_BAD_COUNTS = 2                                        # C3D_OUTLINE_ST_BAD_COUNTS
ST_BAD_PARTNER = 512                                     # C3D_POLIS_ST_BAD_PARTNER
COORD_UNITS = 32768
U = 2.0 ** -53


def value(p, a, b, segment=True):
    """v of the header for the point p and the edge (a, b): the squared distance as a double."""
    ex, ey, wx, wy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    L, t, c = ex * ex + ey * ey, wx * ex + wy * ey, wx * ey - wy * ex
    if L == 0 or (segment and t <= 0):
        return float(wx * wx + wy * wy)
    if segment and t >= L:
        return float((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2)
    return (float(c) * float(c)) / float(L)


def edges_of(ring_list, closing=True, join=False):
    """The edges of an id's rings (lists of points): per ring, or, wrongly, over the concatenated vertex list."""
    if join:
        ring_list = [[p for ring in ring_list for p in ring]]
    out = []
    for ring in ring_list:
        n = len(ring)
        out += [(ring[k], ring[(k + 1) % n]) for k in range(n if closing else n - 1)]
    return out


def distances(points, edges, segment=True):
    return [math.sqrt(min(value(p, a, b, segment) for a, b in edges)) for p in points]


def geometry(rings, vertices, counts, f, max_ids, ring_limit):
    """({id: list of rings, each a list of (x, y)}, set of incomplete ids, largest id seen) by the header's rule."""
    max_rings, max_vertices = len(rings), len(vertices)
    rows = 0 if int(counts[4]) & ST_BAD_COUNTS else min(max(int(counts[1]), 0), max_rings)
    vlimit = min(max(int(counts[3]), 0), max_vertices)
    cmax = COORD_UNITS << f
    geo, incomplete, top = {}, set(), 0
    for r in range(rows):
        i, start, n = (int(v) for v in rings[r, :3])
        if not 1 <= i <= max_ids:
            continue
        top = max(top, i)
        ok = start >= 0 and n >= 0 and start + n <= vlimit
        if ok and n:
            ok = bool((np.abs(vertices[start:start + n].astype(np.int64)) <= cmax).all())
        if not ok:
            incomplete.add(i)
        elif n >= 3:
            geo.setdefault(i, []).append([(int(x), int(y)) for x, y in vertices[start:start + n].tolist()])
    at = 0
    for i in sorted(geo):
        if i in incomplete:
            continue
        if len(geo[i]) > ring_limit:
            incomplete.add(i)
            continue
        nv = sum(len(ring) for ring in geo[i])
        if at + nv > max_vertices:
            incomplete.add(i)
        at += nv
    return geo, incomplete, top


def polis(table_p, f_p, table_g, f_g, match_p, max_g, max_pair_work=2 ** 32, ring_limit=16384, segment=True, closing=True, join=False):
    """dict(pair f64 [max_p, 4], pair_n i32 [max_p, 4], counts i64 [8], sums f64 [4]) as the call defines them."""
    max_p = len(match_p)
    F = max(f_p, f_g)
    geo_p, inc_p, top = geometry(*table_p, f_p, max_p, ring_limit)
    geo_g, inc_g, _ = geometry(*table_g, f_g, max_g, ring_limit)
    pair = np.zeros((max_p, 4), dtype=np.float64)
    pair_n = np.zeros((max_p, 4), dtype=np.int32)
    counts = np.zeros(8, dtype=np.int64)
    sums = np.zeros(4, dtype=np.float64)
    status = int(table_p[2][4]) | int(table_g[2][4])

    def scaled(ring_list, f):
        return [[(x << (F - f), y << (F - f)) for x, y in ring] for ring in ring_list]

    for p in range(1, top + 1):
        g = int(match_p[p - 1][0])
        if not 0 <= g <= max_g:
            status |= ST_BAD_PARTNER
            g = 0
        rp = [] if p in inc_p else geo_p.get(p, [])
        rg = [] if (g < 1 or g in inc_g) else geo_g.get(g, [])
        n_p, n_g = sum(len(r) for r in rp), sum(len(r) for r in rg)
        if g == 0:
            flag = 1
        elif p in inc_p or g in inc_g or n_p == 0 or n_g == 0:
            flag = 2
        elif 2 * n_p * n_g > max_pair_work:
            flag = 3
        else:
            flag = 0
        pair_n[p - 1] = (g, n_p, n_g, flag)
        counts[flag] += 1
        if flag:
            continue
        rp, rg = scaled(rp, f_p), scaled(rg, f_g)
        d_pg = distances([v for ring in rp for v in ring], edges_of(rg, closing, join), segment)
        d_gp = distances([v for ring in rg for v in ring], edges_of(rp, closing, join), segment)
        mean_pg, mean_gp = sum(d_pg) / n_p / (1 << F), sum(d_gp) / n_g / (1 << F)
        pair[p - 1] = ((mean_pg + mean_gp) / 2, max(d_pg + d_gp) / (1 << F), mean_pg, mean_gp)
        counts[4] += n_p
        counts[5] += n_g
        sums[0] += pair[p - 1, 0]
        sums[1] += pair[p - 1, 1]
        sums[2] = max(sums[2], pair[p - 1, 1])
        sums[3] += n_p / n_g
    counts[6] = status
    return dict(pair=pair, pair_n=pair_n, counts=counts, sums=sums)


def bounds(pair_n):
    """Relative bounds (polis, hausdorff, mean_pg, mean_gp) per row from the header's error argument: a distance is within 8 u of
    the exact one, a mean over n of them within (n + 8) u, PoLiS within (n_p + n_g + 16) u."""
    n_p, n_g = pair_n[:, 1].astype(np.float64), pair_n[:, 2].astype(np.float64)
    return np.stack([(n_p + n_g + 16) * U, np.full_like(n_p, 8 * U), (n_p + 8) * U, (n_g + 8) * U], axis=1)
