"""Independent restatement of `c3d_scene_split` (include/change3d_hip.h) in numpy and plain Python: the core from
`edt_reference.edt2`, the seeds from `objects_reference.components`, the growth by a heap Dijkstra over (d, id) (and, to check
it, by a level-synchronous BFS), the table from `objects_reference.objects(labels0=...)`.  Nothing here shares code with the
kernels: no tiles, no rounds, no union-find.  Also the masks of the hand-made cases."""
import heapq

import numpy as np

import edt_reference as E
import objects_reference as R

NOT_CONVERGED, BAD_LABELS = 1, 2


def core_of(mask, r2):
    """bool [H, W]: mask != 0 and dist2 > r2, the outside of the scene being background."""
    fg = np.asarray(mask) != 0
    if r2 == 0:
        return fg
    return fg & (E.edt2(mask, border=True, cap2=r2) > r2)


def seed_ids(core, connectivity):
    """(ids i64 [H, W], n): the linear index of the first pixel of the seed that holds the pixel, -1 outside the core."""
    comp = R.components(core.astype(np.uint8), connectivity)
    n = int(comp.max())
    H, W = comp.shape
    first = np.full(n + 1, -1, dtype=np.int64)
    flat = comp.ravel()
    idx = np.nonzero(flat)[0]
    first[flat[idx][::-1]] = idx[::-1]                      # the smallest index wins: written last
    return np.where(comp > 0, first[comp], -1).reshape(H, W), n


def grow_dijkstra(mask, ids, connectivity, ties="low"):
    """(d, owner) i64 [H, W]: the lexicographically smallest (d(p, s), id(s)) per mask pixel, -1 where no seed reaches.
    `ties="high"` is the WRONG rule (the largest id wins at equal distance), kept for the negative control."""
    fg = (np.asarray(mask) != 0).tolist()
    H, W = ids.shape
    sign = 1 if ties == "low" else -1
    d = [[-1] * W for _ in range(H)]
    own = [[-1] * W for _ in range(H)]
    heap = [(0, sign * int(ids[y, x]), y, x) for y in range(H) for x in range(W) if ids[y, x] >= 0]
    heapq.heapify(heap)
    steps = R.NEIGHBOURS[connectivity]
    while heap:
        dist, sid, y, x = heapq.heappop(heap)
        if d[y][x] >= 0:
            continue
        d[y][x], own[y][x] = dist, sign * sid
        for dy, dx in steps:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and fg[yy][xx] and d[yy][xx] < 0:
                heapq.heappush(heap, (dist + 1, sid, yy, xx))
    return np.asarray(d, dtype=np.int64).reshape(H, W), np.asarray(own, dtype=np.int64).reshape(H, W)


def grow_bfs(mask, ids, connectivity):
    """The same map level by level: every pixel of level d + 1 takes the smallest id among its neighbours of level d."""
    fg = np.asarray(mask) != 0
    H, W = ids.shape
    BIG = np.int64(1) << 40
    own = np.where(ids >= 0, ids, BIG)
    d = np.where(ids >= 0, 0, -1).astype(np.int64)
    frontier = ids >= 0
    level = 0
    while frontier.any():
        cand = np.full((H, W), BIG, dtype=np.int64)
        src = np.where(frontier, own, BIG)
        for dy, dx in R.NEIGHBOURS[connectivity]:
            shifted = np.full((H, W), BIG, dtype=np.int64)
            ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
            xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
            shifted[yd, xd] = src[ys, xs]
            cand = np.minimum(cand, shifted)
        frontier = fg & (d < 0) & (cand < BIG)
        level += 1
        d[frontier] = level
        own[frontier] = cand[frontier]
    return d, np.where(d >= 0, own, -1)


def piece_labels(mask, owner, connectivity):
    """i32 [H, W]: the pieces numbered 1.. in raster order of their own first pixel, before any area filter.  A pixel that no seed
    reached keeps its component."""
    comp = R.components(mask, connectivity)
    n_comp = int(comp.max())
    H, W = comp.shape
    keyed = np.where(owner >= 0, owner + n_comp + 1, comp).ravel()   # one key per piece; 0 on the background
    keys, first = np.unique(keyed, return_index=True)
    keep = keys > 0
    keys, first = keys[keep], first[keep]
    order = np.argsort(first, kind="stable")
    number = np.zeros(len(keys), dtype=np.int32)
    number[order] = np.arange(1, len(keys) + 1, dtype=np.int32)
    out = np.zeros(H * W, dtype=np.int32)
    fgi = np.nonzero(keyed)[0]
    out[fgi] = number[np.searchsorted(keys, keyed[fgi])]
    return out.reshape(H, W)


def split(mask, r2, cls_map=None, score=None, connectivity=8, min_area=1, n_cls=1, first_class=1, max_objects=65536, ties="low"):
    """dict(labels, table, hist, object_cls, counts as `objects_reference.objects` returns them, info i32 [2] = (status 0, number
    of seeds), depth = the largest d)."""
    core = core_of(mask, r2)
    ids, n_seeds = seed_ids(core, connectivity)
    d, owner = grow_dijkstra(mask, ids, connectivity, ties)
    labels0 = piece_labels(mask, owner, connectivity)
    out = R.objects(mask, cls_map, score, connectivity=connectivity, min_area=min_area, n_cls=n_cls, first_class=first_class,
                    max_objects=max_objects, labels0=labels0)
    out["info"] = np.array([0, n_seeds], dtype=np.int32)
    out["depth"] = int(d.max()) if d.size else 0
    out["labels0"] = labels0
    return out


def pieces_are_connected(labels, connectivity):
    """Every label of `labels` is one c-connected set: a flood fill that only steps between equal labels finds each label once."""
    lab = np.asarray(labels).tolist()
    H, W = len(lab), len(lab[0])
    seen = [[False] * W for _ in range(H)]
    found = set()
    for y0 in range(H):
        for x0 in range(W):
            k = lab[y0][x0]
            if not k or seen[y0][x0]:
                continue
            if k in found:
                return False
            found.add(k)
            seen[y0][x0] = True
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in R.NEIGHBOURS[connectivity]:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and lab[yy][xx] == k and not seen[yy][xx]:
                        seen[yy][xx] = True
                        stack.append((yy, xx))
    return True


# ---------------------------------------------------------------------------------------------------------------- the cases
def two_discs():
    return (E.disc((96, 160), 48, 50, 30) | E.disc((96, 160), 48, 100, 30)).astype(np.uint8)


def dumbbell():
    """Two 20 x 20 blocks joined by a neck 2 px high and 12 px long."""
    m = np.zeros((30, 64), np.uint8)
    m[5:25, 4:24] = 1
    m[5:25, 36:56] = 1
    m[14:16, 24:36] = 1
    return m


def bridged_grid():
    """A grid of 9 x 9 blocks, 3 px apart, joined by 1-px bridges: one component, one seed per block at r2 = 4."""
    n, b, g = 6, 9, 3
    S = n * b + (n + 1) * g
    m = np.zeros((S, S), np.uint8)
    for i in range(n):
        for j in range(n):
            y, x = g + i * (b + g), g + j * (b + g)
            m[y:y + b, x:x + b] = 1
            if j + 1 < n:
                m[y + b // 2, x + b:x + b + g] = 1
            if i + 1 < n:
                m[y + b:y + b + g, x + b // 2] = 1
    return m


def ring():
    """A thin ring (no seed at r2 = 4) around a block (one seed), not touching; and a second block touching the ring."""
    m = np.zeros((48, 80), np.uint8)
    m[4:44, 4:44] = 1
    m[6:42, 6:42] = 0                                         # the ring, 2 px thick
    m[16:32, 16:32] = 1                                       # a block inside it, apart
    m[12:36, 44:70] = 1                                       # a block that touches the ring: a seeded piece next to thin arms
    return m


def thick_serpentine(H=67, W=131):
    """Corridors 3 px high on rows y % 4 != 3, joined by 3-px-wide links at alternating ends, and a 7 x 7 block at (0, 0): with
    r2 = 4 only the block holds a seed, and the front walks the whole serpentine.  Only whole periods of four rows (corridor and
    link row) are drawn: at H = 67 the rows 64..66 stay background, and the last link row ends in a stub."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = (yy % 4 != 3)
    link_right = (yy % 8 == 3) & (xx >= W - 3)
    link_left = (yy % 8 == 7) & (xx < 3)
    m = (m | link_right | link_left) & (yy < H // 4 * 4)
    m[0:7, 0:7] = True
    return m.astype(np.uint8)


def hand_cases():
    """list of (name, mask u8, r2)."""
    return [("two_discs", two_discs(), 400), ("dumbbell", dumbbell(), 4), ("bridged_grid", bridged_grid(), 4), ("ring", ring(), 4),
            ("thick_serpentine", thick_serpentine(), 4)]
