"""Restatement of `c3d_regions_sieve` (include/change3d_hip.h) in numpy and plain Python.  The regions come from
tests/regions_reference.py; the border counts are taken per ordered pair of neighbouring region labels over the four shifted
views of the label map; targets, moves and chains are plain dictionaries.  No hash table, no atomics, no union-find."""
import numpy as np

import regions_reference as rref

ST_NOT_CONVERGED, ST_TABLE_FULL = 1, 2
BG = 0                                                      # the label of the background in a round's label map


def analyse(K, connectivity, min_area):
    """One round's decisions on the map K: dict(labels, n, n_small, entries, target {label: label or BG}, moves {label: end
    key}, longest chain)."""
    K = np.asarray(K, dtype=np.uint8)
    labels = rref.regions(K, connectivity)
    n = int(labels.max())
    flat = labels.ravel()
    area = np.bincount(flat, minlength=n + 1).astype(np.int64)             # area[BG] = the zero pixels of K
    root = np.full(n + 1, -1, dtype=np.int64)
    lab_u, first = np.unique(flat, return_index=True)
    root[lab_u] = first
    root[BG] = -1
    small = area < min_area
    small[BG] = False
    codes = []
    for a, b in ((labels[:-1], labels[1:]), (labels[1:], labels[:-1]), (labels[:, :-1], labels[:, 1:]), (labels[:, 1:], labels[:, :-1])):
        sel = (a != b) & small[a]                                          # a pixel of small a, a side with b outside a
        codes.append(a[sel].astype(np.int64) * (n + 1) + b[sel])
    codes, border = np.unique(np.concatenate(codes), return_counts=True)
    best = {}
    for c, cnt in zip(codes.tolist(), border.tolist()):
        r, nb = divmod(c, n + 1)
        cand = (cnt, int(area[nb]), -int(root[nb]), nb)                    # BG: root -1, so -root = 1 beats every region
        if r not in best or cand[:3] > best[r][:3]:
            best[r] = cand
    target = {r: c[3] for r, c in best.items()}
    moving = {}
    for r, t in target.items():
        if t == BG or not small[t] or (int(area[t]), int(root[t])) > (int(area[r]), int(root[r])):
            moving[r] = t
    key_of = np.zeros(n + 1, dtype=np.uint8)
    key_of[labels.ravel()] = K.ravel()
    moves, longest = {}, 0
    for r in moving:
        cur, steps = r, 0
        while cur in moving:                                               # rises in (area, root) among the small: ends
            cur = moving[cur]
            steps += 1
            if cur == BG:
                break
        moves[r] = 0 if cur == BG else int(key_of[cur])
        longest = max(longest, steps)
    return dict(labels=labels, n=n, n_small=int(small.sum()), entries=len(codes), target=target, moves=moves, longest=longest)


def paint(K, a):
    lut = np.zeros(a["n"] + 1, dtype=np.uint8)
    lut[a["labels"].ravel()] = np.asarray(K, dtype=np.uint8).ravel()
    lut[BG] = 0
    for r, k in a["moves"].items():
        lut[r] = k
    return lut[a["labels"]]


def sieve(key, min_area, connectivity=8, max_rounds=8, table_capacity=None):
    """dict(key_out u8 [H, W], info i32 [8], trace = per analysed round (regions, small, entries, moving, longest chain)).
    `table_capacity`: a round with more pairs than this many slots stops the call with ST_TABLE_FULL (the device table may
    also report it a little below that; the tests stay far away from the edge)."""
    K = np.array(key, dtype=np.uint8)
    status = rounds = moved = pixels = most = 0
    trace = []
    for rnd in range(max_rounds + 1):
        a = analyse(K, connectivity, min_area)
        trace.append((a["n"], a["n_small"], a["entries"], len(a["moves"]), a["longest"]))
        most = max(most, a["entries"])
        if table_capacity is not None and a["entries"] > table_capacity:
            status = ST_TABLE_FULL
            break
        if not a["moves"]:
            break
        if rnd == max_rounds:
            status = ST_NOT_CONVERGED
            break
        new = paint(K, a)
        rounds += 1
        moved += len(a["moves"])
        pixels += int((new != K).sum())
        K = new
    info = np.array([status, rounds, moved, pixels, trace[-1][1], trace[0][0], most, 0], dtype=np.int32)
    return dict(key_out=K, info=info, trace=trace)
