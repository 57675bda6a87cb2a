"""Plain restatement of `c3d_scene_edt` and `c3d_boundary_counts` (include/change3d_hip.h) in exact integer numpy: the column
distances by `np.minimum.accumulate` / `np.maximum.accumulate`, the rows by a W x W minimum per row.  Cheap enough for the
shapes of the tests, not for a scene.  tests/test_edt_cpu.py checks it against scipy and against a brute-force minimum."""
import numpy as np

FAR = 0x3fffffff
INVERT, BORDER = 1, 2
_NONE = 1 << 20                                             # a column distance that means "no site": above every true one


def column_distance(site):
    """int64 [H, W]: the distance along the column to the nearest True of `site`, `_NONE` or more where the column has none."""
    H = site.shape[0]
    rows = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(site, rows, -_NONE), axis=0)            # the nearest site row <= y
    below = np.minimum.accumulate(np.where(site, rows, 2 * _NONE)[::-1], axis=0)[::-1]  # the nearest site row >= y
    return np.minimum(rows - above, below - rows)


def apply_cap(full, cap2, cap_strict=False):
    """The cap rule on an uncapped transform: a value above `cap2` > 0 becomes FAR.  `cap_strict=True` is the WRONG rule (`<`
    for `<=`), for a negative control."""
    if cap2 <= 0:
        return full
    return np.where((full >= cap2) if cap_strict else (full > cap2), FAR, full).astype(np.int32)


def edt2(mask, invert=False, border=False, cap2=0, cap_strict=False):
    """i32 [H, W] as `c3d_scene_edt` defines it."""
    mask = np.asarray(mask)
    assert mask.ndim == 2 and mask.shape[0] <= 16384 and mask.shape[1] <= 16384 and cap2 >= 0
    site = (mask != 0) if invert else (mask == 0)
    if border:
        site = np.pad(site, 1, constant_values=True)
    col = column_distance(site)
    g2 = np.where(col >= _NONE, 1 << 30, col * col).astype(np.int32)    # a true value stays below 2^30, a sum below 2^31
    W = site.shape[1]
    xs = np.arange(W, dtype=np.int32)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                   # [x, x']
    out = np.empty(site.shape, dtype=np.int32)
    for y in range(site.shape[0]):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    if border:
        out = out[1:-1, 1:-1]
    return apply_cap(np.where(out >= 1 << 30, FAR, out).astype(np.int32), cap2, cap_strict)


def boundary_counts(P, G, d2, tau2, border=True):
    """The i64 [8] of `c3d_boundary_counts` as a tuple of ints."""
    P, G = np.asarray(P) != 0, np.asarray(G) != 0
    assert P.shape == G.shape and d2 >= 1 and tau2 >= 1
    dP, dG = edt2(P, border=border), edt2(G, border=border)
    Pd, Gd = P & (dP <= d2), G & (dG <= d2)
    Pc, Gc = P & (dP == 1), G & (dG == 1)
    eG, eP = edt2(Gc, invert=True), edt2(Pc, invert=True)
    return (int((Pd & Gd).sum()), int((Pd | Gd).sum()), int(Pc.sum()), int((Pc & (eG <= tau2)).sum()), int(Gc.sum()),
            int((Gc & (eP <= tau2)).sum()), 1, 0)


def disc(shape, cy, cx, r):
    """u8 [H, W]: the pixels within `r` of (cy, cx)."""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)


def brute2(mask, invert=False, border=False):
    """The definition itself, O((H W)^2): for tiny shapes."""
    mask = np.asarray(mask)
    site = (mask != 0) if invert else (mask == 0)
    if border:
        site = np.pad(site, 1, constant_values=True)
    sy, sx = np.nonzero(site)
    H, W = site.shape
    out = np.full((H, W), FAR, dtype=np.int64)
    if len(sy):
        yy, xx = np.mgrid[0:H, 0:W]
        out = ((yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2).min(axis=2)
    if border:
        out = out[1:-1, 1:-1]
    return out.astype(np.int32)
