"""The key maps that the region and sieve tests share, and the hand-counted sieve cases."""
import numpy as np


def block_noise(H, W, classes, seed, block=4, noise=0.25):
    """Blocks of `block` x `block` pixels of keys from {0 .. classes-1}, a quarter of the pixels replaced by iid keys: the maps
    of the survey (20 x 20 there: 5 x 5 blocks)."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, classes, size=((H + block - 1) // block, (W + block - 1) // block), dtype=np.uint8)
    m = np.kron(coarse, np.ones((block, block), dtype=np.uint8))[:H, :W]
    hit = rng.random((H, W)) < noise
    return np.where(hit, rng.integers(0, classes, size=(H, W), dtype=np.uint8), m).astype(np.uint8)


def iid(H, W, k, seed):
    """iid keys from {0 .. k}"""
    return np.random.default_rng(seed).integers(0, k + 1, size=(H, W), dtype=np.uint8) if k < 255 else \
        np.random.default_rng(seed).integers(0, 256, size=(H, W)).astype(np.uint8)


def key_maps(H, W, seed=0):
    """list of (name, u8 [H, W]): the maps every scene size is labelled with."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = [(f"iid{k}", iid(H, W, k, seed + k)) for k in (1, 3, 49, 255)]
    out.append(("blocks4", block_noise(H, W, 4, seed + 1)))
    out.append(("blocks7", block_noise(H, W, 7, seed + 2, block=16)))
    out.append(("nozero", (1 + iid(H, W, 2, seed + 3)).astype(np.uint8)))
    out.append(("one_key", np.full((H, W), 7, np.uint8)))
    out.append(("zero", np.zeros((H, W), np.uint8)))
    # 4-connectivity: every pixel a region; 8-connectivity: two regions that cross at every lattice point
    out.append(("checkerboard", (1 + (yy + xx) % 2).astype(np.uint8)))
    # one-pixel stripes: every seam pixel has an equal key two away and another one next to it
    out.append(("stripes_v", (1 + xx % 2).astype(np.uint8)))
    out.append(("stripes_h", (3 + yy % 2).astype(np.uint8)))
    # key 1 winds through key 2: even rows full, odd rows joined at alternating ends; one region of key 1, long walks over seams
    snake = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == W - 1)) | ((yy % 4 == 3) & (xx == 0))
    out.append(("serpentine", np.where(snake, 1, 2).astype(np.uint8)))
    ring = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    out.append(("rings", (1 + ring % 3).astype(np.uint8)))
    return out


def _grid(rows):
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


# name -> (map, min_area, connectivity, the map after convergence).  Hand-counted; the comments give the borders in sides.
HAND = {
    # a speck of key 2 inside a region of key 1: border 4 with it, no other neighbour
    "speck_inside": (_grid(["111", "121", "111"]), 2, 4, _grid(["111", "111", "111"])),
    # the speck 3 (2 pixels) has 4 sides with key 1 (area 6) and 2 with key 2 (area 8): the longer border beats the larger area
    "longer_border": (_grid(["1122", "1322", "1322", "1122"]), 3, 4, _grid(["1122", "1122", "1122", "1122"])),
    # one side each with key 1 (area 2) and key 2 (area 3): the larger area wins
    "larger_area": (_grid(["113222"]), 2, 4, _grid(["112222"])),
    # one side each, both of area 2: the smaller root (key 1, first in raster order) wins
    "smaller_root": (_grid(["11322"]), 2, 4, _grid(["11122"])),
    # one side with the background (2 zero pixels) and one with key 2 (area 2): a full tie, the background wins
    "bg_full_tie": (_grid(["00322"]), 2, 4, _grid(["00022"])),
    # key 1 (area 2, root 0) and key 2 (area 2, root 2), both small, each the other's only neighbour: exactly the lower
    # (area, root), key 1, moves
    "mutual_pair": (_grid(["1122"]), 3, 4, _grid(["2222"])),
    # 5 -> 4 -> 3 -> key 1 (area 4, not small): areas 1, 2, 3 rise, every target is the next one; all take key 1 in one round
    "chain_of_three": (_grid(["5443331111"]), 4, 4, _grid(["1111111111"])),
    # the speck 2 separates two regions of key 1; it joins one of them and the two are ONE region from the next round on
    "merge_after": (_grid(["11211"]), 2, 4, _grid(["11111"])),
    # a small region that is the whole scene: no neighbour, no target; it stays and the call has converged
    "whole_scene": (_grid(["22", "22"]), 100, 8, _grid(["22", "22"])),
}


def stretch(name, most=320):
    """A hand case blown up by s x s per pixel so that r and its target lie in different tiles: borders grow by s, areas and
    the area bound by s * s, first pixels keep their raster order, so every comparison of the rule, every tie included, is the
    one of the small case.  Returns (map, min_area, connectivity, the map after convergence)."""
    m, min_area, connectivity, want = HAND[name]
    s = min(33, most // m.shape[1])
    one = np.ones((s, s), dtype=np.uint8)
    return np.kron(m, one), min_area * s * s, connectivity, np.kron(want, one)
