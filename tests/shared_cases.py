"""Inputs shared by tests/test_shared_cpu.py, tests/test_shared_gpu.py and tests/test_shared_infer_gpu.py: label maps written
down by hand, the survey masks of tests/valid_cases.py labelled four ways, and combs of a chosen number of augmented vertices.
A case is dict(labels i32 [H, W], counts_obj i32 [2], connectivity)."""
import functools

import numpy as np

import conflicts_cases as C
import objects_reference as O
import outlines_reference as T
import split_reference as SP
import valid_cases as K

TOLERANCES_HAND = (0.0, 0.5, 1.0, 2.0)


def case(rows, connectivity=4):
    lab = np.array(rows, dtype=np.int32)
    return dict(labels=lab, counts_obj=np.array([int(lab.max()), int(lab.max())], dtype=np.int32), connectivity=connectivity)


def grid(text):
    return [[int(ch) for ch in line] for line in text.split()]


def hand_made():
    out = {
        # the wall between 1 and 2 ends inside the upper wall of 3, which runs straight through the junction
        "t_junction": case(grid("""
            0000000
            0111220
            0111220
            0333330
            0333330
            0000000""")),
        "four_at_a_point": case(grid("""
            000000
            011220
            011220
            033440
            033440
            000000""")),
        # 1 touches itself across the diagonal, and so does 2
        "pinch_4": case(grid("""
            000000
            011200
            011200
            022100
            022110
            000000"""), 4),
        "pinch_8": case(grid("""
            000000
            011000
            011000
            000110
            000110
            000000"""), 8),
        # an island of 2 in the hole of 1: no node anywhere, the hole and the island's outline are each other's reverse
        "island": case(grid("""
            0000000000
            0111111110
            0112222110
            0112221110
            0122221110
            0112211110
            0111111110
            0000000000""")),
        # 2 hangs under the wall of 1: between its two nodes on that wall the rest of its ring falls under one chord at 2 px
        "collapse": case(grid("""
            00000000
            01111110
            01111110
            00220000
            00000000""")),
        # 3 is a neck one pixel wide between 1 and 2
        "neck": case(grid("""
            000000000
            011131220
            011131220
            011131220
            011333220
            011333220
            000000000""")),
        # 1 and 2 meet in the corner (3, 3) only: each ring has exactly one node and is one closed arc
        "one_node": case(grid("""
            0000000
            0110000
            0110000
            0002200
            0002200
            0000000"""), 4),
        "stairs": case(grid("""
            00000000000
            01111111110
            01111111220
            01111112220
            01111122220
            01111222220
            01112222220
            01122222220
            00000000000""")),
    }
    return out


def table(c, max_rings=None, max_vertices=None, max_objects=65536):
    """(rings, vertices, counts) that the restatement of c3d_scene_outlines writes for a case."""
    lab = c["labels"]
    o = T.outlines(lab, c["counts_obj"], c["connectivity"], max_objects=max_objects, max_rings=max_rings or lab.size,
                   max_vertices=max_vertices or 4 * lab.size)
    return o["rings"], o["vertices"], o["counts"]


SEEDS, LABELLINGS = C.SEEDS, C.LABELLINGS
GPU_SEEDS = tuple(range(8))


@functools.lru_cache(maxsize=None)
def survey_case(seed, labelling, connectivity):
    mask = K.survey_mask(seed)
    if labelling == "components":
        obj = O.objects(mask, connectivity=connectivity, max_objects=K.SIZE * K.SIZE)
    else:
        obj = SP.split(mask, C.SPLIT_R2, connectivity=connectivity, max_objects=K.SIZE * K.SIZE)
    return dict(labels=np.asarray(obj["labels"], dtype=np.int32), counts_obj=np.asarray(obj["counts"], dtype=np.int32)[:2].copy(),
                connectivity=connectivity)


def comb_labels(sizes):
    """Combs under each other, one object each: t teeth of one pixel, two apart, hanging from a bar, which makes 4 t corners.
    One-pixel neighbours of other ids bring the augmented ring of comb j to sizes[j] vertices: one left of the bar inserts one
    straight-through node into the comb's left wall, one on top of the bar inserts two into its upper wall."""
    teeth = [(n - 1) // 4 for n in sizes]
    assert min(teeth) >= 3
    lab = np.zeros((4 * len(sizes) + 2, 2 * max(teeth) + 3), dtype=np.int32)
    nxt = len(sizes) + 1
    for j, (n, t) in enumerate(zip(sizes, teeth)):
        y, extra = 4 * j + 2, n - 4 * t                  # extra in 1 .. 4
        lab[y, 2:2 * t + 1] = j + 1
        lab[y + 1, 2:2 * t + 1:2] = j + 1
        spots = {1: [(y, 1)], 2: [(y - 1, 3)], 3: [(y, 1), (y - 1, 3)], 4: [(y - 1, 3), (y - 1, 5)]}[extra]
        for yy, xx in spots:
            lab[yy, xx] = nxt
            nxt += 1
    return dict(labels=lab, counts_obj=np.array([nxt - 1, nxt - 1], dtype=np.int32), connectivity=4)
