"""Inputs shared by tests/test_safe_cpu.py, tests/test_safe_gpu.py and tests/test_safe_infer_gpu.py: the hand-made label maps,
survey masks and combs of tests/shared_cases.py, the expected survey table of the issue that introduced the call, and label maps
made for the detector's tiers."""
import functools

import numpy as np

import safe_reference as S
import shared_cases as SC
import valid_cases as K

HAND_MADE, TOLERANCES_HAND = SC.hand_made, SC.TOLERANCES_HAND
SEEDS, GPU_SEEDS, LABELLINGS = SC.SEEDS, SC.GPU_SEEDS, SC.LABELLINGS
TOLERANCES = (1.0, 1.5, 2.0)
MAX_OBJECTS = K.SIZE * K.SIZE

# (labelling, connectivity, tol): (objects with a defect in round 0, at the end, vertices in round 0, at the end,
# {raising rounds: scenes}, arcs refined, arcs) over the 40 survey masks, from the prototype of the loop
SURVEY_TABLE = {
    ("components", 4, 1.0): (180, 0, 6333, 7054, {0: 1, 1: 27, 2: 12}, 559, 3559),
    ("components", 4, 1.5): (184, 0, 5974, 6517, {0: 1, 1: 7, 2: 27, 3: 5}, 577, 3559),
    ("components", 4, 2.0): (215, 0, 5504, 6353, {1: 1, 2: 19, 3: 10, 4: 9, 5: 1}, 732, 3559),
    ("components", 8, 1.0): (43, 0, 6333, 7441, {1: 20, 2: 20}, 905, 3559),
    ("components", 8, 1.5): (43, 0, 5974, 6792, {1: 4, 2: 27, 3: 9}, 920, 3559),
    ("components", 8, 2.0): (45, 0, 5504, 6779, {2: 11, 3: 11, 4: 18}, 1142, 3559),
    ("split", 4, 1.0): (159, 0, 8108, 8485, {0: 3, 1: 31, 2: 6}, 308, 6334),
    ("split", 4, 1.5): (169, 0, 7750, 8025, {0: 3, 1: 20, 2: 14, 3: 3}, 317, 6334),
    ("split", 4, 2.0): (217, 0, 7367, 7810, {0: 2, 1: 1, 2: 27, 3: 5, 4: 3, 5: 2}, 429, 6334),
    ("split", 8, 1.0): (196, 0, 8947, 9704, {0: 1, 1: 20, 2: 19}, 647, 7172),
    ("split", 8, 1.5): (198, 0, 8598, 9126, {0: 1, 1: 7, 2: 23, 3: 9}, 652, 7172),
    ("split", 8, 2.0): (226, 0, 8240, 9077, {0: 1, 2: 12, 3: 10, 4: 17}, 783, 7172),
}


@functools.lru_cache(maxsize=None)
def survey_prep(seed, labelling, connectivity):
    """(case, table, what `safe_reference.prepare` makes of them) of one survey mask."""
    c = SC.survey_case(seed, labelling, connectivity)
    table = SC.table(c)
    return c, table, S.prepare(c["labels"], c["counts_obj"], *table, max_objects=MAX_OBJECTS)


@functools.lru_cache(maxsize=None)
def survey_run(seed, labelling, connectivity, tol, max_rounds=8):
    """(result, history) of the restatement on one survey mask, pairs counted in numpy."""
    c, table, prep = survey_prep(seed, labelling, connectivity)
    history = []
    out = S.simplify_safe(c["labels"], c["counts_obj"], *table, S.R.tol2_q(tol), max_rounds=max_rounds, max_objects=MAX_OBJECTS, fast=True,
                          history=history, prep=prep)
    return out, history


def owners(out, marks):
    """The ids that own an edge of a marked arc."""
    return {int(out["rings"][r, 0]) for r, slot in out["slots"].items() if any(s in marks for s in slot)}


DEEP_SCENE = (3, "components", 4)                            # five raising rounds at 2 px


def nested_ls(t, patch=None):
    """t L-shaped objects one pixel wide, nested two apart.  All their walls are long, so no grid within the budget separates
    them and a few cells hold most edges.  `patch` = a survey seed puts that mask, labelled as 4-connected components, into the
    corner that the innermost L leaves free: its defects then lie in a crowded cell."""
    size = 2 * t + 2 + (K.SIZE + 1 if patch is not None else 0)
    lab = np.zeros((size, size), dtype=np.int32)
    for j in range(t):
        lab[2 * j + 1, 2 * j + 1:size - 1] = j + 1
        lab[2 * j + 1:size - 1, 2 * j + 1] = j + 1
    top = t
    if patch is not None:
        inner = SC.survey_case(patch, "components", 4)["labels"]
        lab[2 * t + 2:2 * t + 2 + K.SIZE, 2 * t + 2:2 * t + 2 + K.SIZE] = np.where(inner > 0, inner + t, 0)
        top = int(lab.max())
    return dict(labels=lab, counts_obj=np.array([top, top], dtype=np.int32), connectivity=4)
