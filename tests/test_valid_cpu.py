"""The restatement of `c3d_rings_valid` (tests/valid_reference.py) against witnesses that share nothing with it: the
intersection of two segments as exact fractions, star polygons whose crossings are known in closed form, one table per pair
class counted by hand, and the survey of noisy masks that the README quotes.  No GPU."""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import valid_cases as K  # noqa: E402
import valid_reference as V  # noqa: E402

HAND_MADE = K.hand_made()
TOLERANCES = (1.0, 1.5, 2.0)


def witness(a, b, c, d):
    """The class of two live segments from the points they share, in exact fractions: the parameters (s, t) of the one
    common point of two lines that are not parallel, or the common stretch of two that are collinear."""
    ex, ey, fx, fy = b[0] - a[0], b[1] - a[1], d[0] - c[0], d[1] - c[1]
    den = ex * fy - ey * fx
    wx, wy = c[0] - a[0], c[1] - a[1]
    if den != 0:
        s, t = Fraction(wx * fy - wy * fx, den), Fraction(wx * ey - wy * ex, den)   # a + s e == c + t f
        if not (0 <= s <= 1 and 0 <= t <= 1):
            return None
        if 0 < s < 1 and 0 < t < 1:
            return V.CROSS
        return V.VV if s in (0, 1) and t in (0, 1) else V.VE
    if wx * ey - wy * ex != 0:
        return None                                          # parallel, apart
    L = ex * ex + ey * ey
    s0, s1 = sorted((Fraction(wx * ex + wy * ey, L), Fraction((d[0] - a[0]) * ex + (d[1] - a[1]) * ey, L)))
    lo, hi = max(s0, 0), min(s1, 1)
    return V.OVERLAP if lo < hi else (V.VV if lo == hi else None)


def test_the_predicate_against_exact_fractions_on_every_pair_of_a_small_lattice():
    pts = [(x, y) for x in range(4) for y in range(3)]
    segs = [(a, b) for a, b in itertools.permutations(pts, 2)]
    seen = {}
    for (a, b), (c, d) in itertools.combinations(segs, 2):
        got, want = V.classify(a, b, c, d), witness(a, b, c, d)
        assert got == want, (a, b, c, d, got, want)
        seen[got] = seen.get(got, 0) + 1
    assert all(seen.get(k, 0) > 50 for k in (None, V.CROSS, V.OVERLAP, V.VV, V.VE)), seen


def test_the_predicate_at_the_corners_of_the_coordinate_range():
    c = 32768 << 8
    rng = np.random.default_rng(5)
    corners = [(-c, -c), (c, c), (c, -c), (-c, c), (0, 0), (c - 1, c), (-c, 1 - c), (1, 0), (c, 0), (0, -c)]
    for _ in range(400):
        a, b, p, q = (corners[k] for k in rng.integers(0, len(corners), 4))
        if a != b and p != q:
            assert V.classify(a, b, p, q) == witness(a, b, p, q), (a, b, p, q)


@pytest.mark.parametrize("n,k", [(5, 2), (7, 3), (64, 5), (257, 3)])
def test_star_polygons_cross_n_times_k_minus_one(n, k):
    m, degenerate, got = V.count_pairs([K.star(n, k)])
    assert (m, degenerate) == (n, 0)
    assert got == {V.CROSS: n * (k - 1), V.OVERLAP: 0, V.VV: 0, V.VE: 0}


@pytest.mark.parametrize("name", [n for n, c in HAND_MADE.items() if c["want"] is not None])
def test_hand_made_cases(name):
    c = HAND_MADE[name]
    out = V.valid(K.tables(c), c["frac_bits"], c["max_ids"])
    assert tuple(out["valid"][0, 4:]) == c["want"], out["valid"][0]
    assert out["valid"][0, 0] == 0
    if name == "degenerate":
        assert out["valid"][0, 1:4].tolist() == [1, 4, 1]
    if name == "interleaved":
        assert out["valid"][:3].tolist() == [[0, 3, 12, 0, 2, 0, 0, 0], [0, 2, 8, 0, 1, 0, 0, 0], [0, 1, 4, 0, 0, 0, 0, 0]]
        assert out["counts"].tolist() == [3, 2, 0, 0, 0, 3, 0, 0]
    if name == "flags":
        assert out["valid"][:, 0].tolist() == [0, 1, 0, 1, 1, 0, 0, 0] and out["valid"][3, 1:4].tolist() == [1, 0, 3]
        assert out["counts"].tolist() == [3, 0, 3, 0, 0, 0, 0, 0]


def test_the_corners_of_the_range_cross_once():
    for f in (0, 4, 8):
        c = HAND_MADE[f"frac_{f}"]
        out = V.valid(K.tables(c), f, c["max_ids"])
        assert out["valid"][0, 0] == 0 and out["valid"][0, 4] >= 1
        too_narrow = V.valid(K.tables(c), f - 1, c["max_ids"]) if f else None
        assert too_narrow is None or too_narrow["valid"][0, 0] == 2


def test_the_work_cap_and_the_negative_controls_change_named_cases():
    c = HAND_MADE["bow_tie"]
    assert V.valid(K.tables(c), 0, c["max_ids"], max_id_work=6)["valid"][0, 0] == 0
    assert V.valid(K.tables(c), 0, c["max_ids"], max_id_work=5)["valid"][0].tolist() == [3, 1, 4, 0, 0, 0, 0, 0]
    assert V.count_pairs(HAND_MADE["corner_shared"]["rings"], strict=False)[2][V.CROSS] > 0
    assert V.count_pairs(HAND_MADE["spike"]["rings"], adjacent_overlap=False)[2][V.OVERLAP] == 0
    assert V.count_pairs(HAND_MADE["corner_shared"]["rings"], ring_adjacency=False)[2][V.VV] == 6   # the closing joints count


def test_the_survey_of_noisy_masks(capsys):
    """Raw traced rings never cross, overlap or touch inside an edge; simplified ones do.  The numbers printed are the ones the
    README quotes: a measurement, not a threshold."""
    objects, raw = 0, {V.CROSS: 0, V.OVERLAP: 0, V.VV: 0, V.VE: 0}
    invalid = {tol: 0 for tol in TOLERANCES}
    smallest = None
    for seed in K.SEEDS:
        for connectivity in (4, 8):
            for i, rings in K.traced(seed, connectivity).items():
                objects += 1
                got = V.count_pairs(rings)[2]
                for what in raw:
                    raw[what] += got[what]
                for tol in TOLERANCES:
                    got = V.count_pairs(K.simplified(rings, tol))[2]
                    if got[V.CROSS] or got[V.OVERLAP]:
                        invalid[tol] += 1
                        n = sum(len(r) for r in rings)
                        smallest = n if smallest is None else min(smallest, n)
    with capsys.disabled():
        print(f"\nvalidity survey: {objects} objects; raw {raw}; invalid after simplification "
              f"{ {tol: n for tol, n in invalid.items()} }, {sum(invalid.values())} (object, tolerance) cases, the smallest id "
              f"of {smallest} raw vertices")
    assert objects > 500
    assert raw[V.CROSS] == 0 and raw[V.OVERLAP] == 0 and raw[V.VE] == 0 and raw[V.VV] > 0
    assert invalid[1.0] > 0


def test_two_rows_of_the_survey():
    got = V.count_pairs(K.simplified(K.traced(4, 4)[30], 1.0))[2]
    assert got[V.OVERLAP] == 1 and got[V.VE] == 1 and got[V.CROSS] == 0, got
    got = V.count_pairs(K.simplified(K.traced(27, 8)[2], 2.0))[2]
    assert got[V.CROSS] == 2 and got[V.OVERLAP] == 0, got
