"""The restatement of `c3d_rings_conflicts` (tests/conflicts_reference.py) against witnesses that share nothing with it: the
intersection of two segments as exact fractions, two concentric stars of different ids whose crossings are counted by hand, one
table per class counted by hand; then the property that raw traced rings never conflict, the survey that the README quotes,
and the fall-back loop on the restatements.  No GPU."""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflicts_cases as C  # noqa: E402
import conflicts_reference as R  # noqa: E402
import valid_cases as K  # noqa: E402

HAND_MADE = C.hand_made()
NAMES = (R.CROSS, R.SAME, R.OPPOSITE, R.VV, R.VE)


def witness(a, b, c, d):
    """The class of two live segments of different ids from the points they share, in exact fractions."""
    ex, ey, fx, fy = b[0] - a[0], b[1] - a[1], d[0] - c[0], d[1] - c[1]
    den = ex * fy - ey * fx
    wx, wy = c[0] - a[0], c[1] - a[1]
    if den != 0:
        s, t = Fraction(wx * fy - wy * fx, den), Fraction(wx * ey - wy * ex, den)   # a + s e == c + t f
        if not (0 <= s <= 1 and 0 <= t <= 1):
            return None
        if 0 < s < 1 and 0 < t < 1:
            return R.CROSS
        return R.VV if s in (0, 1) and t in (0, 1) else R.VE
    if wx * ey - wy * ex != 0:
        return None                                          # parallel, apart
    L = ex * ex + ey * ey
    s_c, s_d = Fraction(wx * ex + wy * ey, L), Fraction((d[0] - a[0]) * ex + (d[1] - a[1]) * ey, L)
    lo, hi = max(min(s_c, s_d), 0), min(max(s_c, s_d), 1)
    if lo < hi:
        return R.SAME if s_d > s_c else R.OPPOSITE           # d lies further along (a, b) than c: the same way
    return R.VV if lo == hi else None


def test_the_predicate_against_exact_fractions_on_every_pair_of_a_small_lattice():
    pts = [(x, y) for x in range(4) for y in range(3)]
    segs = list(itertools.permutations(pts, 2))
    seen = {}
    for (a, b), (c, d) in itertools.combinations(segs, 2):
        got, want = R.pair_class(a, b, c, d), witness(a, b, c, d)
        assert got == want, (a, b, c, d, got, want)
        seen[got] = seen.get(got, 0) + 1
    assert all(seen.get(k, 0) > 50 for k in (None,) + NAMES), seen


def test_the_predicate_at_the_corners_of_the_coordinate_range():
    c = 32768 << 8
    rng = np.random.default_rng(5)
    corners = [(-c, -c), (c, c), (c, -c), (-c, c), (0, 0), (c - 1, c), (-c, 1 - c), (1, 0), (c, 0), (0, -c)]
    for _ in range(400):
        a, b, p, q = (corners[k] for k in rng.integers(0, len(corners), 4))
        if a != b and p != q:
            assert R.pair_class(a, b, p, q) == witness(a, b, p, q), (a, b, p, q)


@pytest.mark.parametrize("n,k", [(5, 2), (7, 3), (9, 2)])
def test_two_concentric_stars_of_different_ids(n, k):
    """{n/k} on the radius 30000 as id 1 and a star of the same kind on the radius 29000, turned by half a step, as id 2.  The 2 n
    points are in convex position and alternate round the circle.  A chord of id 1 skips k - 1 vertices of its own star, so k
    vertices of id 2 lie strictly on its short side; each is the end of two chords of id 2, and no chord of id 2 has both ends
    among k neighbours, so 2 k chords of id 2 cross it: 2 n k crossings, every pair once (20 for the two pentagrams).  The
    witness counts the same edge by edge."""
    import math
    one = K.star(n, k, radius=30000)
    turn = math.pi / n
    two = [(int(round(29000 * math.cos(2 * math.pi * ((i * k) % n) / n + turn))), int(round(29000 * math.sin(2 * math.pi * ((i * k) % n) / n + turn))))
           for i in range(n)]
    c = C.case([one, two], ids=[1, 2])
    out = R.conflicts(C.tables(c), 0, c["max_ids"])
    by_witness = sum(witness(one[i], one[(i + 1) % n], two[j], two[(j + 1) % n]) == R.CROSS for i in range(n) for j in range(n))
    assert out["counts"][5] == by_witness and out["conflict"][0, 3] == by_witness and out["conflict"][1, 3] == by_witness
    assert out["conflict"][0, 1] == 2 and out["conflict"][1, 1] == 1 and out["counts"][:2].tolist() == [2, 2]
    assert by_witness == 2 * n * k
    # the stars cross themselves as well: nothing of that is counted
    assert out["conflict"][:2, 4:].sum() == 0


@pytest.mark.parametrize("name", [n for n, c in HAND_MADE.items() if c["want"] is not None])
def test_hand_made_cases(name):
    c = HAND_MADE[name]
    out = R.conflicts(C.tables(c), c["frac_bits"], c["max_ids"])
    for i, want in c["want"].items():
        assert tuple(out["conflict"][i - 1, 3:]) == want, (i, out["conflict"][i - 1])
        assert out["conflict"][i - 1, 0] == 0
    if name == "two_neighbours":
        assert out["conflict"][:3, 1].tolist() == [3, 3, 1] and out["counts"].tolist() == [3, 3, 0, 0, 0, 4, 0, 0]
    if name == "opposite":
        assert out["counts"][:2].tolist() == [2, 0] and out["info"].tolist() == [8, 0, 0, 0, 0, 0, 1, 6]
    if name == "same":
        assert out["counts"].tolist() == [2, 2, 0, 0, 0, 0, 1, 0] and out["conflict"][:2, 1].tolist() == [2, 1]
    if name == "bow_tie_alone":
        assert out["conflict"][0].tolist() == [0, 0, 4, 0, 0, 0, 0, 0]


def test_the_corners_of_the_range_cross():
    for f in (0, 4, 8):
        c = HAND_MADE[f"frac_{f}"]
        out = R.conflicts(C.tables(c), f, c["max_ids"])
        assert out["conflict"][0, 0] == 0 and out["conflict"][0, 3] >= 1
        too_narrow = R.conflicts(C.tables(c), f - 1, c["max_ids"]) if f else None
        assert too_narrow is None or too_narrow["conflict"][:3, 0].tolist() == [2, 2, 2]


def test_the_edges_of_an_incomplete_id_take_part_in_nothing():
    c = HAND_MADE["cross"]
    table = C.tables(c)
    table[0][1, 1] = -1                                      # id 2: a row with start < 0
    out = R.conflicts(table, 0, c["max_ids"])
    assert out["conflict"][:2].tolist() == [[0, 0, 4, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0]]
    assert out["counts"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]


def test_the_negative_controls_change_named_cases():
    for name, wrong in (("bow_tie_alone", dict(same_id=True)), ("opposite", dict(direction=False)), ("touch_vv", dict(strict=False))):
        c = HAND_MADE[name]
        good, bad = R.conflicts(C.tables(c), 0, c["max_ids"]), R.conflicts(C.tables(c), 0, c["max_ids"], **wrong)
        assert good["counts"][1] == 0 and bad["counts"][1] > 0, name


def test_the_survey_tool_agrees_with_the_restatement():
    for seed, labelling, connectivity, tol in ((2, "split", 8, 1.0), (5, "components", 4, 2.0), (37, "split", 4, None)):
        geo = C.scene(seed, labelling, connectivity) if tol is None else C.simplified_scene(seed, labelling, connectivity, tol)
        rows, sums = C.fast_counts(geo)
        c = C.scene_case(geo)
        out = R.conflicts(C.tables(c), 0, c["max_ids"])
        for i, want in rows.items():
            assert tuple(out["conflict"][i - 1, 3:]) == want, (seed, i)
        assert (out["counts"][5], out["counts"][6], out["info"][6], out["info"][7]) == (sums[0], sums[1], sums[2], sums[3] + sums[4])
        assert out["counts"][1] == len(C.in_conflict(rows))


def test_the_survey_of_noisy_masks_and_the_fall_back_loop(capsys):
    """Raw traced rings never conflict, whether components or split pieces; the pieces share walls.  Simplified ones conflict,
    the pieces in nearly every scene.  Falling back to the raw vertices is not a repair in one pass, and always ends clean.  The
    numbers printed are the ones the README quotes: measurements, not thresholds."""
    lines = []
    for labelling, connectivity in C.LABELLINGS:
        objects, raw = 0, [0] * 5
        hit = {tol: [0, 0] for tol in C.TOLERANCES}
        rounds = {}
        for seed in C.SEEDS:
            geo = C.scene(seed, labelling, connectivity)
            objects += len(geo)
            raw = [x + y for x, y in zip(raw, C.fast_counts(geo)[1])]
            for tol in C.TOLERANCES:
                n = len(C.in_conflict(C.fast_counts(C.simplified_scene(seed, labelling, connectivity, tol))[0]))
                hit[tol][0] += n
                hit[tol][1] += n > 0
            if labelling == "split":
                r, mixed = C.fall_back(geo, C.simplified_scene(seed, labelling, connectivity, 1.0))
                rounds[r] = rounds.get(r, 0) + 1
                assert not C.in_conflict(C.fast_counts(mixed)[0]), "the loop ends clean"
        assert raw[0] == 0 and raw[1] == 0, "raw traced rings never cross and never overlap the same way"
        if labelling == "split":
            assert raw[2] > 0 and hit[1.0][0] > 0 and max(rounds) >= 2
        lines.append(f"  {labelling} {connectivity}-conn: {objects} objects; raw {dict(zip(NAMES, raw))}; in conflict (objects, scenes of "
                     f"{len(C.SEEDS)}) " + ", ".join(f"{tol} px {n} in {s}" for tol, (n, s) in hit.items())
                     + (f"; rounds of the fall-back loop at 1 px {dict(sorted(rounds.items()))}" if rounds else ""))
    with capsys.disabled():
        print("\nconflict survey:\n" + "\n".join(lines))


def test_the_grid_rule_on_named_cases():
    limits = (64, 256, 256, 16384, 2, 4)
    c = HAND_MADE["diagonals"]
    g = C.grid(C.tables(c), 0, c["max_ids"], limits)
    assert g["cells_x"] * g["cells_y"] > 1 and g["entries"] <= 2 * 246, "246 live edges"
    for t in (21, 22, 257):                                  # no grid within the budget separates the inscribed triangles
        c = C.crowded(t)
        g = C.grid(C.tables(c), 0, c["max_ids"], limits)
        assert (g["cells_x"], g["cells_y"], g["entries"], g["work"]) == (1, 1, 3 * t, 3 * t * (3 * t - 1) // 2)
