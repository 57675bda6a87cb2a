"""The rule of c3d_outlines_simplify_shared on the restatement alone (tests/shared_reference.py): the twin property over the
whole survey, the round trip at tolerance 0, the tolerance bound in exact rationals, the two negative controls, and the survey
table of objects in conflict beside the plain simplifier's."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import conflicts_cases as C
import fill_reference as F
import shared_cases as SC
import shared_reference as R
import valid_cases as K

TOLERANCES = (0.0, 1.0, 1.5, 2.0)


@functools.lru_cache(maxsize=None)
def survey(seed, labelling, connectivity, tol, tie="position", insert_nodes=True):
    c = SC.survey_case(seed, labelling, connectivity)
    return R.simplify_shared(c["labels"], c["counts_obj"], *SC.table(c), R.tol2_q(tol), max_objects=K.SIZE * K.SIZE, tie=tie,
                             insert_nodes=insert_nodes)


def run(c, tol, **kw):
    return R.simplify_shared(c["labels"], c["counts_obj"], *SC.table(c), R.tol2_q(tol), **kw)


def test_the_array_distance_is_the_scalar_one():
    rng = np.random.default_rng(5)
    for _ in range(500):
        a = tuple(int(v) for v in rng.integers(0, 12, 2))
        b = a if rng.random() < 0.2 else tuple(int(v) for v in rng.integers(0, 12, 2))
        pts = rng.integers(0, 12, (6, 2)).astype(np.int64)
        nums, den = R.distances(a, b, pts[:, 0], pts[:, 1])
        assert [(int(n), den) for n in nums] == [R.distance(a, b, tuple(p)) for p in pts.tolist()]
    far = 16384                                              # the largest products: 2^28 squared, times nothing more
    nums, den = R.distances((0, 0), (far, far), np.array([far, 0], dtype=np.int64), np.array([0, far], dtype=np.int64))
    assert [(int(n), den) for n in nums] == [R.distance((0, 0), (far, far), p) for p in ((far, 0), (0, far))]


def test_twin_property_over_the_survey():
    failures = checked = 0
    for seed in SC.SEEDS:
        for labelling, conn in SC.LABELLINGS:
            for tol in TOLERANCES:
                out = survey(seed, labelling, conn, tol)
                assert int(out["counts"][4]) == 0
                failures += len(R.twin_failures(out))
                checked += int((out["left"][:int(out["counts"][3])] > 0).sum())
    print(f"twin property: {checked} shared edges, {failures} failures")
    assert checked > 0 and failures == 0


@pytest.mark.parametrize("name", sorted(SC.hand_made()))
def test_twin_property_hand_made(name):
    for tol in SC.TOLERANCES_HAND:
        assert R.twin_failures(run(SC.hand_made()[name], tol)) == []


def cases_tol0():
    out = [(name, c) for name, c in sorted(SC.hand_made().items())]
    out += [(f"{lab}{conn}_{seed}", SC.survey_case(seed, lab, conn)) for seed in range(0, 40, 5) for lab, conn in SC.LABELLINGS]
    return out


def test_tolerance_zero_fills_back_to_the_labels():
    for name, c in cases_tol0():
        out = run(c, 0.0)
        lab = c["labels"]
        assert int(out["info"][5]) == 0, name
        got = F.fill(out["rings"], out["vertices"], out["counts"], *lab.shape, max_objects=int(lab.max()) + 1)
        assert np.array_equal(got["labels"], lab), name


def test_tolerance_zero_is_the_augmented_ring():
    c = SC.hand_made()["t_junction"]
    out = run(c, 0.0)
    geo, _ = R.geometry(out)
    assert (4, 3) in geo[3][0] and int(out["info"][0]) == 1   # the end of the wall between 1 and 2, inside the upper wall of 3
    rings, vertices, counts = SC.table(c)
    assert int(out["counts"][3]) == int(counts[3]) + 1


def test_dropped_vertices_lie_within_the_tolerance():
    checked = 0
    for seed in range(0, 40, 4):
        for labelling, conn in SC.LABELLINGS:
            for tol in (1.0, 1.5, 2.0):
                q = R.tol2_q(tol)
                c = SC.survey_case(seed, labelling, conn)
                lab = R.Labels(c["labels"], c["counts_obj"], K.SIZE * K.SIZE)
                rings, vertices, _ = SC.table(c)
                for _, start, n, *_ in rings[:int(SC.table(c)[2][1])].tolist():
                    aug = R.rotate(R.augment([tuple(p) for p in vertices[start:start + n].tolist()], lab))
                    ring = [(a[0], a[1]) for a in aug]
                    at = R.simplify_ring(aug, q)
                    for a, b in zip(at, at[1:] + [at[0] + len(ring)]):
                        for k in range(a + 1, b):
                            num, den = R.distance(ring[a], ring[b % len(ring)], ring[k % len(ring)])
                            assert Fraction(num, den) <= Fraction(q, 16)
                            checked += 1
    assert checked > 1000


def test_negative_control_tie_by_index():
    """Two pieces along a staircase whose steps tie: with the ring's own index the two directions choose different steps."""
    c = SC.hand_made()["stairs"]
    assert R.twin_failures(run(c, 0.5)) == []
    assert R.twin_failures(run(c, 0.5, tie="index")) != []


def test_negative_control_no_inserted_nodes():
    c = SC.hand_made()["t_junction"]
    assert R.twin_failures(run(c, 0.0)) == []
    assert R.twin_failures(run(c, 0.0, insert_nodes=False)) != []


def test_closed_arc_guard_keeps_the_area():
    c = SC.hand_made()["island"]
    for tol in (2.0, 8.0, 100.0):
        out = run(c, tol)
        assert int(out["info"][5]) == 0 and (out["rings"][:int(out["counts"][1]), 2] >= 3).all()
        assert (out["rings"][:int(out["counts"][1]), 3] != 0).all()


def test_island_and_hole_are_each_others_reverse():
    c = SC.hand_made()["island"]
    for tol in SC.TOLERANCES_HAND:
        geo, _ = R.geometry(run(c, tol))
        hole = [r for r in geo[1] if R.shoelace2(r) < 0][0]
        island = geo[2][0]
        assert hole[0] == island[0] and hole[1:] == island[1:][::-1]


def test_a_piece_between_two_nodes_collapses():
    out = run(SC.hand_made()["collapse"], 2.0)
    assert int(out["info"][5]) >= 1 and R.twin_failures(out) == []


def test_truncation_and_bad_rows():
    c = SC.hand_made()["four_at_a_point"]
    full = run(c, 1.0)
    need = int(full["counts"][3])
    cut = run(c, 1.0, max_vertices_out=need - 1)
    assert int(cut["counts"][2]) == need and int(cut["counts"][3]) < need and int(cut["counts"][4]) & R.ST_TRUNCATED
    assert int(cut["rings"][int(cut["counts"][1]) - 1, 1]) == -1
    rings, vertices, counts = SC.table(c)
    vertices = vertices.copy()
    vertices[int(rings[1, 1]) + 1] += (1, 1)             # an edge that is not parallel to an axis
    rings = rings.copy()
    rings[2, 1] = -1
    out = R.simplify_shared(c["labels"], c["counts_obj"], rings, vertices, counts, 16)
    assert int(out["counts"][4]) == R.ST_BAD_INPUT and out["rings"][1, 1] == -1 and out["rings"][2, 1] == -1 and out["rings"][0, 1] == 0


def conflict_table():
    rows = {}
    for labelling, conn in C.LABELLINGS:
        for tol in C.TOLERANCES:
            plain = shared = objects = 0
            for seed in C.SEEDS:
                geo_p = C.simplified_scene(seed, labelling, conn, tol)
                geo_s, _ = R.geometry(survey(seed, labelling, conn, tol))
                assert sorted(geo_s) == sorted(geo_p)
                objects += len(geo_p)
                plain += len(C.in_conflict(C.fast_counts(geo_p)[0]))
                shared += len(C.in_conflict(C.fast_counts(geo_s)[0]))
            rows[(labelling, conn, tol)] = (objects, plain, shared)
    return rows


def test_fewer_objects_in_conflict_than_the_plain_simplifier():
    rows = conflict_table()
    print("objects in conflict, plain simplifier -> shared rule")
    for (labelling, conn, tol), (objects, plain, shared) in rows.items():
        print(f"  {labelling} {conn}-conn ({objects} objects) {tol:g} px: {plain} -> {shared}")
    for (labelling, conn, tol), (objects, plain, shared) in rows.items():
        if labelling == "split":
            assert shared < plain, (labelling, conn, tol, plain, shared)
        else:
            assert shared <= plain, (labelling, conn, tol, plain, shared)


def test_vertex_totals():
    n0_raw = n0 = n1 = n1_plain = 0
    for seed in C.SEEDS:
        c = SC.survey_case(seed, "split", 4)
        n0_raw += int(SC.table(c)[2][3])
        n0 += int(survey(seed, "split", 4, 0.0)["counts"][3])
        n1 += int(survey(seed, "split", 4, 1.0)["counts"][3])
        n1_plain += sum(len(r) for rings in C.simplified_scene(seed, "split", 4, 1.0).values() for r in rings)
    print(f"split 4-conn: raw {n0_raw} -> augmented {n0}; at 1 px plain keeps {n1_plain}, shared keeps {n1}")
    assert n0 >= n0_raw and n1 <= n0
