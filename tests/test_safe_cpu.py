"""The rule of c3d_outlines_simplify_safe on the restatement alone (tests/safe_reference.py): the plain pair count against the
numpy one, the termination argument (all arcs raw: no defect) on every survey scene, the twin property after every round, equal
keys for twins and for an island and its hole, what follows from the rule (tolerance 0, a clean round 0), and the survey table of
the loop, printed and held against the figures of the prototype."""
import numpy as np
import pytest

import safe_cases as SA
import safe_reference as S
import shared_cases as SC
import shared_reference as R


def run(c, tol, **kw):
    return S.simplify_safe(c["labels"], c["counts_obj"], *SC.table(c), R.tol2_q(tol), **kw)


def test_level_cap():
    assert [S.level_cap(q) for q in (0, 1, 3, 4, 15, 16, 64, R.TOL2_Q_MAX)] == [0, 1, 1, 2, 2, 3, 4, 13]


def test_plain_pairs_equal_the_numpy_count():
    checked = 0
    for name, c in sorted(SA.HAND_MADE().items()):
        for tol in SA.TOLERANCES_HAND:
            history = []
            run(c, tol, history=history)
            for out, marks, pairs, bad_rows in history:
                edges = S.edges_of(out)
                for ve in (True, False):
                    assert S.detect(edges, ve) == S.detect_numpy(edges, ve), (name, tol)
                checked += pairs
    for seed in SA.SEEDS[::8]:
        for labelling, conn in SA.LABELLINGS:
            _, history = SA.survey_run(seed, labelling, conn, 2.0)
            for out, marks, pairs, bad_rows in history:
                edges = S.edges_of(out)
                plain, n = S.detect(edges)
                for r in bad_rows:
                    plain.update(out["slots"][r])
                assert (plain, n) == (marks, pairs), (seed, labelling, conn)
                checked += pairs
    assert checked > 100


def test_raw_arcs_have_no_defect_on_every_survey_scene():
    """The termination argument: with every level at L_cap the output is the raw augmented ring and nothing is marked."""
    for tol in (1.0, 2.0):
        q = R.tol2_q(tol)
        cap = S.level_cap(q)
        for seed in SA.SEEDS:
            for labelling, conn in SA.LABELLINGS:
                c, table, prep = SA.survey_prep(seed, labelling, conn)
                start = {key: cap for ring in prep["rows"] if ring for _, _, key in ring["arcs"]}
                out = S.simplify_safe(c["labels"], c["counts_obj"], *table, q, max_rounds=1, fast=True, start_levels=start, prep=prep)
                raw = R.simplify_shared(c["labels"], c["counts_obj"], *table, 0, max_objects=SA.MAX_OBJECTS)
                assert out["safe"].tolist()[4:] == [0, 0, 0, S.ST_CONVERGED], (seed, labelling, conn)
                assert all(np.array_equal(out[n], raw[n]) for n in ("rings", "vertices", "left", "counts"))


def test_twin_property_after_every_round():
    rounds = 0
    for seed in SA.SEEDS:
        for labelling, conn in SA.LABELLINGS:
            out, history = SA.survey_run(seed, labelling, conn, 2.0)
            for step, _, _, _ in history:
                assert R.twin_failures(step) == [], (seed, labelling, conn)
                rounds += 1
            assert R.twin_failures(out) == []
    for name, c in sorted(SA.HAND_MADE().items()):
        for tol in SA.TOLERANCES_HAND:
            history = []
            run(c, tol, history=history)
            assert all(R.twin_failures(step) == [] for step, _, _, _ in history), name
    assert rounds > 4 * len(SA.SEEDS)


def _arcs_by_edge(out):
    """{(p, q, id): slot} of every output edge."""
    found = {}
    V_ = out["vertices"].tolist()
    for r, slot in out["slots"].items():
        rid, start, n = (int(v) for v in out["rings"][r, :3])
        for k in range(n):
            found[(tuple(V_[start + k]), tuple(V_[start + (k + 1) % n]), rid)] = slot[k]
    return found


def test_twins_and_islands_share_their_key():
    shared = 0
    cases = list(sorted(SA.HAND_MADE().items())) + [((seed, lab, conn), SA.survey_prep(seed, lab, conn)[0]) for seed in SA.SEEDS[::5]
                                                    for lab, conn in SA.LABELLINGS]
    for name, c in cases:
        out = run(c, 0.0, max_rounds=1, fast=True, max_objects=SA.MAX_OBJECTS)   # raw edges: a reversed edge is the twin's
        by_edge = _arcs_by_edge(out)
        for (p, q, rid), slot in by_edge.items():
            twins = [s for (p2, q2, other), s in by_edge.items() if (p2, q2) == (q, p) and other != rid]
            assert all(s == slot for s in twins), name
            shared += len(twins)
    assert shared > 1000
    out = run(SA.HAND_MADE()["island"], 0.0)
    geo, _ = R.geometry(out)
    hole = [r for r, slot in out["slots"].items() if int(out["rings"][r, 0]) == 1 and int(out["rings"][r, 3]) < 0][0]
    island = [r for r in out["slots"] if int(out["rings"][r, 0]) == 2][0]
    assert set(out["slots"][hole]) == set(out["slots"][island]) and len(set(out["slots"][island])) == 1


def test_distinct_arcs_have_distinct_keys():
    for seed in SA.SEEDS[::5]:
        for labelling, conn in SA.LABELLINGS:
            _, _, prep = SA.survey_prep(seed, labelling, conn)
            seen = {}
            for r, ring in enumerate(prep["rows"]):
                for i, j, key in ring["arcs"] if ring else ():
                    seen.setdefault(key, []).append(frozenset(map(frozenset, zip(ring["pts"][i:j], ring["pts"][i + 1:j + 1]))))
            assert all(len(v) <= 2 and len(set(v)) == 1 for v in seen.values()), "one key: one arc, and at most its twin"


@pytest.mark.parametrize("name", sorted(SA.HAND_MADE()))
def test_tolerance_zero_and_clean_rounds_are_the_shared_call(name):
    c = SA.HAND_MADE()[name]
    for tol in SA.TOLERANCES_HAND:
        out = run(c, tol)
        shared = R.simplify_shared(c["labels"], c["counts_obj"], *SC.table(c), R.tol2_q(tol))
        clean = int(out["safe"][4]) == 0 and int(out["safe"][6]) == 0
        assert int(out["safe"][7]) == S.ST_CONVERGED
        if tol == 0.0:
            assert clean and out["safe"].tolist()[:3] == [1, 0, 0] and not out["level"].any()
        if clean:
            assert all(np.array_equal(out[n], shared[n]) for n in ("rings", "vertices", "left", "counts")), (name, tol)
            assert np.array_equal(out["info"][:6], shared["info"][:6])
        else:
            assert int(out["safe"][1]) >= 1 and int(out["safe"][2]) >= 1 and int(out["info"][5]) == 0


def test_collapse_is_repaired():
    """Object 2 of `collapse` falls under one chord at 2 px: a defective ring in round 0, whole at the end."""
    c = SA.HAND_MADE()["collapse"]
    history = []
    out = run(c, 2.0, history=history)
    assert len(history[0][3]) >= 1 and int(out["safe"][6]) >= 1 and int(out["safe"][7]) == S.ST_CONVERGED and int(out["info"][5]) == 0
    assert all(int(r[2]) >= 3 for r in out["rings"][:int(out["counts"][1])])


def test_stopping_rules():
    c, table, prep = SA.survey_prep(*SA.DEEP_SCENE)
    q = R.tol2_q(2.0)
    full = S.simplify_safe(c["labels"], c["counts_obj"], *table, q, fast=True, prep=prep)
    assert int(full["safe"][1]) >= 3 and int(full["safe"][7]) == S.ST_CONVERGED
    for rounds in (1, 2):
        cut = S.simplify_safe(c["labels"], c["counts_obj"], *table, q, max_rounds=rounds, fast=True, prep=prep)
        assert cut["safe"].tolist()[:2] == [rounds, rounds] and int(cut["safe"][7]) == S.ST_NOT_CONVERGED
    below = S.simplify_safe(c["labels"], c["counts_obj"], *table, q, max_work=full["work"] - 1, fast=True, prep=prep)
    assert int(below["safe"][7]) == S.ST_OVER_WORK


def test_survey_table():
    """The table of the issue that introduced the call, from the restatement."""
    print("\nlabelling conn tol | objects with a defect 0 -> end | vertices 0 -> end | raising rounds: scenes | arcs refined of all")
    worst = 0
    for (labelling, conn, tol), want in SA.SURVEY_TABLE.items():
        obj0 = obj1 = v0 = v1 = refined = arcs = 0
        raising = {}
        for seed in SA.SEEDS:
            out, history = SA.survey_run(seed, labelling, conn, tol)
            assert int(out["safe"][7]) == S.ST_CONVERGED and int(out["safe"][5]) == 0 and int(out["info"][5]) == 0
            obj0 += len(SA.owners(history[0][0], history[0][1]))
            obj1 += len(SA.owners(history[-1][0], history[-1][1]))
            v0 += int(history[0][0]["counts"][3])
            v1 += int(out["counts"][3])
            k = int(out["safe"][1])
            raising[k] = raising.get(k, 0) + 1
            refined += int(out["safe"][2])
            arcs += int(out["info"][2])
            worst = max(worst, k)
        got = (obj0, obj1, v0, v1, dict(sorted(raising.items())), refined, arcs)
        print(f"{labelling:10s} {conn} {tol:3.1f} | {obj0} -> {obj1} | {v0} -> {v1} | {got[4]} | {refined} of {arcs}")
        assert obj1 == 0
        assert got == want, (labelling, conn, tol, got, want)
    assert worst <= 5
