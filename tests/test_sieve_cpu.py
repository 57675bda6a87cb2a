"""The restatement of `c3d_regions_sieve` (tests/sieve_reference.py) on hand-counted cases, the survey of how the rule
behaves on noisy class maps (printed, and asserted against the rule's own invariants), and the pipeline check: keyed regions,
raw and sieved, through the restatements of the tracer, the fill and the crossing-free simplifier.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_reference as F  # noqa: E402
import outlines_reference as T  # noqa: E402
import regions_cases as RC  # noqa: E402
import regions_reference as R  # noqa: E402
import safe_reference as SAFE  # noqa: E402
import shared_reference as SH  # noqa: E402
import sieve_reference as S  # noqa: E402

SURVEY = [(4, 2, 4), (4, 4, 9), (4, 7, 16), (8, 4, 9), (8, 7, 16)]      # (connectivity, classes, min_area)
SEEDS = 20


@pytest.mark.parametrize("name", sorted(RC.HAND))
def test_hand_counted_cases(name):
    key, min_area, connectivity, want = RC.HAND[name]
    out = S.sieve(key, min_area, connectivity)
    assert np.array_equal(out["key_out"], want), (name, out["key_out"])
    assert out["info"][0] == 0


def test_what_the_hand_cases_are_about():
    run = lambda name: S.sieve(*RC.HAND[name][:3])  # noqa: E731
    a = S.analyse(*[RC.HAND["longer_border"][i] for i in (0, 2, 1)])
    assert a["target"] == {3: 1} and a["entries"] == 2                   # the speck is region 3; key 1's region is region 1
    a = S.analyse(*[RC.HAND["bg_full_tie"][i] for i in (0, 2, 1)])
    assert a["target"] == {1: S.BG} and a["moves"] == {1: 0}
    a = S.analyse(*[RC.HAND["mutual_pair"][i] for i in (0, 2, 1)])
    assert a["target"] == {1: 2, 2: 1} and a["moves"] == {1: 2}          # both small, each the other's target: one moves
    out = run("chain_of_three")
    assert out["trace"][0][3:] == (3, 3) and out["info"][1:4].tolist() == [1, 3, 6]
    out = run("merge_after")
    assert [t[0] for t in out["trace"]] == [3, 1]                         # one region the round after
    out = run("whole_scene")
    assert out["info"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0]              # it stays, and that counts as converged


def test_status_words():
    key = RC.block_noise(20, 20, 7, seed=0)                               # a map that needs two rounds
    full = S.sieve(key, 16, 4)
    assert full["info"][0] == 0 and full["info"][1] == 2
    cut = S.sieve(key, 16, 4, max_rounds=1)
    assert cut["info"][0] == S.ST_NOT_CONVERGED and cut["info"][1] == 1
    assert np.array_equal(cut["key_out"], S.paint(key, S.analyse(key, 4, 16)))
    tight = S.sieve(key, 16, 4, table_capacity=16)
    assert tight["info"][0] == S.ST_TABLE_FULL and np.array_equal(tight["key_out"], key) and tight["info"][1] == 0
    same = S.sieve(key, 1, 4)
    assert np.array_equal(same["key_out"], key) and same["info"][:5].tolist() == [0, 0, 0, 0, 0]


def test_survey_of_the_rule(capsys):
    lines = ["conn classes min_area  regions before -> after  scenes needing 0/1/2/3+ rounds  longest chain"]
    for connectivity, classes, min_area in SURVEY:
        before = after = longest = 0
        needed = [0, 0, 0, 0]
        for seed in range(SEEDS):
            key = RC.block_noise(20, 20, classes, seed)
            out = S.sieve(key, min_area, connectivity, max_rounds=8)
            trace = out["trace"]
            assert out["info"][0] == 0, (connectivity, classes, seed)                      # converged
            final = R.regions(out["key_out"], connectivity)
            area = np.bincount(final.ravel())[1:]
            if (area < min_area).any():                                                    # only a region that is alone stays
                assert all(r not in S.analyse(out["key_out"], connectivity, min_area)["target"]
                           for r in np.flatnonzero(area < min_area) + 1)
            for a, b in zip(trace, trace[1:]):
                assert b[0] < a[0]                                                         # every round that moves lowers the count
            before += trace[0][0]
            after += trace[-1][0]
            longest = max(longest, max(t[4] for t in trace))
            needed[min(int(out["info"][1]), 3)] += 1
        lines.append(f"{connectivity:4d} {classes:7d} {min_area:8d}  {before:6d} -> {after:5d}  "
                     f"{needed[0]:2d} / {needed[1]:2d} / {needed[2]:2d} / {needed[3]:2d}  {longest:3d}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_regions_go_through_the_tracer_the_fill_and_the_safe_simplifier(connectivity):
    q = SH.tol2_q(1.0)
    for seed in range(12):
        key = RC.block_noise(20, 20, 4, 100 + seed)
        for sieved in (False, True):
            k = S.sieve(key, 6, connectivity)["key_out"] if sieved else key
            obj = R.region_objects(k, connectivity=connectivity, max_objects=400)
            labels, counts_obj = obj["labels"], obj["counts"]
            o = T.outlines(labels, counts_obj, connectivity, max_objects=400, max_rings=labels.size, max_vertices=4 * labels.size)
            assert o["counts"][4] == 0
            back = F.fill(o["rings"], o["vertices"], o["counts"], 20, 20, max_objects=400)
            assert np.array_equal(back["labels"], labels), (seed, sieved)
            out = SAFE.simplify_safe(labels, counts_obj, o["rings"], o["vertices"], o["counts"], q, fast=True, max_objects=400)
            assert out["safe"][7] == SAFE.ST_CONVERGED, (seed, sieved, out["safe"])
            assert SH.twin_failures(out) == [], (seed, sieved)
