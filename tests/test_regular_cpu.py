"""The restatement of `c3d_rings_regularize` (tests/regular_reference.py) against independent witnesses, without a GPU: levels
and the mapping back computed in exact fractions and rounded at the end, the properties that follow from the rule, rotated
rectangles taken through the reference pipeline (rasterise, trace, simplify, hull, regularise, fill) with their IoU printed,
the two negative controls of the GPU test, and the argument checks of the `ops` wrappers."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_reference as FR  # noqa: E402
import hull_reference as HR  # noqa: E402
import objects_reference as O  # noqa: E402
import outlines_reference as T  # noqa: E402
import regular_cases as K  # noqa: E402
import regular_reference as R  # noqa: E402
import simplify_reference as SR  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

HAND_MADE = K.hand_made()


def _tables(name_or_case, max_objects=None):
    lists, ids, dirs = HAND_MADE[name_or_case] if isinstance(name_or_case, str) else name_or_case
    table = SR.table(lists, max_rings=len(lists) + 2, max_vertices=sum(len(v) for v in lists) + 3, ids=ids)
    return table, K.hull_tables(dirs, (max(ids) + 2) if max_objects is None else max_objects)


def _rings_of(out):
    return [(row, [tuple(p) for p in out["vertices"][row[1]:row[1] + row[2]].tolist()]) for row in out["rings"][:int(out["counts"][1])].tolist() if row[1] >= 0]


def _primitive(d):
    g = math.gcd(abs(d[0]), abs(d[1]))
    return d[0] // g, d[1] // g


def _round_half_up(q):
    return math.floor(q + Fraction(1, 2))


def _witness(v, u, f):
    """The rule once more, in fractions throughout: levels as true weighted means of the edge midpoints in the true frame
    (divided by |u|^2 only at the very end), rounded half up once per level and once per coordinate."""
    n, S, N = len(v), 1 << f, u[0] * u[0] + u[1] * u[1]
    T_ = [Fraction(x * u[0] + y * u[1]) for x, y in v]
    C_ = [Fraction(y * u[0] - x * u[1]) for x, y in v]
    H = [abs(T_[(k + 1) % n] - T_[k]) >= abs(C_[(k + 1) % n] - C_[k]) for k in range(n)]
    J = [k for k in range(n) if H[k - 1] != H[k]]
    levels = []
    for j in range(len(J)):
        k, num, den = J[j - 1], Fraction(0), Fraction(0)
        h = H[k]
        while k != J[j]:
            a, b = (T_, C_) if h else (C_, T_)
            w = abs(a[(k + 1) % n] - a[k])
            num += w * (b[k] + b[(k + 1) % n]) / 2
            den += w
            k = (k + 1) % n
        levels.append(_round_half_up(S * num / den))
    out = []
    for j, k in enumerate(J):
        behind, ahead = levels[j], levels[(j + 1) % len(J)]
        Tq, Cq = (behind, ahead) if H[k] else (ahead, behind)
        out.append((_round_half_up(Fraction(Tq * u[0] - Cq * u[1], N)), _round_half_up(Fraction(Tq * u[1] + Cq * u[0], N))))
    return out


@pytest.mark.parametrize("name", list(HAND_MADE))
@pytest.mark.parametrize("f", [0, 4, 8])
def test_restatement_against_fractions_and_the_properties_of_the_rule(name, f):
    (rings, vertices, counts), hull = _tables(name)
    out = R.regularize(rings, vertices, counts, *hull, f)
    S = 1 << f
    assert out["counts"][4] == 0 and out["counts"][1] == counts[1]
    for r, (row, new) in enumerate(_rings_of(out)):
        old = [tuple(p) for p in vertices[rings[r, 1]:rings[r, 1] + rings[r, 2]].tolist()]
        assert row[0] == rings[r, 0] and row[7] == len(old) and len(new) <= len(old)
        u = R.direction(row[0], *hull)
        if not row[3]:
            assert new == [(x * S, y * S) for x, y in old]
            continue
        info = {}
        assert R.regular_ring(old, u, f, info=info) == new == _witness(old, u, f)
        assert len(new) % 2 == 0 and len(new) >= 4
        Ts, Cs = zip(*(R.frame(p, u) for p in old))
        assert all(S * min(Ts) <= Tq <= S * max(Ts) and S * min(Cs) <= Cq <= S * max(Cs) for Tq, Cq in info["levels"])
        lv, runs = info["levels"], info["runs"]
        for j in range(len(lv)):                             # vertices j and j + 1 are the ends of the run that ends at j + 1
            h = runs[(j + 1) % len(lv)][0]
            assert lv[j][1 if h else 0] == lv[(j + 1) % len(lv)][1 if h else 0], "an H run keeps one C, a V run one T"
            assert runs[j][0] != runs[j - 1][0], "consecutive vertices share C and T alternately"


def test_copied_and_regularised_rows_are_the_expected_ones():
    flags = {name: [row[3] for row, _ in _rings_of(R.regularize(*_tables(name)[0], *_tables(name)[1], 4))] for name in HAND_MADE}
    assert flags["n3"] == [0] and flags["R0"] == [0] and flags["R2"] == [0] and flags["zero_edge"] == [0]
    assert flags["n4_junction_at_0"] == [1] and flags["run_wraps_0"] == [1] and flags["tie45"] == [1] and flags["gcd"] == [1]
    assert flags["negative_u"] == [1, 1] and flags["holes"] == [1, 1, 1] and flags["not_contiguous"] == [1, 1, 1, 1]
    assert flags["no_direction"] == [0, 0, 1, 0, 0] and flags["empty_ring"] == [0, 1, 0]
    info = {}
    R.regular_ring(HAND_MADE["run_wraps_0"][0][0], (1, 0), 4, info=info)
    assert info["junctions"] == [1, 2, 3, 4] and info["runs"][0][1] == 8, "the H run of edges 4 and 0 wraps index 0"
    R.regular_ring(HAND_MADE["n4_junction_at_0"][0][0], (1, 0), 4, info=info)
    assert info["junctions"][0] == 0
    assert R.direction(1, *K.hull_tables({1: (6, 2)}, 3)) == (3, 1)
    assert all(t < 0 for t, _ in (R.frame(p, (-3, -1)) for p in K.WOBBLY))


@pytest.mark.parametrize("f", [0, 4, 8])
def test_axis_parallel_rectilinear_rings_come_back_as_themselves(f):
    plus = [(2, 0), (4, 0), (4, 2), (6, 2), (6, 4), (4, 4), (4, 6), (2, 6), (2, 4), (0, 4), (0, 2), (2, 2)]
    for ring in (plus, plus[5:] + plus[:5], [(1, 1), (9, 1), (9, 5), (1, 5)], [(3, 2), (3, 4), (7, 4), (7, 2)]):
        assert R.regular_ring(ring, (1, 0), f) == [(x << f, y << f) for x, y in ring]


def test_full_range_needs_more_than_64_bits_and_still_agrees_with_fractions():
    lists, ids, dirs = K.FULL_RANGE
    u = _primitive(dirs[1])
    for ring in lists:
        info = {}
        new = R.regular_ring(ring, u, 8, info=info)
        assert new == _witness(ring, u, 8) and len(new) >= 4
        assert max(abs(256 * A + W) for _, W, A in info["runs"]) >= 2 ** 63, "the dividend of a level leaves 64 bits"
        assert max(abs(q) for lv in info["levels"] for q in lv) < 2 ** 38


def test_many_small_rings_against_fractions():
    lists, ids, dirs = K.many_small(300, seed=5)
    hull = K.hull_tables(dirs, 42)
    seen = 0
    for ring, rid in zip(lists, ids):
        u = R.direction(rid, *hull)
        if u is not None and (new := R.regular_ring(ring, u, 4)) is not None:
            assert new == _witness(ring, u, 4)
            seen += 1
    assert seen > 150


def test_the_negative_controls_differ_where_the_gpu_test_says():
    for name, wrong in (("tie45", dict(tie="strict")), ("negative_u", dict(division="truncate"))):
        table, hull = _tables(name)
        good, bad = R.regularize(*table, *hull, 4), R.regularize(*table, *hull, 4, **wrong)
        assert not np.array_equal(good["vertices"], bad["vertices"]), name


DIRECTIONS = [(3, 1), (2, 5), (1, 1), (1, 0), (5, -2)]
IOU = {}


@pytest.mark.parametrize("d", DIRECTIONS)
def test_rotated_rectangles_through_the_reference_pipeline(d):
    """Rasterise, trace, simplify at 1 px, hull, regularise, fill at 1/16 px.  The IoU against the raster is printed and
    recorded in the README; it is a measurement, not a threshold.  Measured on 40 x 25 px: (3, 1) 0.9724, (2, 5) 0.9910,
    (1, 1) 1.0000, (1, 0) 1.0000, (5, -2) 0.9832."""
    mask = K.rotated_rectangle(d)
    H, W = mask.shape
    labels = O.components(mask, 8)
    n_obj = int(labels.max())
    assert n_obj == 1
    raw = T.outlines(labels, np.array([n_obj, n_obj], np.int32), 8, max_objects=4, max_rings=8, max_vertices=4 * H * W)
    simple = SR.simplify(raw["rings"], raw["vertices"], raw["counts"], SR.tol2_q(1.0))
    hull = HR.hulls(raw["rings"], raw["vertices"], raw["counts"], 4, 4 * H * W)
    hull = (hull["hulls"], hull["vertices"], hull["rects"], hull["counts"])
    out = R.regularize(simple["rings"], simple["vertices"], simple["counts"], *hull, 4)
    filled = FR.fill(out["rings"], out["vertices"], out["counts"], H, W, f=4, max_objects=4)["labels"] > 0
    iou = (filled & (mask > 0)).sum() / max(1, (filled | (mask > 0)).sum())
    u = R.direction(1, *hull)
    old = [tuple(p) for p in simple["vertices"][:simple["rings"][0, 2]].tolist()]
    info = {}
    R.regular_ring(old, u, 4, info=info)
    runs = len(info.get("junctions", []))
    print(f"rotated rectangle along {d}: u = {u}, simplified n = {len(old)}, runs = {runs}, n' = {out['rings'][0, 2]}, IoU = {iou:.4f}")
    assert filled.any() and out["counts"][4] == 0
    if runs == 4:
        assert out["rings"][0, 2] == 4 and out["rings"][0, 3] == 1


def test_ops_bindings_exist_and_refuse_host_tensors():
    assert callable(ops.rings_regularize) and callable(ops.rings_regularize_limits)
    assert L.REGULAR_ST_BAD_ROW == R.ST_BAD_ROW == 256
    (rings, vertices, counts), hull = _tables("gcd")
    host = [torch.from_numpy(a) for a in (rings, vertices, counts) + tuple(hull)]
    with pytest.raises(L.Change3DHipError):
        ops.rings_regularize(*host)
