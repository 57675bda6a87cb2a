"""The restatement of `c3d_outlines_simplify` (tests/simplify_reference.py) checked on the CPU against facts it does not use:
the kept vertices are an ordered subsequence with both anchors, a zero tolerance is the identity on traced rings, every
dropped vertex lies within the tolerance of the kept chord that spans it (exact, with fractions), the largest tolerance
leaves a triangle, an independent recursive float64 Douglas-Peucker agrees where no comparison is close, and the comparison
is strict.  Then the host pieces: the tolerance conversion, the GeoJSON writer with simplified rings, the refusals that
need no device and the `_lib` signatures."""
import ctypes as C
import json
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_reference as O  # noqa: E402
import outlines_reference as R  # noqa: E402
import simplify_cases as K  # noqa: E402
import simplify_reference as S  # noqa: E402


def _traced(mask, connectivity=8):
    labels = O.components(np.asarray(mask, np.uint8), connectivity)
    return [r["vertices"] for r in R.trace(labels, int(labels.max()), connectivity)]


MASKS = K.masks()
RINGS = {name: _traced(mask) for name, mask in MASKS.items()}


def test_the_cases_are_what_they_claim():
    assert all(m.shape[0] <= 96 and m.shape[1] <= 96 for m in MASKS.values())
    assert any(len(set(v)) < len(v) for v in RINGS["diagonal_pair"]), "the 8-connected pair repeats a lattice point"
    assert len(RINGS["holed"]) == 4 and len(RINGS["serpentine"]) == 1 and max(len(v) for v in RINGS["disc"]) > 100
    info = {}
    S.simplify_ring(RINGS["serpentine"][0], S.tol2_q(1.0), info=info)
    assert info["depth"] >= len(RINGS["serpentine"][0]) // 8 > 4          # deep: levels grow with the ring, not its logarithm


@pytest.mark.parametrize("name", list(RINGS))
def test_kept_vertices_are_an_ordered_subsequence_with_both_anchors(name):
    for tol in K.TOLERANCES:
        for v in RINGS[name]:
            info = {}
            kept = S.simplify_ring(v, S.tol2_q(tol), info=info)
            assert kept == sorted(set(kept)) and all(0 <= k < len(v) for k in kept)
            d = [(p[0] - v[0][0]) ** 2 + (p[1] - v[0][1]) ** 2 for p in v]
            assert info["A"] == 0 and d[info["B"]] == max(d) and all(d[k] < max(d) for k in range(info["B"]))
            assert 0 in kept and info["B"] in kept and len(kept) >= 3


@pytest.mark.parametrize("name", list(RINGS))
def test_zero_tolerance_is_the_identity_on_traced_rings(name):
    for v in RINGS[name]:
        assert S.simplify_ring(v, 0) == list(range(len(v)))
    rings, vertices, counts = S.table(RINGS[name])
    out = S.simplify(rings, vertices, counts, 0)
    assert np.array_equal(out["vertices"], vertices) and np.array_equal(out["counts"], counts)
    assert np.array_equal(out["rings"][:, :3], rings[:, :3]) and np.array_equal(out["rings"][:, 7], rings[:, 2])
    assert np.array_equal(out["rings"][:, 3], 2 * rings[:, 3]), "traced rings have integer areas"


def _segment_distance2(a, b, p):
    """Exact squared distance to the segment, by projection: no case table."""
    a, b, p = ([Fraction(c) for c in q] for q in (a, b, p))
    d = (b[0] - a[0], b[1] - a[1])
    L2 = d[0] * d[0] + d[1] * d[1]
    t = 0 if L2 == 0 else min(max(((p[0] - a[0]) * d[0] + (p[1] - a[1]) * d[1]) / L2, 0), 1)
    q = (a[0] + t * d[0], a[1] + t * d[1])
    return (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2


@pytest.mark.parametrize("name", list(RINGS))
def test_dropped_vertices_lie_within_the_tolerance_of_their_chord(name):
    for tol in K.TOLERANCES:
        q = S.tol2_q(tol)
        for v in RINGS[name]:
            info = {}
            kept = S.simplify_ring(v, q, info=info)
            if len(v) <= 3:
                continue
            # the third vertex of a collapsed ring is extra: the bound holds for the chords of the chains A..B and B..n
            chain = sorted(set(k for k in kept if any(k in (i, j, m) for i, j, m, _, _ in info["judged"])) | {0, info["B"]})
            ends = chain + [len(v)]
            w = list(v) + [v[0]]
            for i, j in zip(ends[:-1], ends[1:]):
                for k in range(i + 1, j):
                    if k in kept:
                        continue                            # only the extra vertex can sit inside a kept chord
                    assert 16 * _segment_distance2(w[i], w[j], w[k]) <= q, (name, tol, i, j, k)


@pytest.mark.parametrize("name", list(RINGS))
def test_the_largest_tolerance_leaves_triangles_of_non_zero_area(name):
    for v in RINGS[name]:
        kept = S.simplify_ring(v, S.tol2_q(1024))
        assert len(kept) == 3 and S.shoelace2([v[k] for k in kept]) != 0


def _float_dp(v, eps, margins):
    """Textbook recursive Douglas-Peucker in float64 on the two chains of the ring, squared segment distances.  Appends the
    relative margin of every comparison against eps^2 to `margins`."""
    n = len(v)
    if n <= 3:
        return list(range(n))
    w = [(float(x), float(y)) for x, y in v] + [(float(v[0][0]), float(v[0][1]))]

    def d2(a, b, p):
        dx, dy = b[0] - a[0], b[1] - a[1]
        L2 = dx * dx + dy * dy
        if L2 == 0.0:
            return (p[0] - a[0]) ** 2 + (p[1] - a[1]) ** 2
        t = ((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) / L2
        if t <= 0.0:
            return (p[0] - a[0]) ** 2 + (p[1] - a[1]) ** 2
        if t >= 1.0:
            return (p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2
        c = dx * (p[1] - a[1]) - dy * (p[0] - a[0])
        return c * c / L2

    def rec(i, j):
        if j <= i + 1:
            return []
        far = [d2(w[i], w[j], w[k]) for k in range(i + 1, j)]
        m = i + 1 + far.index(max(far))
        margins.append(abs(max(far) - eps * eps) / max(eps * eps, 1e-300) if eps > 0 else (1.0 if max(far) == 0 or max(far) > 1e-6 else 0.0))
        return rec(i, m) + [m] + rec(m, j) if max(far) > eps * eps else []

    from_a = [(p[0] - w[0][0]) ** 2 + (p[1] - w[0][1]) ** 2 for p in w[:n]]
    B = from_a.index(max(from_a))
    kept = sorted(set([0, B] + rec(0, B) + rec(B, n)))
    if len(kept) <= 2:
        c = [abs((w[B][0] - w[0][0]) * (p[1] - w[0][1]) - (w[B][1] - w[0][1]) * (p[0] - w[0][0])) for p in w[:n]]
        kept = sorted(set(kept + [c.index(max(c))]))
    return kept


@pytest.mark.parametrize("name", list(RINGS))
def test_agrees_with_a_recursive_float64_implementation(name):
    # tolerances whose square is no ratio of small integers times 1/16 a lattice distance can hit: nothing lands within 1e-9
    sys.setrecursionlimit(10000)
    for tol in (0.0, 0.75, 1.3, 2.9, 7.3):            # tol2_q = 0, 9, 27, 135, 853
        q = S.tol2_q(tol)
        eps = math.sqrt(q / 16)
        for v in RINGS[name]:
            margins = []
            want = _float_dp(v, eps, margins)
            assert all(m > 1e-9 for m in margins), "choose another tolerance: a comparison lies on the threshold"
            assert S.simplify_ring(v, q) == want, (name, tol)


def test_the_comparison_is_strict_and_the_distance_is_to_the_segment():
    on, off = K.hand_made()["strictness"]
    q = S.tol2_q(1.0)
    assert S.distance((0, 0), (6000, 8000), (1, 3)) == (10 ** 8, 10 ** 8) and q == 16
    assert S.simplify_ring(on, q) == [0, 2, 3] and S.simplify_ring(off, q) == [0, 1, 2, 3]
    assert S.simplify_ring(on, q, strict=False) == [0, 1, 2, 3], "the wrong rule keeps a vertex that lies on the tolerance"
    assert S.simplify_ring(on, q - 1) == [0, 1, 2, 3]
    # beyond the chord's end the distance is to the end point, not to the line
    assert S.distance((0, 0), (10, 0), (13, 4)) == (25 * 100, 100) and S.distance((0, 0), (10, 0), (13, 4), segment=False) == (1600, 100)
    assert S.distance((0, 0), (10, 0), (-3, 4)) == (2500, 100) and S.distance((2, 2), (2, 2), (5, 6)) == (25, 1)
    hook = K.hand_made()["hook"][0]                        # (4, 11) lies 1 px off the line of a chord that it lies before
    assert S.simplify_ring(hook, S.tol2_q(2.0)) == [0, 1, 2, 3] and S.simplify_ring(hook, S.tol2_q(2.0), segment=False) == [0, 2, 3]


def test_the_table_rules_of_the_restatement():
    rings, vertices, counts = S.table(K.hand_made()["holed"] + K.hand_made()["degenerate"], max_rings=9, max_vertices=40)
    out = S.simplify(rings, vertices, counts, S.tol2_q(1.0))
    assert out["counts"].tolist() == [7, 7, int(out["rings"][:7, 2].sum()), int(out["rings"][:7, 2].sum()), 0]
    assert out["rings"][0].tolist() == [1, 0, 4, 216, 42, 0, 0, 4] and out["rings"][1, 3] < 0 and not out["rings"][7:].any()
    assert out["rings"][2].tolist()[1:4] == [int(out["rings"][:2, 2].sum()), 1, 0], "five equal points keep one"
    assert out["rings"][6].tolist()[1:4] == [int(out["counts"][2]), 0, 0], "an empty ring stays empty"
    cut = rings.copy()
    cut[1, 1] = -1                                           # a ring the outlines call had no room for
    cut[3, 2] = 400                                          # past the written vertices
    vertices[int(rings[4, 1])] = (16385, 0)                  # a coordinate out of range
    counts[4] = S.ST_TRUNCATED
    out = S.simplify(cut, vertices, counts, S.tol2_q(1.0))
    assert out["counts"][4] == S.ST_TRUNCATED | S.ST_BAD_INPUT
    assert [out["rings"][r, 1:4].tolist() for r in (1, 3, 4)] == [[-1, 0, 0]] * 3 and out["rings"][3, 7] == 400
    assert out["rings"][2, 1] == 4 and out["rings"][5, 1] == 5
    counts[4] = S.ST_BAD_COUNTS | S.ST_TRUNCATED
    out = S.simplify(cut, vertices, counts, 16)
    assert out["counts"].tolist() == [0, 0, 0, 0, S.ST_BAD_COUNTS] and not out["rings"].any() and not out["vertices"].any()


def test_simplify_tol2_q():
    from change3d_amd.ops import simplify_tol2_q
    assert [simplify_tol2_q(t) for t in (0, 0.5, 1, 2, 3.0, 1024)] == [0, 4, 16, 64, 144, 16 * 1024 * 1024]
    assert simplify_tol2_q(0.7) == round(16 * 0.49) == S.tol2_q(0.7) and simplify_tol2_q(0.1) == 0
    for bad in (-0.001, 1024.001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            simplify_tol2_q(bad)


def _arrays(mask, connectivity=8, **kw):
    obj = O.objects(np.asarray(mask, np.uint8), connectivity=connectivity, score=np.full(np.shape(mask), 0.5, np.float32), max_objects=64)
    out = R.outlines(obj["labels"], obj["counts"], connectivity, 64, **kw)
    rows = int(obj["counts"][1])
    return obj["table"][:rows], out


def test_geojson_writer_with_simplified_rings():
    from change3d_amd.scripts.predict_scene import polygons_geojson
    mask = np.zeros((40, 48), np.uint8)
    yy, xx = np.mgrid[:40, :48]
    mask[(xx - 14) ** 2 + (yy - 16) ** 2 < 144] = 1          # a disc with a hole
    mask[14:18, 12:17] = 0
    mask[30:36, 30:44] = 1                                   # a box
    table, out = _arrays(mask, max_rings=16, max_vertices=400)
    nr, nv = int(out["counts"][1]), int(out["counts"][3])
    raw = (table, out["rings"][:nr], out["vertices"][:nv])
    simple = S.simplify(out["rings"], out["vertices"], out["counts"], S.tol2_q(1.0))
    before, skipped0 = polygons_geojson(*raw)
    assert json.dumps(before) == json.dumps(polygons_geojson(*raw, None)[0]) == json.dumps(polygons_geojson(*raw, simplified=None)[0])
    assert all(set(f["properties"]) == {"id", "area", "cls", "score", "perimeter"} for f in before["features"])
    doc, skipped = polygons_geojson(*raw, (simple["rings"][:nr], simple["vertices"][:int(simple["counts"][3])]))
    doc = json.loads(json.dumps(doc))
    assert skipped == skipped0 == [] and len(doc["features"]) == len(before["features"]) == 2
    for f, g in zip(doc["features"], before["features"]):
        p = f["properties"]
        assert {k: p[k] for k in g["properties"]} == g["properties"]
        rings_f, rings_g = f["geometry"]["coordinates"], g["geometry"]["coordinates"]
        assert len(rings_f) == len(rings_g) and all(r[0] == r[-1] and len(r) >= 4 for r in rings_f)
        assert p["vertices_raw"] == sum(len(r) - 1 for r in rings_g) and p["vertices"] == sum(len(r) - 1 for r in rings_f)
        assert all(set(map(tuple, a)) <= set(map(tuple, b)) for a, b in zip(rings_f, rings_g))
    disc, box = doc["features"]
    assert disc["properties"]["vertices"] < disc["properties"]["vertices_raw"] and box["properties"]["vertices"] == 4
    # a ring whose simplified area vanished or changed sign keeps its raw vertices
    broken = simple["rings"][:nr].copy()
    broken[0, 3] = 0
    broken[1, 3] = -broken[1, 3]
    broken[2, 1] = -1
    doc2, _ = polygons_geojson(*raw, (broken, simple["vertices"][:int(simple["counts"][3])]))
    by_row = {}
    for at, row in enumerate(out["rings"][:nr].tolist()):
        by_row[at] = out["vertices"][row[1]:row[1] + row[2]].tolist()
    flat = [r for f in doc2["features"] for r in f["geometry"]["coordinates"]]
    raw_flat = [r for f in before["features"] for r in f["geometry"]["coordinates"]]
    fell_back = [a == b for a, b in zip(flat, raw_flat)]
    assert sum(fell_back) >= 3 and sum(f["properties"]["vertices"] for f in doc2["features"]) > sum(f["properties"]["vertices"] for f in doc["features"])


def test_predict_and_parser_refusals_that_need_no_device():
    from change3d_amd.infer import SceneInferencer
    from change3d_amd.scripts import predict_scene
    inf = SceneInferencer.__new__(SceneInferencer)          # the refusal comes before the model or a device is looked at
    with pytest.raises(ValueError, match="outlines=True"):
        inf.predict(np.zeros((4, 4, 6), np.uint8), objects=True, simplify=1.0)
    with pytest.raises(ValueError, match="1024"):
        inf.predict(np.zeros((4, 4, 6), np.uint8), objects=True, outlines=True, simplify=2000.0)
    with pytest.raises(SystemExit):
        predict_scene.parse_args(["--weights", "w", "--objects", "--simplify", "1.0"])
    with pytest.raises(SystemExit):
        predict_scene.parse_args(["--weights", "w", "--objects", "--polygons", "--simplify", "-1"])
    args = predict_scene.parse_args(["--weights", "w", "--objects", "--polygons", "--simplify", "1.5"])
    assert args.simplify == 1.5 and predict_scene.parse_args(["--weights", "w", "--objects", "--polygons"]).simplify is None


def test_lib_declares_the_new_symbols():
    from change3d_amd import _lib as L
    res, args = L.SIGNATURES["c3d_outlines_simplify"]
    assert res is C.c_int32 and len(args) == 11 and args[3:6] == [C.c_int32, C.c_int32, C.c_int64]
    assert L.SIGNATURES["c3d_outlines_simplify_ws_bytes"] == (C.c_int64, [C.c_int32, C.c_int32])
    assert (L.SIMPLIFY_ST_BAD_INPUT, L.SIMPLIFY_TOL2_Q_MAX) == (S.ST_BAD_INPUT, S.TOL2_Q_MAX)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "change3d_hip.h")).read()
    assert "int c3d_outlines_simplify(" in header and "int64_t c3d_outlines_simplify_ws_bytes(" in header
    assert "void c3d_outlines_simplify_limits(" in header and "#define C3D_SIMPLIFY_ST_BAD_INPUT 8" in header
    lib = L.lib()
    assert lib.c3d_outlines_simplify_ws_bytes(0, 5) == -1 and lib.c3d_outlines_simplify_ws_bytes(5, 0) == -1
    assert lib.c3d_outlines_simplify_ws_bytes(1, 1) >= 256 + 16 + 17
    out = (C.c_int32 * 2)()
    lib.c3d_outlines_simplify_limits(out)
    assert 4 <= out[0] < out[1]
