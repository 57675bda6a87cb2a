"""The restatement of `c3d_scene_outlines` (tests/outlines_reference.py) checked on the CPU against facts it does not use: one
ring of positive area per object, the first vertex from the object table, areas, the even-odd round trip and scipy's count
of holes under the dual connectivity; fixed cases with literal vertices; then the GeoJSON writer on arrays, the refusals of
`predict` and of `predict_scene`'s parser that need no device, and the `_lib` signatures."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_reference as O  # noqa: E402
import outlines_reference as R  # noqa: E402

DENSITIES = (0.3, 0.5, 0.59, 0.7, 0.9)


def _holes(labels, i, connectivity):
    """Holes of object i: components of the padded complement under the dual connectivity, minus the outside."""
    from scipy import ndimage
    comp = np.pad(labels != i, 1, constant_values=True)
    dual = ndimage.generate_binary_structure(2, 1 if connectivity == 8 else 2)
    return ndimage.label(comp, structure=dual)[1] - 1


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", DENSITIES)
def test_restatement_against_independent_facts_on_random_masks(connectivity, density):
    rng = np.random.default_rng(int(density * 100) * 10 + connectivity)
    for _ in range(10):
        H, W = (int(v) for v in rng.integers(1, 25, 2))
        mask = (rng.random((H, W)) < density).astype(np.uint8)
        obj = O.objects(mask, connectivity=connectivity, max_objects=H * W)
        labels, n = obj["labels"], int(obj["counts"][0])
        rings = R.trace(labels, n, connectivity)
        assert [r["key"] for r in rings] == sorted(r["key"] for r in rings)
        for i in range(1, n + 1):
            own = [r for r in rings if r["id"] == i]
            outline = [r for r in own if r["area"] > 0]
            assert len(outline) == 1 and all(r["area"] < 0 for r in own if r is not outline[0])
            first = int(obj["table"][i - 1, 6])
            assert outline[0]["vertices"][0] == (first % W, first // W)
            assert sum(r["area"] for r in own) == int(obj["table"][i - 1, 0])
            assert np.array_equal(R.rasterise([r["vertices"] for r in own], H, W), labels == i)
            assert len(own) - 1 == _holes(labels, i, connectivity)
            for r in own:
                v = r["vertices"]
                assert len(v) >= 4 and r["perimeter"] == sum(abs(v[k][0] - v[k - 1][0]) + abs(v[k][1] - v[k - 1][1]) for k in range(len(v)))
                assert all((v[k][0] == v[k - 1][0]) != (v[k][1] == v[k - 1][1]) for k in range(len(v)))            # axis-parallel steps
                assert all((v[k][0] == v[k - 1][0]) != (v[k - 1][0] == v[k - 2][0]) for k in range(len(v)))        # no collinear vertex


def _traced(mask, connectivity):
    labels = O.components(np.asarray(mask, np.uint8), connectivity)
    return R.trace(labels, int(labels.max()), connectivity)


def test_diagonal_pair():
    (ring,) = _traced([[1, 0], [0, 1]], 8)
    assert ring["vertices"] == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]
    assert (ring["area"], ring["perimeter"], ring["id"]) == (2, 8, 1)
    a, b = _traced([[1, 0], [0, 1]], 4)
    assert a["vertices"] == [(0, 0), (1, 0), (1, 1), (0, 1)] and b["vertices"] == [(1, 1), (2, 1), (2, 2), (1, 2)]
    assert (a["area"], b["area"], a["id"], b["id"]) == (1, 1, 1, 2)


def test_block_with_diagonal_holes():
    block = np.ones((4, 4), np.uint8)
    block[1, 1] = block[2, 2] = 0
    outline, hole = _traced(block, 4)                       # the holes join across the diagonal
    assert (outline["area"], hole["area"], len(hole["vertices"]), hole["perimeter"]) == (16, -2, 8, 8)
    assert outline["vertices"] == [(0, 0), (4, 0), (4, 4), (0, 4)]
    # the hole's smallest edge is the bottom side of (0, 1), a corner here; it runs with the object on its right
    assert hole["vertices"] == [(2, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (2, 2)]
    rings = _traced(block, 8)                               # the holes split there
    assert [r["area"] for r in rings] == [16, -1, -1]
    assert rings[1]["vertices"] == [(2, 1), (1, 1), (1, 2), (2, 2)] and rings[2]["vertices"] == [(3, 2), (2, 2), (2, 3), (3, 3)]


def test_wide_hole_starts_at_a_corner_not_at_its_smallest_edge():
    block = np.ones((3, 5), np.uint8)
    block[1, 1:4] = 0
    outline, hole = _traced(block, 8)
    # the hole's smallest edge is the bottom side of (0, 1), reached straight from (0, 2)'s: no corner.  Its smallest corner
    # edge is the bottom side of (0, 3), whose start vertex is (4, 1)
    assert hole["key"] == 4 * 3 + 2 and hole["vertices"] == [(4, 1), (1, 1), (1, 2), (4, 2)] and hole["area"] == -3


def test_truncation_is_prefix_shaped():
    mask = (np.random.default_rng(3).random((12, 17)) < 0.3).astype(np.uint8)
    obj = O.objects(mask, connectivity=4, max_objects=200)
    full = R.outlines(obj["labels"], obj["counts"], 4, 200, 500, 5000)
    nr, _, nv, _, st = full["counts"]
    assert st == 0 and nr > 4 and np.array_equal(full["counts"], [nr, nr, nv, nv, 0])
    cut = R.outlines(obj["labels"], obj["counts"], 4, 200, nr - 1, nv // 2)
    assert cut["counts"][0] == nr and cut["counts"][1] == nr - 1 and cut["counts"][2] == nv and cut["counts"][4] == R.ST_TRUNCATED
    fit = cut["rings"][:, 1] >= 0
    k = int(fit[:nr - 1].sum())
    assert 0 < k < nr - 1 and fit[:k].all() and (cut["rings"][k:nr - 1, 1] == -1).all()
    assert cut["counts"][3] == full["rings"][k, 1] and np.array_equal(cut["vertices"][:cut["counts"][3]], full["vertices"][:cut["counts"][3]])
    assert np.array_equal(np.delete(cut["rings"][:nr - 1], 1, axis=1), np.delete(full["rings"][:nr - 1], 1, axis=1))
    few = R.outlines(obj["labels"], np.array([obj["counts"][0], 2], np.int32), 4, 2, 500, 5000)
    assert set(few["rings"][:few["counts"][1], 0]) == {1, 2} and few["counts"][4] == R.ST_TRUNCATED
    bad = R.outlines(obj["labels"], np.array([-1, 0], np.int32), 4, 200, 500, 5000)
    assert bad["counts"].tolist() == [0, 0, 0, 0, R.ST_BAD_COUNTS] and not bad["rings"].any()


def test_flip_is_a_different_rule():
    a, b = _traced([[1, 0], [0, 1]], 8), R.trace(O.components(np.array([[1, 0], [0, 1]], np.uint8), 8), 1, 8, flip=True)
    assert len(a) == 1 and len(b) == 2


def _arrays(mask, connectivity=8, **kw):
    obj = O.objects(np.asarray(mask, np.uint8), connectivity=connectivity, score=np.full(np.shape(mask), 0.5, np.float32),
                    max_objects=64)
    out = R.outlines(obj["labels"], obj["counts"], connectivity, 64, **kw)
    rows = int(obj["counts"][1])
    return obj["table"][:rows], out["rings"][:out["counts"][1]], out["vertices"][:out["counts"][3]]


def test_geojson_writer_on_arrays():
    from change3d_amd.scripts.predict_scene import polygons_geojson
    mask = np.zeros((7, 12), np.uint8)
    mask[1:6, 1:6] = 1
    mask[2, 2] = mask[4, 4] = 0                              # two holes
    mask[2, 8:11] = 1                                       # a second object, no hole
    doc, skipped = polygons_geojson(*_arrays(mask, max_rings=16, max_vertices=64))
    doc = json.loads(json.dumps(doc))
    assert skipped == [] and doc["type"] == "FeatureCollection" and len(doc["features"]) == 2
    a, b = doc["features"]
    assert a["type"] == "Feature" and a["geometry"]["type"] == "Polygon"
    assert a["properties"] == {"id": 1, "area": 23, "cls": 0, "score": 0.5, "perimeter": 20}
    assert a["geometry"]["coordinates"] == [[[1, 1], [6, 1], [6, 6], [1, 6], [1, 1]], [[3, 2], [2, 2], [2, 3], [3, 3], [3, 2]],
                                            [[5, 4], [4, 4], [4, 5], [5, 5], [5, 4]]]
    assert b["geometry"]["coordinates"] == [[[8, 2], [11, 2], [11, 3], [8, 3], [8, 2]]] and b["properties"]["id"] == 2
    # the vertex list ends inside object 1's rings: it is left out, object 2 (whose ring comes later) with it; a ring table
    # that ends before object 1's last hole leaves it out and keeps nothing it cannot vouch for
    doc, skipped = polygons_geojson(*_arrays(mask, max_rings=16, max_vertices=10))
    assert skipped == [1, 2] and doc["features"] == []
    doc, skipped = polygons_geojson(*_arrays(mask, max_rings=3, max_vertices=64))
    assert skipped == [1] and [f["properties"]["id"] for f in doc["features"]] == [2]


def test_predict_and_parser_refusals_that_need_no_device():
    from change3d_amd.infer import SceneInferencer, SceneOutlines
    from change3d_amd.scripts import predict_scene
    assert SceneOutlines._fields == ("rings", "vertices", "counts")
    inf = SceneInferencer.__new__(SceneInferencer)          # the refusal comes before the model or a device is looked at
    with pytest.raises(ValueError, match="objects=True"):
        inf.predict(np.zeros((4, 4, 6), np.uint8), outlines=True)
    with pytest.raises(ValueError, match="max_rings"):
        inf.predict(np.zeros((4, 4, 6), np.uint8), objects=True, outlines=True, max_rings=0)
    with pytest.raises(SystemExit):
        predict_scene.parse_args(["--weights", "w", "--polygons"])
    args = predict_scene.parse_args(["--weights", "w", "--objects", "--polygons", "--max_rings", "9"])
    assert args.polygons and args.max_rings == 9 and args.max_vertices is None
    assert not predict_scene.parse_args(["--weights", "w", "--objects"]).polygons


def test_outline_defaults_are_cut_to_the_scene():
    from change3d_amd.ops import scene_outlines_defaults
    assert scene_outlines_defaults(1024, 1024) == (262144, 4194304)
    assert scene_outlines_defaults(3, 5, 65536) == (15, 60) and scene_outlines_defaults(100, 100, 10) == (40, 640)


def test_lib_declares_the_two_new_symbols():
    from change3d_amd import _lib as L
    res, args = L.SIGNATURES["c3d_scene_outlines_ws_bytes"]
    assert res is C.c_int64 and args == [C.c_int32, C.c_int32]
    res, args = L.SIGNATURES["c3d_scene_outlines"]
    assert res is C.c_int32 and len(args) == 13 and args[2:8] == [C.c_int32] * 6
    assert (L.OUTLINE_ST_TRUNCATED, L.OUTLINE_ST_BAD_COUNTS, L.OUTLINE_ST_STEP_CAP) == (R.ST_TRUNCATED, R.ST_BAD_COUNTS, R.ST_STEP_CAP)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "change3d_hip.h")).read()
    assert "int64_t c3d_scene_outlines_ws_bytes(" in header and "int c3d_scene_outlines(" in header
    assert all(f"#define C3D_OUTLINE_ST_{n} {v}" in header for n, v in (("TRUNCATED", 1), ("BAD_COUNTS", 2), ("STEP_CAP", 4)))
    assert L.lib().c3d_scene_outlines_ws_bytes(0, 5) == -1 and L.lib().c3d_scene_outlines_ws_bytes(1 << 15, 1 << 14) == -2
    assert L.lib().c3d_scene_outlines_ws_bytes(1, 1) >= 256 + 2 * 4 * 16
