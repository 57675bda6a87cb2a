"""The restatement of `c3d_rings_fill` (tests/fill_reference.py) checked on the CPU against what it does not use: the even-odd
raster of tests/outlines_reference.py on round trips, and an exact point-in-polygon in `fractions.Fraction`, also where a
centre lies on an edge or a vertex.  Then `change3d_amd/vector_labels.py` on GeoJSON written by `polygons_geojson` and on an
xBD-style label file, the parser's errors, the GeoJSON writer's `iou` guard, the new refusals of `predict` and of
`predict_scene`'s parser, and the `_lib` signatures."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as K  # noqa: E402
import fill_reference as F  # noqa: E402
import objects_reference as O  # noqa: E402
import outlines_reference as R  # noqa: E402

from change3d_amd import vector_labels as V  # noqa: E402


def _traced_table(labels, connectivity):
    n = int(labels.max())
    traced = R.trace(labels, n, connectivity)
    return F.table([r["vertices"] for r in traced], [r["id"] for r in traced]), traced, n


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", [(17, 23), (40, 33), (30, 30)])
def test_restatement_gives_traced_labels_back(shape, connectivity):
    rng = np.random.default_rng(shape[0] * 10 + connectivity)
    masks = [(rng.random(shape) < d).astype(np.uint8) for d in (0.3, 0.59, 0.8)] + [K.touching_mask(*shape) if shape[0] >= 30 else K.masks(*shape)["blobs"]]
    for mask in masks:
        obj = O.objects(mask, connectivity=connectivity, max_objects=mask.size)
        labels = obj["labels"]
        table, traced, n = _traced_table(labels, connectivity)
        got = F.fill(*table, *shape, 0, None, max_objects=mask.size)
        assert np.array_equal(got["labels"], labels)
        assert np.array_equal(got["table"][:, :5], obj["table"][:, :5]) and np.array_equal(got["table"][:, 6], obj["table"][:, 6])
        assert got["counts_obj"].tolist() == [n, n] and got["info"].tolist() == [0, len(traced), n, 0]
        for i in range(1, n + 1):                           # ring by ring against the raster of the outlines' restatement
            own = [r["vertices"] for r in traced if r["id"] == i]
            assert np.array_equal(R.rasterise(own, *shape), labels == i)


def test_restatement_on_pieces_that_share_pixel_edges():
    labels = np.zeros((12, 14), dtype=np.int32)
    labels[2:9, 1:6], labels[2:9, 6:11], labels[9:11, 3:9] = 1, 2, 3        # three pieces, two shared edges, one T junction
    labels[4:6, 5:7] = 4
    table, traced, n = _traced_table(labels, 4)
    assert np.array_equal(F.fill(*table, 12, 14, 0, None, max_objects=4)["labels"], labels), "polygons that share edges partition the pixels"
    for f in (1, 4):                                     # the same polygons on a finer lattice
        fine = F.table([[(x << f, y << f) for x, y in r["vertices"]] for r in traced], [r["id"] for r in traced])
        assert np.array_equal(F.fill(*fine, 12, 14, f, None, max_objects=4)["labels"], labels)


@pytest.mark.parametrize("f", [0, 1, 4])
def test_restatement_against_exact_rationals(f):
    rng = np.random.default_rng(40 + f)
    s = 1 << f
    H, W = 9, 11
    half = max(s // 2, 1)
    on_centres = 0
    for trial in range(40):
        n = int(rng.integers(3, 8))
        if trial % 2 and f:                              # vertices on pixel centres: odd multiples of half a pixel
            ring = [(int(2 * rng.integers(-1, W + 1) + 1) * half, int(2 * rng.integers(-1, H + 1) + 1) * half) for _ in range(n)]
            on_centres += 1
        elif trial % 2:                                  # f = 0: diagonals of the lattice pass through centres
            x, y, d = (int(v) for v in rng.integers(0, 5, 3))
            ring = [(x, y), (x + d + 2, y + d + 2), (x, y + d + 2)]
        else:
            ring = [(int(rng.integers(-2 * s, (W + 2) * s)), int(rng.integers(-2 * s, (H + 2) * s))) for _ in range(n)]
        rings = [ring, [(2 * s, 2 * s), (6 * s, 3 * s), (4 * s, 7 * s)]]
        got = F.fill(*F.table(rings, [1, 1]), H, W, f, None, max_objects=1)["labels"] > 0
        want = np.array([[F.inside_exact(rings, x, y, f) for x in range(W)] for y in range(H)])
        assert np.array_equal(got, want), (f, rings)
    assert f == 0 or on_centres == 20


def test_hand_built_cases_say_what_they_claim():
    for f in (0, 1, 4, 8):
        cases = K.hand_built(f)
        lim = 32768 << f
        assert max(abs(c) for v in cases["outside"][0] for p in v for c in p) == lim
        rings, ids, max_objects = cases["overlap"]
        out = F.fill(*F.table(rings, ids), K.HS, K.WS, f, None, max_objects)
        assert out["table"][3, 0] == 0 and out["table"][4, 0] == 25 * 40 and out["info"].tolist() == [0, 7, 7, 0]
    rings, ids, max_objects = K.hand_built(1)["strictness"]
    t = F.table(rings, ids)
    strict, loose = F.fill(*t, K.HS, K.WS, 1, None, max_objects), F.fill(*t, K.HS, K.WS, 1, None, max_objects, strict=False)
    assert strict["table"][0, 0] == 20 * 21 // 2 and loose["table"][0, 0] == 20 * 19 // 2, \
        "a centre on the diagonal is not strictly right of it: the edge is not counted and the pixel is inside"
    assert not np.array_equal(strict["labels"], loose["labels"])
    rings, ids, max_objects = K.hand_built(0)["stars_and_triangles"]
    t = F.table(rings, ids)
    assert not np.array_equal(F.fill(*t, K.HS, K.WS, 0, None, max_objects)["labels"], F.fill(*t, K.HS, K.WS, 0, None, max_objects, winding=True)["labels"])


# ------------------------------------------------------------------------------------------------------ vector labels
def _arrays(mask, connectivity=8):
    obj = O.objects(mask, connectivity=connectivity, max_objects=mask.size)
    out = R.outlines(obj["labels"], obj["counts"], connectivity, max_objects=mask.size, max_rings=mask.size, max_vertices=4 * mask.size)
    rows, ring_rows, written = int(obj["counts"][1]), int(out["counts"][1]), int(out["counts"][3])
    return obj, (obj["table"][:rows], out["rings"][:ring_rows], out["vertices"][:written])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_geojson_written_by_predict_scene_reads_back_to_the_labels(tmp_path, connectivity):
    from change3d_amd.scripts.predict_scene import polygons_geojson
    mask = K.masks(33, 41)["ring_with_holes"] | K.masks(33, 41)["diagonal"]
    obj, arrays = _arrays(mask, connectivity)
    doc, skipped = polygons_geojson(*arrays)
    assert not skipped and len(doc["features"]) == int(obj["counts"][1])
    path = tmp_path / "scene.geojson"
    path.write_text(json.dumps(doc))
    for f in (0, 4):
        rings, vertices, counts, id_cls = V.read_polygons(str(path), frac_bits=f)
        assert rings.dtype == vertices.dtype == counts.dtype == np.int32 and id_cls.dtype == np.uint8
        assert counts[0] == counts[1] == len(arrays[1]) and counts[2] == counts[3] == len(arrays[2]) and counts[4] == 0
        assert id_cls.tolist() == [int(c) for c in arrays[0][:, 5]]
        got = F.fill(rings, vertices, counts, 33, 41, f, id_cls, max_objects=len(id_cls))
        assert np.array_equal(got["labels"], obj["labels"]) and np.array_equal(got["table"][:, 0], arrays[0][:, 0])


XBD = {"features": {"lng_lat": [], "xy": [
    {"properties": {"feature_type": "building", "subtype": "no-damage", "uid": "a"}, "wkt": "POLYGON ((2 2, 10 2, 10 8, 2 8, 2 2))"},
    {"properties": {"feature_type": "building", "subtype": "destroyed", "uid": "b"},
     "wkt": "POLYGON ((10.0 2.0, 18.5 2.0, 18.5 8.0, 10.0 8.0, 10.0 2.0), (12 4, 14 4, 14 6, 12 6, 12 4))"},
    {"properties": {"feature_type": "building", "subtype": "minor-damage", "uid": "c"}, "wkt": "polygon((1.25e1 10,20 1.0E1,16 15.5,12.5 10))"},
    {"properties": {"feature_type": "building", "subtype": "un-classified", "uid": "d"}, "wkt": "POLYGON ((-5 12, 4 12, 4 30, -5 30, -5 12))"},
    {"properties": {"feature_type": "building", "subtype": "major-damage", "uid": "e"}, "wkt": "POLYGON Z ((30 30 0, 31 30 0, 31 31 0, 30 30 0))"},
    {"properties": {"feature_type": "building", "uid": "f"}, "wkt": "POLYGON ((6 12, 9 12, 9 15, 6 15, 6 12))"}]},
    "metadata": {"width": 24, "height": 20}}


def test_xbd_label_file(tmp_path):
    path = tmp_path / "scene.json"
    path.write_text(json.dumps(XBD))
    rings, vertices, counts, id_cls = V.read_polygons(str(path))
    assert id_cls.tolist() == [1, 4, 2, 1, 3, 1] and counts.tolist() == [7, 7, 26, 26, 0]
    assert rings[:, 0].tolist() == [1, 2, 2, 3, 4, 5, 6] and rings[:, 2].tolist() == [4, 4, 4, 3, 4, 3, 4]
    assert vertices[4:8].tolist() == [[160, 32], [296, 32], [296, 128], [160, 128]], "rounded to 1/16 pixel, the closing repeat dropped"
    got = F.fill(rings, vertices, counts, 20, 24, 4, id_cls, max_objects=6)
    labels = got["labels"]
    assert (labels[2:8, 2:10] == 1).all() and (labels[2:8, 10:18] [:, [0, 1, 4, 5, 6, 7]] == 2).all() and not labels[4:6, 12:14].any()
    assert labels[5, 18] == 2 and labels[5, 19] == 0, "the edge x = 18.5 runs through the centres of column 18: not strictly left, not counted"
    assert got["table"][:, 0].tolist() == [48, 50, got["table"][2, 0], 4 * 8, 0, 9] and got["table"][:, 5].tolist() == [1, 4, 2, 1, 3, 1]
    assert got["table"][3, 1:5].tolist() == [0, 12, 3, 19], "clipped by the scene"
    assert np.array_equal(got["cls_map"], np.where(labels > 0, id_cls[np.maximum(labels, 1) - 1], 0))
    # two buildings that share the edge x = 10 stay two objects; their raster is one component
    assert O.objects((labels > 0).astype(np.uint8))["counts"][0] < 5 == int((got["table"][:, 0] > 0).sum())


def test_parser_errors_name_the_feature(tmp_path):
    def read(doc):
        path = tmp_path / "bad.json"
        path.write_text(doc if isinstance(doc, str) else json.dumps(doc))
        return V.read_polygons(str(path))

    def xbd(k, **change):
        doc = json.loads(json.dumps(XBD))
        doc["features"]["xy"][k].update(change)
        return doc

    for doc, word in ((xbd(2, wkt="LINESTRING (0 0, 1 1)"), "feature 2"), (xbd(1, wkt="POLYGON ((0 0, 1 x, 1 1))"), "feature 1"),
                      (xbd(3, wkt="POLYGON ((0 0, 1 1, 1 0)) junk"), "feature 3"), (xbd(4, wkt=None), "feature 4"),
                      (xbd(0, properties={"subtype": "flattened"}), "feature 0"), (xbd(5, wkt="POLYGON ((0 0, 40000 0, 5 5))"), "feature 5"),
                      (xbd(2, wkt="POLYGON ((0 0, 1e999 0, 5 5))"), "feature 2"), (xbd(1, wkt="POLYGON ()"), "feature 1")):
        with pytest.raises(V.PolygonFileError, match=word):
            read(doc)
    point = {"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [[[0, 0], [4, 0], [4, 4]]]}, "properties": {}},
                                                       {"type": "Feature", "geometry": {"type": "Point", "coordinates": [1, 2]}, "properties": {}}]}
    with pytest.raises(V.PolygonFileError, match="feature 1"):
        read(point)
    point["features"][1] = {"type": "Feature", "geometry": {"type": "MultiPolygon", "coordinates": [[[[0, 0], [4, 0], [4, "4"]]]]}, "properties": {}}
    with pytest.raises(V.PolygonFileError, match="feature 1"):
        read(point)
    point["features"][1] = {"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [[[0, 0], [4, 0], [4, 4]]]}, "properties": {"cls": 300}}
    with pytest.raises(V.PolygonFileError, match="feature 1"):
        read(point)
    for doc in ("not json", {"type": "FeatureCollection"}, {"features": {"lng_lat": []}}):
        with pytest.raises(V.PolygonFileError):
            read(doc)
    with pytest.raises(ValueError):
        V.polygons_table([], frac_bits=9)
    multi = {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"cls": 3}, "geometry": {"type": "MultiPolygon", "coordinates": [
        [[[0, 0], [4, 0], [4, 4], [0, 4], [0, 0]]], [[[6, 0], [9, 0], [9, 3], [6, 0]], [[7, 1], [8, 1], [8, 2], [7, 1]]]]}}]}
    rings, vertices, counts, id_cls = read(multi)
    assert rings[:3, 0].tolist() == [1, 1, 1] and rings[:3, 2].tolist() == [4, 3, 3] and id_cls.tolist() == [3]
    empty = read({"type": "FeatureCollection", "features": []})
    assert empty[0].shape == (1, 8) and empty[1].shape == (1, 2) and empty[2].tolist() == [0, 0, 0, 0, 0] and len(empty[3]) == 0
    assert "fillPoly" in V.__doc__


# ------------------------------------------------------------------------------------------ the layers above, no device
def test_geojson_writer_takes_iou_and_keeps_drifted_objects_raw():
    import simplify_reference as S
    from change3d_amd.scripts.predict_scene import polygons_geojson
    mask = K.masks(33, 41)["blobs"]
    obj, raw = _arrays(mask)
    counts = np.array([len(raw[1]), len(raw[1]), len(raw[2]), len(raw[2]), 0], dtype=np.int32)
    simple = S.simplify(raw[1], raw[2], counts, S.tol2_q(1.0))
    simplified = (simple["rings"][:len(raw[1])], simple["vertices"][:int(simple["counts"][3])])
    rows = len(raw[0])
    assert rows >= 2
    plain, _ = polygons_geojson(*raw, simplified)
    iou = np.linspace(0.5, 1.0, rows)
    doc, _ = polygons_geojson(*raw, simplified, iou, None)
    assert [f["properties"]["iou"] for f in doc["features"]] == [round(float(v), 4) for v in iou]
    assert [f["geometry"] for f in doc["features"]] == [f["geometry"] for f in plain["features"]] and "iou" not in plain["features"][0]["properties"]
    guarded, _ = polygons_geojson(*raw, simplified, iou, 0.75)
    untouched, _ = polygons_geojson(*raw)
    for k, f in enumerate(guarded["features"]):
        want = plain if iou[k] > 0.75 else untouched
        assert f["geometry"] == want["features"][k]["geometry"]
        assert f["properties"]["vertices"] == (f["properties"]["vertices_raw"] if iou[k] <= 0.75 else plain["features"][k]["properties"]["vertices"])
    assert any(f["properties"]["vertices"] < f["properties"]["vertices_raw"] for f in guarded["features"])


def test_new_refusals_of_the_parser_and_of_predict():
    from change3d_amd.infer import SceneFill, SceneInferencer
    from change3d_amd.scripts.predict_scene import parse_args
    base = ["--weights", "w.pth", "--pre", "a.png", "--post", "b.png"]
    for extra in (["--simplify_check"], ["--objects", "--polygons", "--simplify_check"], ["--simplify_min_iou", "0.9"],
                  ["--objects", "--polygons", "--simplify", "1", "--simplify_min_iou", "1.5"], ["--task", "SCD", "--label_polygons", "x.json"],
                  ["--label_polygons", "x.json", "--label", "l.png"]):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
    args = parse_args(base + ["--objects", "--polygons", "--simplify", "1.5", "--simplify_min_iou", "0.9", "--label_polygons", "x.json"])
    assert args.simplify_check and args.simplify_min_iou == 0.9 and args.label_polygons == "x.json"
    assert not parse_args(base).simplify_check and parse_args(base).label_polygons == ""
    assert SceneFill._fields == ("labels", "table", "counts", "info", "match")

    class _Model:
        args = type("A", (), dict(in_height=64, in_width=64, num_class=1))()

        def eval(self):
            return self
    inf = SceneInferencer(_Model(), "bcd")
    with pytest.raises(ValueError, match="simplify_check"):
        inf.predict(np.zeros((64, 64, 6), np.uint8), objects=True, outlines=True, simplify_check=True)


def test_lib_declares_the_fill_entries():
    import ctypes as C
    from change3d_amd import _lib as L
    assert L.SIGNATURES["c3d_rings_fill"][1].count(C.c_void_p) == 12 and L.SIGNATURES["c3d_rings_fill"][1].count(C.c_int32) == 6
    assert L.SIGNATURES["c3d_rings_fill_ws_bytes"] == (C.c_int64, [C.c_int32] * 5)
    assert (L.FILL_ST_BAD_ID, L.FILL_ST_BAD_RING) == (F.ST_BAD_ID, F.ST_BAD_RING)
    assert L.FILL_ST_BAD_ID > L.SIMPLIFY_ST_BAD_INPUT and L.FILL_ST_BAD_ID & L.FILL_ST_BAD_RING == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "change3d_hip.h")).read()
    assert f"#define C3D_FILL_ST_BAD_ID {L.FILL_ST_BAD_ID}\n" in header and f"#define C3D_FILL_ST_BAD_RING {L.FILL_ST_BAD_RING}\n" in header
