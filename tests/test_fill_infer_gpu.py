"""`c3d_rings_fill` in the layers above it: `predict(simplify=tol, simplify_check=True)` against the ops chained by hand, and
`predict_scene` in child processes on a synthetic 300 x 280 pair -- `--label_polygons` against the score line computed from the
restatements, two touching labelled squares that stay two ground-truth objects where the raster joins them, and
`--simplify_min_iou`, which leaves the objects that drifted on their raw vertices."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_reference as F  # noqa: E402
import objects_match_reference as M  # noqa: E402
import objects_reference as O  # noqa: E402

from change3d_amd import ops, vector_labels  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS, WS = 300, 280


@pytest.fixture(scope="module")
def bcd_model():
    from test_scene_bda_gpu import _model
    return _model("bcd")


def test_predict_with_simplify_check_equals_the_ops_chained_by_hand(bcd_model):
    from change3d_amd.infer import SceneFill, SceneInferencer, SceneOutlines
    from test_scene_bda_gpu import _scene
    scene = _scene(70, 90, 2)
    inf = SceneInferencer(bcd_model, "bcd", stride=32, batch=5)
    today = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0)
    off = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0, simplify_check=False)
    out = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0, simplify_check=True)
    assert len(today) == len(off) == 5 and len(out) == 6 and isinstance(out[4], SceneOutlines) and isinstance(out[5], SceneFill)
    n = int(today[4].counts[3])
    for a, b, c in zip(today, off, out):                    # exactly today's tuple, and the same tuple in front of the SceneFill
        for x, y, z in zip(*(t if isinstance(t, tuple) else (t,) for t in (a, b, c))):
            if x is None:
                assert y is None and z is None
            else:
                cut = (lambda t: t[:n]) if x.dim() == 2 and x.shape[-1] == 2 else (lambda t: t)
                assert torch.equal(cut(x), cut(y)) and torch.equal(cut(x), cut(z))
    objects, simple, fill = out[2], out[4], out[5]
    labels, table, counts, _, _, info = ops.rings_fill(*simple, 70, 90)
    match = ops.objects_match(objects.labels, objects.table, objects.counts, labels, table, counts, n_cls=1, iou_thr=0.5)
    assert torch.equal(fill.labels, labels) and torch.equal(fill.table, table) and torch.equal(fill.counts, counts) and torch.equal(fill.info, info)
    assert all(torch.equal(a, b) for a, b in zip(fill.match, match))
    rows = int(objects.counts[1])
    assert rows > 0 and fill.info.tolist() == [0, int(simple.counts[1]), int(fill.counts[0]), 0] and int(fill.counts[0]) <= rows
    want = F.fill(*(t.cpu().numpy() for t in simple), 70, 90, 0, None, max_objects=table.shape[0])
    assert np.array_equal(labels.cpu().numpy(), want["labels"]) and np.array_equal(table.cpu().numpy(), want["table"])
    exact = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=0.0, simplify_check=True)
    assert torch.equal(exact[5].labels, exact[2].labels), "at tolerance 0 the filled polygons are the objects"
    assert (exact[5].match[0][:rows, 0] == torch.arange(1, rows + 1, device=labels.device)).all()
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, outlines=True, simplify_check=True)


def _run(tmp, name, extra):
    from test_scene_bda_gpu import T
    cmd = [sys.executable, "-m", "change3d_amd.scripts.predict_scene", "--task", "BCD", "--weights", str(tmp / "best_model.pth"), "--pre",
           str(tmp / "a.png"), "--post", str(tmp / "b.png"), "--stride", "32", "--batch_size", "32", "--act_dtype", "f32", "--in_height", str(T),
           "--in_width", str(T), "--pretrained", "/nonexistent", "--out_dir", str(tmp / name), "--objects"] + extra
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    return done.stdout.splitlines()


@pytest.fixture(scope="module")
def scene_dir(bcd_model, tmp_path_factory):
    """The pair, the weights and a polygon label file: the outlines of the model's own objects as `--polygons` writes them (so
    that some objects match), then two squares that share an edge and a triangle on the half-pixel lattice."""
    from PIL import Image
    from change3d_amd.infer import SceneInferencer
    from change3d_amd.scripts.predict_scene import polygons_geojson
    from test_scene_bda_gpu import _scene
    tmp = tmp_path_factory.mktemp("fill_scene")
    scene = _scene(HS, WS, 6)
    Image.fromarray(scene[:, :, 0:3]).save(tmp / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp / "b.png")
    torch.save(bcd_model.state_dict(), tmp / "best_model.pth")
    out = SceneInferencer(bcd_model, "bcd", stride=32, batch=32).predict(scene, objects=True, min_area=30, outlines=True,
                                                                         max_rings=HS * WS, max_vertices=4 * HS * WS)
    rows, ring_rows, written = int(out[2].counts[1]), int(out[3].counts[1]), int(out[3].counts[3])
    doc, skipped = polygons_geojson(out[2].table[:rows].cpu().numpy(), out[3].rings[:ring_rows].cpu().numpy(), out[3].vertices[:written].cpu().numpy())
    assert not skipped
    doc["features"] = doc["features"][:40]
    for ring in ([[100, 100], [130, 100], [130, 130], [100, 130], [100, 100]], [[130, 100], [160, 100], [160, 130], [130, 130], [130, 100]],
                 [[200.5, 20.5], [260, 40.5], [220.5, 90], [200.5, 20.5]]):
        doc["features"].append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [ring]}, "properties": {"cls": 1}})
    (tmp / "gt.geojson").write_text(json.dumps(doc))
    return tmp


def _object_line(stdout):
    lines = [ln for ln in stdout if ln.startswith("objects:")]
    assert len(lines) == 1, stdout[-8:]
    return lines[0]


def test_predict_scene_scores_polygon_labels_in_a_child_process(scene_dir):
    from PIL import Image
    from change3d_amd.object_metrics import scores_from_totals
    tmp = scene_dir
    rings, vertices, counts, id_cls = vector_labels.read_polygons(str(tmp / "gt.geojson"))
    K = len(id_cls)
    gt = F.fill(rings, vertices, counts, HS, WS, 4, id_cls, max_objects=K)
    assert gt["info"].tolist() == [0, int(counts[1]), K, 0] and (gt["table"][K - 3:, 0] == [900, 900, gt["table"][K - 1, 0]]).all()
    Image.fromarray(gt["mask"] * 255).save(tmp / "gt.png")
    poly = _run(tmp, "poly", ["--label_polygons", str(tmp / "gt.geojson"), "--boundary", "2"])
    raster = _run(tmp, "raster", ["--label", str(tmp / "gt.png"), "--boundary", "2"])
    # the line the child must print, from the restatements: its own mask labelled on the host, joined to the filled polygons
    mask = (np.asarray(Image.open(tmp / "poly" / "scene.png")) > 0).astype(np.uint8)
    assert np.array_equal(mask, (np.asarray(Image.open(tmp / "raster" / "scene.png")) > 0).astype(np.uint8))
    pred = O.objects(mask, connectivity=8, max_objects=65536)
    res = M.match(pred["labels"], pred["table"], pred["counts"], gt["labels"], gt["table"], gt["counts_obj"], n_cls=1, iou_thr=0.5)
    s = scores_from_totals([int(v) for v in res["counts"][1:4]] + [int(res["counts"][0]), 0] + [0], res["sum_iou"], 1)
    want = (f"objects: tp = {s['tp']} fp = {s['fp']} fn = {s['fn']} precision = {s['precision']:.4f} recall = {s['recall']:.4f} "
            f"f1 = {s['f1']:.4f} sq = {s['sq']:.4f} rq = {s['rq']:.4f} pq = {s['pq']:.4f}")
    assert _object_line(poly) == want
    assert s["tp"] > 0 and s["tp"] + s["fn"] == K, "one ground-truth object per feature"
    # the raster of the same labels joins the two squares (and whatever else touches): fewer ground-truth objects
    joined = int(O.components(gt["mask"], 8).max())
    tp, fn = (int(v) for v in re.search(r"tp = (\d+) fp = \d+ fn = (\d+)", _object_line(raster)).groups())
    assert tp + fn == joined < K
    # pixel scores and boundary scores read the filled mask: the same lines on both paths
    same = [ln for ln in poly if ln.startswith(("boundary:", "Test:"))]
    assert len(same) == 2 and same == [ln for ln in raster if ln.startswith(("boundary:", "Test:"))]
    rows = (tmp / "poly" / "objects" / "scene.match.csv").read_text().split("# gt\n")[1].splitlines()
    assert len(rows) - 1 == K


def test_predict_scene_simplify_min_iou_in_a_child_process(bcd_model, scene_dir):
    from change3d_amd.infer import SceneInferencer
    from test_scene_bda_gpu import _scene
    tmp, tol = scene_dir, 1.5
    out = SceneInferencer(bcd_model, "bcd", stride=32, batch=32).predict(_scene(HS, WS, 6), objects=True, outlines=True, simplify=tol,
                                                                         simplify_check=True)
    rows = int(out[2].counts[1])
    m = out[5].match[0][:rows].cpu().numpy().astype(np.int64)
    iou = np.where(m[:, 2] > 0, m[:, 1] / np.maximum(m[:, 2], 1), 0.0)
    area = out[2].table[:rows, 0].cpu().numpy()
    thin = int(np.argmin(np.where(area >= 4, iou, 2.0)))     # the object the simplification hurt most: F lies just above its IoU
    bound = round(float(iou[thin]) + 0.0005, 4)
    assert 0 < (iou <= bound).sum() < rows, "some objects drift past the bound, others do not"
    raw = _run(tmp, "raw", ["--polygons"])
    guard = _run(tmp, "guard", ["--polygons", "--simplify", str(tol), "--simplify_min_iou", str(bound)])
    docs = {k: json.loads((tmp / k / "objects" / "scene.geojson").read_text())["features"] for k in ("raw", "guard")}
    assert len(docs["raw"]) == len(docs["guard"]) == rows and not [ln for ln in raw if ln.startswith("simplify:")]
    kept_raw = simplified = 0
    for f, g in zip(docs["guard"], docs["raw"]):
        p = f["properties"]
        if p["id"] == thin + 1:
            assert f["geometry"] == g["geometry"] and p["iou"] <= bound, "the chosen object keeps its raw vertices in every ring"
        if p["iou"] < bound - 1e-4 or p["id"] == thin + 1:   # the property is rounded to four places: stay clear of the bound
            assert f["geometry"] == g["geometry"] and p["vertices"] == p["vertices_raw"]
            kept_raw += 1
        elif p["vertices"] < p["vertices_raw"]:
            simplified += 1
    assert kept_raw > 0 and simplified > 0
    line = [ln for ln in guard if ln.startswith("simplify:")]
    assert len(line) == 1
    got = dict(re.findall(r"(\w+) = ([\d.]+)", line[0]))
    ious = [f["properties"]["iou"] for f in docs["guard"]]
    assert float(got["tol"]) == tol and int(got["objects"]) == rows and int(got["kept"]) <= rows
    assert int(got["vanished"]) == int((out[5].table[:rows, 0] == 0).sum()) and int(got["kept"]) == int((m[:, 0] == np.arange(1, rows + 1)).sum())
    assert abs(float(got["iou_mean"]) - float(np.mean(iou))) < 1e-4 and abs(float(got["iou_min"]) - min(ious)) < 1e-4
