"""`c3d_rings_regularize` in the layers above it: `predict(regularize=True)` against the op on `predict`'s own simplified rings
and hulls, its launch counts with and without `shapes=True`, `regularize_check=True` against fill and match done by hand, and
`predict_scene --regularize` in a child process on a small synthetic pair."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regular_reference as R  # noqa: E402

from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS, WS = 150, 170
HULL_LAUNCHES, REGULAR_LAUNCHES = 9, 5                      # as include/change3d_hip.h documents them


@pytest.fixture(scope="module")
def bcd_model():
    from test_scene_bda_gpu import _model
    return _model("bcd")


def _equal(a, b):
    """Two result tuples of predict, vertex rows past the written count aside."""
    assert len(a) == len(b)
    for p, q in zip(a, b):
        n = int(p.counts[3]) if hasattr(p, "vertices") else None   # SceneOutlines, SceneShapes, SceneRegular: counts[3] rows are written
        for x, y in zip(*(t if isinstance(t, tuple) else (t,) for t in (p, q))):
            if x is None:
                assert y is None
            elif isinstance(x, tuple):                       # the match of a SceneFill
                assert all(torch.equal(s, t) for s, t in zip(x, y))
            elif n is not None and x.dim() == 2 and x.shape[-1] == 2:
                assert torch.equal(x[:n], y[:n])
            else:
                assert torch.equal(x, y)


def test_predict_with_regularize_equals_the_op_on_its_own_rings(bcd_model):
    from change3d_amd.infer import SceneFill, SceneInferencer, SceneRegular, SceneShapes
    from test_scene_bda_gpu import _scene
    scene = _scene(70, 90, 2)
    inf = SceneInferencer(bcd_model, "bcd", stride=32, batch=5)
    for extra in (dict(), dict(shapes=True), dict(split=2.0), dict(simplify_check=True, shapes=True)):
        today = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0, **extra)
        before = ops.launch_count()
        off = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0, regularize=False, **extra)
        plain = ops.launch_count() - before
        before = ops.launch_count()
        out = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0, regularize=True, **extra)
        added = REGULAR_LAUNCHES + (0 if extra.get("shapes") else HULL_LAUNCHES)   # the hull call is shared with shapes=True
        assert ops.launch_count() - before == plain + added
        assert len(today) == len(off) == len(out) - 1 and isinstance(out[-1], SceneRegular)
        _equal(today, off)
        _equal(today, out[:-1])
        objects, raw, simple, regular = out[2], out[3], out[4], out[-1]
        hull = ops.rings_hull(*raw, max_objects=objects.table.shape[0])
        if extra.get("shapes"):
            assert isinstance(out[-2], SceneShapes) and torch.equal(out[-2].hulls, hull[0]) and torch.equal(out[-2].rects, hull[2])
        by_hand = ops.rings_regularize(*simple, *hull, frac_bits=4)
        written = int(by_hand[2][3])
        assert torch.equal(regular.rings, by_hand[0]) and torch.equal(regular.counts, by_hand[2])
        assert torch.equal(regular.vertices[:written], by_hand[1][:written])
        want = R.regularize(*(t.cpu().numpy() for t in tuple(simple) + tuple(hull)), 4)
        assert np.array_equal(regular.rings.cpu().numpy(), want["rings"]) and np.array_equal(regular.counts.cpu().numpy(), want["counts"])
        assert np.array_equal(regular.vertices[:written].cpu().numpy(), want["vertices"][:written])
        assert int(regular.counts[4]) == 0 and int(regular.counts[1]) == int(simple.counts[1]) > 0
    # the check: fill at 1/16 px and match, by hand
    before = ops.launch_count()
    out = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0, regularize=True)
    unchecked = ops.launch_count() - before
    before = ops.launch_count()
    checked = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0, regularize=True, regularize_check=True)
    with_check = ops.launch_count() - before
    assert len(checked) == len(out) + 1 and isinstance(checked[-1], SceneFill) and isinstance(checked[-2], SceneRegular)
    _equal(out, checked[:-1])
    objects, fill = checked[2], checked[-1]
    before = ops.launch_count()
    f_labels, f_table, f_counts, _, _, f_info = ops.rings_fill(*checked[-2], 70, 90, frac_bits=4, max_objects=objects.table.shape[0])
    match = ops.objects_match(objects.labels, objects.table, objects.counts, f_labels, f_table, f_counts, n_cls=1, iou_thr=0.5)
    assert with_check - unchecked == ops.launch_count() - before
    assert torch.equal(fill.labels, f_labels) and torch.equal(fill.table, f_table) and torch.equal(fill.counts, f_counts)
    assert torch.equal(fill.info, f_info) and all(torch.equal(s, t) for s, t in zip(fill.match, match)) and int(f_info[0]) == 0
    before = ops.launch_count()
    for bad in (dict(regularize=True), dict(simplify=1.0, regularize_check=True), dict(regularize=True, regularize_check=True)):
        with pytest.raises(ValueError):
            inf.predict(scene, objects=True, outlines=True, **bad)
    assert ops.launch_count() == before, "refused before anything is enqueued"


def _run(tmp, name, extra):
    from test_scene_bda_gpu import T
    cmd = [sys.executable, "-m", "change3d_amd.scripts.predict_scene", "--task", "BCD", "--weights", str(tmp / "best_model.pth"), "--pre",
           str(tmp / "a.png"), "--post", str(tmp / "b.png"), "--stride", "32", "--batch_size", "32", "--act_dtype", "f32", "--in_height", str(T),
           "--in_width", str(T), "--pretrained", "/nonexistent", "--out_dir", str(tmp / name)] + extra
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    return done.stdout.splitlines()


LINE = r"regularize: objects = (\d+) regular = (\d+) fallback = (\d+) iou_mean = ([\d.]+) iou_min = ([\d.]+)"


def test_predict_scene_regularize_end_to_end_in_a_child_process(bcd_model, tmp_path):
    from PIL import Image
    from test_scene_bda_gpu import _scene
    tmp = tmp_path
    scene = _scene(HS, WS, 6)
    Image.fromarray(scene[:, :, 0:3]).save(tmp / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp / "b.png")
    torch.save(bcd_model.state_dict(), tmp / "best_model.pth")
    base = ["--objects", "--polygons", "--simplify", "1", "--max_rings", str(HS * WS), "--max_vertices", str(4 * HS * WS), "--min_area", "4"]
    plain = _run(tmp, "plain", base)
    lines = _run(tmp, "regular", base + ["--regularize"])
    fallen = _run(tmp, "fallback", base + ["--regularize", "--regularize_min_iou", "1"])
    main = (tmp / "plain" / "objects" / "scene.geojson").read_bytes()
    for name, out in (("regular", lines), ("fallback", fallen)):
        assert [ln.replace(str(tmp / name), str(tmp / "plain")) for ln in out[:-1]] == plain and re.fullmatch(LINE, out[-1])
        assert sorted(os.listdir(tmp / name / "objects")) == ["scene.csv", "scene.geojson", "scene.regular.geojson"]
        assert (tmp / name / "objects" / "scene.geojson").read_bytes() == main
        assert (tmp / name / "objects" / "scene.csv").read_bytes() == (tmp / "plain" / "objects" / "scene.csv").read_bytes()
    before = json.loads(main)["features"]
    feats = json.loads((tmp / "regular" / "objects" / "scene.regular.geojson").read_text())["features"]
    assert len(feats) == len(before) >= 1
    squared = 0
    for f, b in zip(feats, before):
        p = dict(f["properties"])
        regular = p.pop("regular")
        assert p == b["properties"] and isinstance(regular, bool) and len(f["geometry"]["coordinates"]) == len(b["geometry"]["coordinates"])
        if not regular:
            assert f["geometry"] == b["geometry"]
            continue
        squared += 1
        for ring in f["geometry"]["coordinates"]:
            assert ring[0] == ring[-1] and len(ring) >= 5 and len(ring) % 2 == 1
            assert all(float(c * 16).is_integer() for v in ring for c in v), "coordinates are sixteenths of a pixel"
    m = re.fullmatch(LINE, lines[-1])
    assert [int(m.group(k)) for k in (1, 2, 3)] == [len(feats), squared, len(feats) - squared]
    feats = json.loads((tmp / "fallback" / "objects" / "scene.regular.geojson").read_text())["features"]
    m = re.fullmatch(LINE, fallen[-1])                       # no IoU is above 1: every object falls back
    assert [int(m.group(k)) for k in (1, 2, 3)] == [len(before), 0, len(before)] and 0 <= float(m.group(5)) <= float(m.group(4)) <= 1
    for f, b in zip(feats, before):
        assert f["geometry"] == b["geometry"] and f["properties"]["regular"] is False and 0 <= f["properties"]["iou"] <= 1


def test_regularize_flag_needs_polygons_and_simplify(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    common = ["--weights", "w.pth", "--pre", "a.png", "--post", "b.png", "--objects"]
    for extra in (["--regularize"], ["--polygons", "--regularize"], ["--polygons", "--simplify", "1", "--regularize_min_iou", "0.5"]):
        with pytest.raises(SystemExit):
            parse_args(common + extra)
        assert "--regularize" in capsys.readouterr().err
    assert parse_args(common + ["--polygons", "--simplify", "1", "--regularize", "--regularize_min_iou", "0.5"]).regularize
